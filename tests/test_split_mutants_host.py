"""The mutant table of the split-kernel tests.  No GPU: tests/split_harness.py restates dwxh_split_kernel and dx1w1_split_kernel piece by
piece, and a MUTANT is that restatement with one piece product lost, a third piece zero or taken from a neighbouring element, or a
two-piece cut -- what an edit that moves the piece reads or the MFMAs of those kernels can get wrong.  Asserted here:
  * the probe construction: both cuts return exactly the three pieces a probe value was built from, the six products sum without any
    rounding in every order to float32(x) * float32(y), and losing any one product moves the value by at least 4e-7 of it;
  * the ownership maps of the GPU probe tests own every k, every row slot of both LDS buffers (dx1w1) / of the ring of four sub-chunks
    (dwxh), every slot of a piece's plane, and the boundary rows the GPU tests' docstrings name;
  * the unmutated restatement reproduces the probes' expected arrays bit for bit and EVERY mutant fails to (item "probe" of the table);
  * on the GPU tests' own random inputs (H = 128, the smaller N) the old bound |err| <= 2e-5 max|ref64| lets the third-order mutants
    through, the unmutated restatement meets every accuracy criterion the GPU tests assert (split_harness.RATIO / MEAN_C, set from the
    f32 kernels' errors measured on an MI355X for these very cases), and every mutant a criterion claims misses it.
The table is printed (pytest -s)."""
import itertools

import numpy as np
import pytest

from tests import split_harness as sh
from tests import test_dwxh_split_gpu as tw
from tests import test_dx1w1_split_gpu as tx

H = 128
HOST_SIZES = {'dwxh': (1, 21, 349, 409), 'dx1w1': (1, 21, 160, 161, 349)}


def test_harness_restates_the_gpu_tests_shapes():
    assert sh.WIDTHS == tw.WIDTHS == tx.WIDTHS and sh.SIZES == {'dwxh': tw.SIZES, 'dx1w1': tx.SIZES}
    assert (sh.G, sh.S, sh.L, sh.NZ, sh.SMAX) == (tw.G, tw.S, tw.L, tw.NZ, tx.SMAX) and (tx.G, tx.S) == (sh.G, sh.S)
    for Hh in sh.WIDTHS:
        for a, b in zip(sh.structure(Hh), tx._structure(Hh)):
            assert np.array_equal(a, b)


def test_probe_values_have_the_same_pieces_under_both_cuts_and_exact_products():
    rng = np.random.RandomState(0)
    x, y = sh.probe_values(rng, (20000,)), sh.probe_values(rng, (20000,))
    for v in (x, y):
        t, r = sh.dx_cut8(v), sh.put(v)
        for a, b in zip(t, r):
            assert np.array_equal(a, b)
            assert ((a.view(np.uint32) & np.uint32(0xffff)) == 0).all()
            assert (np.abs(a) >= 2.0 ** -126).all()                            # normal bf16 values: flushing plays no role
        assert np.array_equal(t[0].astype(np.float64) + t[1] + t[2], v.astype(np.float64))
        m = np.abs(t[0]) / 2.0 ** np.floor(np.log2(np.abs(t[0])))
        assert set(np.unique(m)) == {1.0, 1.5}                                 # m1 = 2 or 3
        assert (np.abs(t[1]) >= np.abs(t[0]) * 2.0 ** -11).all() and (np.abs(t[2]) >= np.abs(t[1]) * 2.0 ** -11).all()
    px, py = sh.put(x), sh.dx_cut8(y)
    want = x * y                                                               # f32 x f32, correctly rounded
    prods = [px[i - 1] * py[j - 1] for i, j in sh.SIX]
    for p, (i, j) in zip(prods, sh.SIX):
        assert np.array_equal(p.astype(np.float64), px[i - 1].astype(np.float64) * py[j - 1].astype(np.float64))
    assert np.array_equal(sum(p.astype(np.float64) for p in prods), want.astype(np.float64))
    for order in itertools.permutations(range(6)):                             # every order, f32 at every step
        acc = np.zeros_like(want)
        exact = np.zeros(len(want))
        for o in order:
            acc = acc + prods[o]
            exact = exact + prods[o].astype(np.float64)
            assert np.array_equal(acc.astype(np.float64), exact), order
        assert np.array_equal(acc, want)
    for p in prods:                                                            # any single product lost: several ulps
        assert (np.abs(p) >= 4e-7 * np.abs(want)).all() and (np.abs(p) >= 3 * np.spacing(np.abs(want))).all()


def _position(splits, rows):
    n0 = np.array([a for a, _ in splits])
    return rows - n0[np.searchsorted(n0, rows, side='right') - 1]


def test_probe_ownership_covers_every_slot_and_boundary():
    # dx1w1: a chunk is 32 rows, two LDS buffers -> position % 64 = (buffer, row slot); the plane slot is (row slot, k)
    cov = np.zeros((64, sh.NZ), bool)
    for Hh in sh.WIDTHS:
        kcov = np.zeros((Hh, sh.NZ), bool)
        for N in sh.SIZES['dx1w1']:
            splits = sh.dx1w1_splits(N, sh.S)
            seen, qs = set(), set()
            for q0, boundary, seed in sh.probe_calls('dx1w1', Hh, N):
                *_, owner, ks = sh.dx1w1_probe(Hh, N, sh.G, sh.S, q0, boundary, seed)
                assert (0 <= owner).all() and (owner < N).all()
                assert not np.array_equal(owner[0], owner[1]) or N == 1        # different probes per tower
                assert not np.array_equal(ks[0], ks[1])
                for g in range(sh.G):
                    assert len(set(ks[g])) == Hh
                    cov[_position(splits, owner[g]) % 64, ks[g]] = True
                    kcov[np.arange(Hh), ks[g]] = True
                    seen |= set(owner[g])
                if not boundary:
                    assert q0 not in qs
                    qs.add(q0)
            assert set(sh.boundary_rows(splits)) <= seen, (Hh, N)              # first and last row of every split
            if N == 349:
                assert splits[3] == (288, 61) and 348 in seen and (348 - 288) % 32 == 28        # the clamped tail ends inside row tile 1
            if N == 161:
                assert splits[2] == (128, 33) and 160 in seen                  # a clamped chunk of one row
        assert kcov.any(0).all(), Hh                                           # every k position 0 .. 255
    assert cov.all(), int((~cov).sum())
    # dwxh: a sub-chunk is 16 rows, a ring of four -> position % 64 = (ring slot, row slot); the plane slot is (row slot, feature)
    for Hh in sh.WIDTHS:
        F = Hh + sh.L
        cov = np.zeros((64, F), bool)
        for N in sh.SIZES['dwxh']:
            splits = sh.dwxh_splits(N, sh.S)
            seen = set()
            for q0, boundary, seed in sh.probe_calls('dwxh', Hh, N):
                *_, owner = sh.dwxh_probe(Hh, N, sh.G, sh.S, q0, boundary, seed)
                assert (owner < N).all() and not np.array_equal(owner[0], owner[1])
                for g in range(sh.G):
                    f = np.nonzero(owner[g] >= 0)[0]
                    cov[_position(splits, owner[g, f]) % 64, f] = True
                    seen |= set(owner[g, f])
            assert set(sh.boundary_rows(splits)) <= seen, (Hh, N)
            if N == 409:
                assert splits[4] == (328, 81) and 408 in seen and 80 % 16 == 0             # the single-row last step
            if N == 349:
                assert splits[4] == (280, 69) and 348 in seen
        assert cov.reshape(4, 16, F).any(0).all(), Hh                          # every slot of a piece's plane
        assert cov.any(1).all(), Hh                                            # every row slot of every sub-chunk of the ring
        # (dZ is dense in this probe: every k position 0 .. 255 of every row carries a product)


def _probe_outputs(kernel, Hh, N, call, mutant):
    q0, boundary, seed = call
    if kernel == 'dwxh':
        X1, Hp, dZ, exp, owner = sh.dwxh_probe(Hh, N, sh.G, sh.S, q0, boundary, seed)
        return sh.dwxh_restated(X1, Hp, dZ, mutant)[:, :Hh + sh.L].astype(np.float32), exp
    dZ, X1, Wx, obs, exp, owner, ks = sh.dx1w1_probe(Hh, N, sh.G, sh.S, q0, boundary, seed)
    return sh.dx1w1_restated(dZ, X1, Wx, obs, sh.structure(Hh)[2], mutant).astype(np.float32), exp


@pytest.mark.parametrize('kernel', ['dwxh', 'dx1w1'])
def test_probes_pass_the_restatement_and_kill_every_mutant(kernel):
    """One ownership map and the boundary map of (H = 128, N = 21) and (H = 128, N = 349)"""
    for N in (21, 349):
        calls = sh.probe_calls(kernel, H, N)
        for call in (calls[0], calls[-1]):
            out, exp = _probe_outputs(kernel, H, N, call, sh.UNMUTATED)
            assert np.array_equal(out, exp), (kernel, N, call)
            for name, mutant in sh.MUTANTS.items():
                out, exp = _probe_outputs(kernel, H, N, call, mutant)
                wrong = float((out != exp).mean())
                print('%s N=%d q0=%d %-28s: %5.1f %% of the probe entries differ' % (kernel, N, call[0], name, 100 * wrong))
                assert wrong > 0.2, (kernel, N, call, name, wrong)


def _random_cases(kernel):
    """(N, kind, float64 reference, per-entry sum of |terms|, mutant -> restated output) on the GPU tests' own inputs and seeds at H = 128"""
    for N in HOST_SIZES[kernel]:
        rng = np.random.RandomState(1000 * H + N)
        for kind in 'abcd':
            if kernel == 'dwxh':
                host = tw._inputs(kind, H, N, rng)
                ref, mag = sh.dwxh_ref64(*host)
                assert np.abs(ref - tw._ref64(*host)).max() <= 1e-12 * np.abs(ref).max()      # the GPU test's own reference
                yield N, kind, ref, mag, (lambda m, host=host: sh.dwxh_restated(*host, m))
            else:
                host = tx._inputs(kind, H, N, rng)
                mask = sh.structure(H)[2]
                ref, mag = sh.dx1w1_ref64(*host, mask)
                assert np.abs(ref - tx._ref64(*host, mask)).max() <= 1e-12 * np.abs(ref).max()
                yield N, kind, ref, mag, (lambda m, host=host, mask=mask: sh.dx1w1_restated(*host, mask, m))


def test_thresholds_follow_the_rule():
    """threshold = the geometric mean of the two measured sides, adopted only with a factor 2 on each: never a number of its own"""
    for un, mu, thr in list(sh.RATIO.values()) + list(sh.MEAN_C.values()):
        if mu / un >= 4:
            assert thr is not None and abs(thr - np.sqrt(un * mu)) <= 0.006 and thr >= 2 * un and mu >= 2 * thr, (un, mu, thr)
        else:
            assert thr is None, (un, mu, thr)
    # the floor: the max ratio on kinds a and d holds for every tensor of both kernels that carries a piece product
    for kernel, names in (('dwxh', ('dWx', 'dWh')), ('dx1w1', ('dW1', 'db1'))):
        for kind in 'ad':
            assert {t for _, t, _, _, _ in sh.accuracy_criteria(kernel, kind)} == set(names)
        assert not sh.accuracy_criteria(kernel, 'b')


@pytest.mark.parametrize('kernel', ['dwxh', 'dx1w1'])
def test_mutant_table_on_the_gpu_tests_random_inputs(kernel):
    names = [t for t, _, _ in sh.tensors(kernel, H) if t != 'dbl']
    passes_old = {name: [0, 0] for name in sh.MUTANTS}                         # cases that meet 2e-5, cases
    best = {}                                                                  # (criterion, tensor, kind, mutant) -> largest ratio
    killed = {name: set() for name in sh.MUTANTS}
    for N, kind, ref, mag, restated in _random_cases(kernel):
        out = restated(sh.UNMUTATED)
        e0 = sh.errors(kernel, H, out, ref)
        assert all(e0[t][0] <= tw.BOUND for t in e0), (kernel, N, kind, e0)
        # the three products the kernels leave out: |a2 b3| + |a3 b2| + |a3 b3| <= (2^-8 2^-15 + 2^-16 2^-7 + 2^-31) |a b| < 2^-21 |a b|
        # with the truncating cut's piece sizes (the rounding cut's are half of them)
        assert (np.abs(out - ref) <= 2.0 ** -21 * mag).all(), (kernel, N, kind)
        if kind != 'b':
            f32 = sh.F32_MEASURED[(kernel, N, kind)]
            assert not sh.accuracy_failures(kernel, kind, e0, f32), (kernel, N, kind, sh.accuracy_failures(kernel, kind, e0, f32))
        for name, mutant in sh.MUTANTS.items():
            e = sh.errors(kernel, H, restated(mutant), ref)
            ok = all(e[t][0] <= tw.BOUND for t in names)
            passes_old[name][0] += ok
            passes_old[name][1] += 1
            if not ok:
                killed[name].add('2e-5 bound')
            if kind != 'b':
                for crit, t, i, thr, claims in sh.accuracy_criteria(kernel, kind):
                    key = (crit, t, kind, name)
                    best[key] = max(best.get(key, 0.0), e[t][i] / f32[t][i])
                    if e[t][i] > thr * f32[t][i]:
                        killed[name].add('%s %s (%s)' % (crit, t, kind))
    # why the new criteria exist: the old bound alone sees the second-order products and lets the third-order mutants through
    for name in sh.MUTANTS:
        ok, n = passes_old[name]
        print('%-6s %-28s meets the 2e-5 bound in %2d of %2d cases; killed by: probes%s'
              % (kernel, name, ok, n, ''.join(', ' + k for k in sorted(killed[name]))))
        if name in sh.THIRD_ORDER:
            assert ok >= 0.9 * n, (kernel, name, ok, n)
        else:
            assert ok == 0, (kernel, name, ok, n)
    # every criterion kills every mutant it claims, with the factor 2 to spare, and the recorded mutant side is what this run finds
    for kind in 'acd':
        for crit, t, i, thr, claims in sh.accuracy_criteria(kernel, kind):
            worst = min(best[(crit, t, kind, name)] for name in claims)
            rec = (sh.RATIO[(kernel, t, kind)] if i == 0 else sh.MEAN_C[(kernel, t)])[1]
            assert abs(worst - rec) <= 0.02 * rec, (kernel, crit, t, kind, worst, rec)
            for name in claims:
                assert best[(crit, t, kind, name)] >= 2 * thr, (kernel, crit, t, kind, name, best[(crit, t, kind, name)], thr)
                assert '%s %s (%s)' % (crit, t, kind) in killed[name]
    for name in sh.THIRD_ORDER:                                                # no third-order mutant survives the accuracy criteria
        assert any(k.startswith('max ratio') for k in killed[name]), (kernel, name, killed[name])


def test_harness_cuts_are_the_cuts_of_the_two_host_restatements():
    """one restatement per device function: dx_cut8 == tests/test_dx1w1_split_host.cut3, put == tests/test_dwxh_split_host.split3"""
    import torch
    from tests.test_dwxh_split_host import split3
    from tests.test_dx1w1_split_host import cut3
    rng = np.random.RandomState(3)
    v = (rng.randn(50000) * np.exp(3 * rng.randn(50000))).astype(np.float32)
    v[:4] = (0.0, -0.0, 1 + 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -16))        # zeros and ties of the rounding cut
    for a, b in zip(sh.dx_cut8(v), cut3(v)):
        assert np.array_equal(a, b)
    for a, b in zip(sh.put(v), split3(torch.from_numpy(v.copy()))):
        assert np.array_equal(a, b.float().numpy())
