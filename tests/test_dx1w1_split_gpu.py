"""dx1w1_split_kernel (the first-layer pass of the LSTM update with dX1 = dZ Wx^T on the bf16 matrix cores, both operands cut into three bf16
pieces, six products) and the exact-f32 dx1w1_kernel2 through the test entry tsc_dx1w1_f32, against a float64 NumPy reference of the same
inputs:  dX1 = (dZ Wx^T) * [X1 > 0],  dW1 = obs^T dX1 inside the block structure of the first layer,  db1 = colsum(dX1).

Shapes: G = 2 towers (one agent), S = 5 row splits, every fused width H = 224 / 192 / 160 / 128, SMAX = 40 (three feature tiles, the last
half empty), N at every boundary of the 32-row chunk loop (split_rows rounds a split to 32 rows; a chunk runs unclamped while its successor
is whole, i.e. row + 64 <= end of the split; tests/test_dx1w1_split_host.py counts the same):
    N = 1      one row, four empty splits
    N = 21     one split of 21 rows, four empty ones
    N = 160    every split is exactly one clamped chunk: the plain loop is never entered
    N = 161    splits of 64 / 64 / 33: one plain chunk + a clamped one; a clamped chunk whose successor holds one row
    N = 349    splits of 96 and a last one of 61: plain chunks, then a clamped tail that ends in the middle of row tile 1
    N = 1280   splits of 256: seven plain chunks and a clamped one whose rows are all valid
The split kernel's loop has no boundary of its own: it is dx1w1_kernel2's loop; a wave with two column units stages the next chunk in two
halves, in every chunk alike.
Inputs: (a) gaussian dZ x 1e-3, (b) log-normal magnitudes exp(3 normal) with random signs in dZ and Wx, (c) dZ, Wx and obs all positive,
(d) structure: whole hidden columns of Wx and whole gate columns of dZ exactly zero, one hidden column of X1 nowhere positive, and the
first half of the rows cancelling in pairs (row n + N / 4 repeats row n with the opposite dZ).  About half of X1 is <= 0 in every kind.
Bound (the project's, for BOTH kernels): |out - ref64| <= 2e-5 * max|ref64| per tensor (dW1, db1).  Entries outside the block structure,
feature tiles without a structural non-zero and all-zero columns are exactly zero.  One Inf and one NaN in dZ of tower 1, in rows whose X1
is positive throughout, leave every db1 entry and every dW1 entry inside the structure of that tower non-finite, and tower 0 finite.
That bound alone cannot see the loss of one third-order piece product (2^-16 of a term; tests/test_split_mutants_host.py shows every
such mutant of the host restatement meeting it in at least 19 of 20 cases).  Two things pin the six-product arithmetic:
  * test_exact_probes_come_back_bit_for_bit: inputs whose six piece products sum exactly in any order, one product per output entry,
    both kernels np.array_equal to one expected array (tests/split_harness.py; the host test counts what the ownership maps own);
  * in test_both_kernels_match_float64 the split kernel's error is held to a multiple of the f32 kernel's on the same case, per tensor:
    split_harness.RATIO (max) and MEAN_C (mean, all-positive kind c), each threshold the geometric mean of the real kernels' largest
    ratio (measured here over all widths and sizes) and the weakest restated mutant's, with a factor 2 on each side.  Max on kinds a
    and d for dW1 and db1 (thresholds 3.45 .. 3.77; real kernels <= 1.63, mutants >= 8.7).  Mean on kind c (13.4 / 14.3; real kernels
    <= 1.08, mutants >= 174): it claims only the mutants that lose a product of Wx's third piece, the operand dx_cut8 TRUNCATES, whose
    remainders all have one sign.  Not adopted: the max on kind c and the mean on kind c over all third-order mutants (gap 0.2 / 0.3)
    -- dZ is rounded to nearest, so a lost a3 product is no bias there and lies below the f32 kernel's own error.  Kind b has no ratio
    criterion: the f32 kernel is at times unusually good on heavy tails (37 x on one case, `finding` of the profile) and b stays under
    the 2e-5 bound only.  The figures are printed and recorded in profiles/dx1w1_split_bench.json under `accuracy`.
test_split_path_differs_from_the_exact_path_only_in_w1_b1 keeps the bound 2e-5 max|g|: normalised per tower by the largest entry of
W1 | b1 the real paths differ by up to 3.8e-7 (large_grid) and 6.5e-7 (real_net), and the weakest mutant restated on the rows the
update read (dZ and X1 from the activation cache, Wx from the parameters, the obs fed in; towers 0, 1, 6, 7) by 1.2e-6 and 1.6e-6 --
gaps of 3.1 and 2.5, no room for a threshold at these small batches."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import split_harness as sh

pytestmark = pytest.mark.gpu

G, S, NZ, SMAX = 2, 5, 256, 40
WIDTHS = (224, 192, 160, 128)
SIZES = (1, 21, 160, 161, 349, 1280)
BOUND = 2e-5


def _structure(H):
    """-> rowrange [1][SMAX][2] int16, ftm [1][H / 16] int32, mask [SMAX][H] bool: obs rows 0..11 feed columns [0, H / 2), rows 12..23
    the last block, rows 24..35 the 32 columns between them, rows 36..39 nothing (agents/policies.py:41-61 in miniature)"""
    cw, cf = H // 2, 32
    rr = np.zeros((1, SMAX, 2), np.int16)
    rr[0, 0:12] = (0, cw)
    rr[0, 12:24] = (cw + cf, H)
    rr[0, 24:36] = (cw, cw + cf)
    ftm = np.zeros((1, H // 16), np.int32)
    for u in range(H // 16):
        for j in range(SMAX):
            if rr[0, j, 0] < 16 * u + 16 and rr[0, j, 1] > 16 * u:
                ftm[0, u] |= 1 << (j >> 4)
    cols = np.arange(H)[None, :]
    mask = (cols >= rr[0, :, 0:1]) & (cols < rr[0, :, 1:2])
    return rr, ftm, mask


def _run(H, N, dev, split):
    """-> [G][SMAX + 1][H] float32 from device tensors (dZ, X1, Wx, obs, ftm, rowrange)"""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import _setup_lib
    lib = _lib.lib()
    _setup_lib(lib)
    out = torch.full((G, SMAX + 1, H), float('nan'), dtype=torch.float32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.tsc_dx1w1_f32(H, N, G, S, SMAX, *[p(t) for t in dev], p(out), split))
    return out.cpu().numpy()


def _inputs(kind, H, N, rng):
    X1 = rng.randn(G, N, H)                                     # about half <= 0: the relu mask
    X1[rng.rand(G, N, H) < 0.05] = 0
    obs = rng.rand(N, 1, SMAX) * 2
    if kind == 'a':
        dZ, Wx = rng.randn(G, N, NZ) * 1e-3, rng.randn(G, H, NZ) * 0.1
    elif kind == 'b':
        ln = lambda *shp: np.exp(3 * rng.randn(*shp)) * rng.choice([-1.0, 1.0], shp)
        dZ, Wx = ln(G, N, NZ), ln(G, H, NZ)
    elif kind == 'c':
        dZ, Wx, obs = rng.rand(G, N, NZ) + 0.5, rng.rand(G, H, NZ) + 0.5, obs + 0.5
    else:
        dZ, Wx = rng.randn(G, N, NZ), rng.randn(G, H, NZ)
        Wx[:, ::7] = 0; dZ[:, :, 3::11] = 0
        X1[:, :, 5] = -np.abs(X1[:, :, 5])
        q = N // 4                                              # rows n and n + q (n < q) cancel: same X1 and obs, opposite dZ
        X1[:, q:2 * q], obs[q:2 * q], dZ[:, q:2 * q] = X1[:, :q], obs[:q], -dZ[:, :q]
    return [np.ascontiguousarray(v, np.float32) for v in (dZ, X1, Wx, obs)]


def _ref64(dZ, X1, Wx, obs, mask):
    with np.errstate(all='ignore'):
        dX1 = np.einsum('gnk,ghk->gnh', dZ.astype(np.float64), Wx.astype(np.float64)) * (X1 > 0)
        dW1 = np.einsum('nj,gnh->gjh', obs[:, 0].astype(np.float64), dX1) * mask[None]
        return np.concatenate([dW1, dX1.sum(1, keepdims=True)], 1)


def _errors(out, ref):
    """-> per tensor (dW1, db1): (max, mean) of |out - ref| / max|ref|"""
    res = []
    for lo, hi in ((0, SMAX), (SMAX, SMAX + 1)):
        sc = np.abs(ref[:, lo:hi]).max()
        e = np.abs(out[:, lo:hi] - ref[:, lo:hi])
        res.append((float(e.max() / sc) if sc > 0 else float(e.max()), float(e.mean() / sc) if sc > 0 else float(e.mean())))
    return res


def _device(arrs):
    return [torch.from_numpy(a).cuda() for a in arrs]


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('H', WIDTHS)
def test_both_kernels_match_float64(H, N):
    rng = np.random.RandomState(1000 * H + N)
    rr, ftm, mask = _structure(H)
    for kind in 'abcd':
        host = _inputs(kind, H, N, rng)
        ref = _ref64(*host, mask)
        dev = _device(host + [ftm, rr])
        outs = {split: _run(H, N, dev, split) for split in (1, 0)}
        errs = {split: _errors(outs[split], ref) for split in (1, 0)}
        for i, name in enumerate(('dW1', 'db1')):
            (ms, as_), (mf, af) = errs[1][i], errs[0][i]
            print('H=%d N=%d (%s) %s: split max %.3e mean %.3e | f32 max %.3e mean %.3e | ratio of max %.2f'
                  % (H, N, kind, name, ms, as_, mf, af, ms / mf if mf > 0 else float('nan')))
        for split in (1, 0):
            o = outs[split]
            assert np.isfinite(o).all()
            for (mx, _), name in zip(errs[split], ('dW1', 'db1')):
                assert mx <= BOUND, (H, N, kind, name, 'split' if split else 'f32', mx)
            assert (o[:, :SMAX][:, ~mask] == 0).all(), (H, N, kind, split)          # outside the structure, empty feature tiles
            if kind == 'd':
                assert (o[:, :, ::7] == 0).all() and (o[:, :, 5] == 0).all(), (H, N, split)
        named = [dict(zip(('dW1', 'db1'), errs[split])) for split in (1, 0)]
        assert kind == 'b' or sh.accuracy_criteria('dx1w1', kind)
        assert not sh.accuracy_failures('dx1w1', kind, *named), (H, N, kind, sh.accuracy_failures('dx1w1', kind, *named))
        if kind == 'd':
            assert (ref[:, :, ::7] == 0).all() and (ref[:, :, 5] == 0).all()


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('H', WIDTHS)
def test_exact_probes_come_back_bit_for_bit(H, N):
    """tests/split_harness.dx1w1_probe: every column of dX1 has ONE row that passes the relu mask, and that entry is ONE product whose
    six piece products sum exactly, in any order, to the f32 product; obs entries are powers of two.  db1 and every dW1 entry are
    single exact values, the same for both kernels: np.array_equal is the assertion, zeros outside the structure included."""
    rr, ftm, mask = _structure(H)
    for q0, boundary, seed in sh.probe_calls('dx1w1', H, N):
        dZ, X1, Wx, obs, exp, owner, ks = sh.dx1w1_probe(H, N, G, S, q0, boundary, seed)
        assert (exp[:, SMAX] != 0).all() and (exp[:, :SMAX][:, mask] != 0).all() and (exp[:, :SMAX][:, ~mask] == 0).all()
        dev = _device([dZ, X1, Wx, obs, ftm, rr])
        for split in (1, 0):
            o = _run(H, N, dev, split)
            bad = np.argwhere(o != exp)
            assert len(bad) == 0, (H, N, q0, boundary, 'split' if split else 'f32', len(bad), bad[0], owner[bad[0][0], bad[0][2]],
                                   ks[bad[0][0], bad[0][2]], float(o[tuple(bad[0])]), float(exp[tuple(bad[0])]))
            assert np.array_equal(o, exp)


@pytest.mark.parametrize('H', WIDTHS)
def test_inf_and_nan_in_dz_poison_their_tower(H):
    N = 349
    rng = np.random.RandomState(H)
    rr, ftm, mask = _structure(H)
    dZ, X1, Wx, obs = _inputs('a', H, N, rng)
    r_inf, r_nan = 130, 340                                     # a plain chunk of the second split; the clamped tail of the fourth
    dZ[1, r_inf, 37 + H // 32] = np.inf
    dZ[1, r_nan, 201] = np.nan
    X1[1, r_inf] = 1.0
    X1[1, r_nan] = 1.0
    dev = _device([dZ, X1, Wx, obs, ftm, rr])
    for split in (1, 0):
        o = _run(H, N, dev, split)
        assert np.isfinite(o[0]).all(), (H, split)
        assert not np.isfinite(o[1, SMAX]).any(), (H, split, int(np.isfinite(o[1, SMAX]).sum()))
        assert not np.isfinite(o[1, :SMAX][mask]).any(), (H, split, int(np.isfinite(o[1, :SMAX][mask]).sum()))
        assert (o[1, :SMAX][~mask] == 0).all(), (H, split)


def _rand_obs(scn, E, rng):
    obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
    for a, n in enumerate(scn.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


def _rollout_grads(scenario, E, T, monkeypatch, dx_split):
    """The rollout of tests/test_dwxh_split_gpu._rollout_grads, then compute_grads -> (flat gradient, layout)"""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    monkeypatch.setenv('TSC_DX_SPLIT', dx_split)
    scn = build_scenario(scenario, 'ma2c')
    cfg = dict(batch_size=T)
    if scenario == 'real_net':
        cfg['reward_norm'] = 1.0
    m = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, int(scn.green_tab.shape[1]), cfg, device=0, seed=5, name='ma2c')
    assert m.plan[2] == 1 and m.dx_split == int(dx_split)
    m.reset()
    rng = np.random.RandomState(123)
    obs, done = _rand_obs(scn, E, rng), np.ones(E, np.uint8)
    for t in range(T):
        d_obs, d_done = torch.from_numpy(obs).cuda(), torch.from_numpy(done).cuda()
        _, v, _ = m.forward_sample(d_obs, d_done)
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, scn.n_agent) * 3.0 * m.cfg['reward_norm']
        dpost = (rng.rand(E) < 0.1).astype(np.uint8)
        m.add_transition(d_obs, d_done, torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(), v.clone(), torch.from_numpy(dpost).cuda())
        obs, done = _rand_obs(scn, E, rng), dpost
    Rb = m.forward(torch.from_numpy(obs).cuda(), False, 'v').clone()
    _lib.check(m._L.tsc_model_compute_grads(m._h, C.c_void_p(Rb.data_ptr()), 0.01))
    g = m.grad_tensor().cpu().numpy().copy()
    lay = (C.c_int64 * 12)()
    _lib.check(m._L.tsc_model_layout(m._h, lay))
    m.close()
    return g, [int(x) for x in lay]


@pytest.mark.parametrize('scenario,E,T', [('large_grid', 33, 25), ('real_net', 40, 9)])
def test_split_path_differs_from_the_exact_path_only_in_w1_b1(scenario, E, T, monkeypatch):
    new, lay = _rollout_grads(scenario, E, T, monkeypatch, '1')
    ref, _ = _rollout_grads(scenario, E, T, monkeypatch, '0')
    towers, stride, oW1, oWx = lay[0], lay[1], lay[4], lay[6]
    new, ref = new.reshape(towers, stride), ref.reshape(towers, stride)
    assert oW1 == 0
    np.testing.assert_array_equal(new[:, oWx:], ref[:, oWx:])             # everything after W1 | b1: bit for bit
    scale = np.abs(ref).max()
    assert scale > 0 and np.abs(ref[:, :oWx]).max() > 0
    print('%s E=%d T=%d: max |split - f32| = %.3e of max|g| = %.3e' % (scenario, E, T, np.abs(new - ref).max() / scale, scale))
    np.testing.assert_allclose(new[:, :oWx], ref[:, :oWx], atol=BOUND * scale, rtol=0)
    np.testing.assert_array_equal(new == 0, ref == 0)
