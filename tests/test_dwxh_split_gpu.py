"""dwxh_split_kernel (dWx | dWh | dbl on the bf16 matrix cores, every f32 operand cut into three bf16 pieces, six products) and the
exact-f32 dwxh_kernel through the test entry tsc_dwxh_f32, against a float64 NumPy product of the same inputs.

Shapes: G = 2 towers, every fused width H = 224 / 192 / 160 / 128, S = 5 row splits, N at every boundary of the split kernel's row loop
(16-row steps; an interval of two steps runs unclamped while 16 (c + 5) <= R; tests/test_dwxh_split_host.py counts the same):
    N = 1      one row, four empty splits
    N = 21     splits of 6 / 6 / 6 / 3 / 0 rows: shorter than one step, an empty split
    N = 349    splits of 70 and an odd last one of 69: five clamped steps across two barriers, no unclamped interval
    N = 409    splits of 82 and a last one of 81: ONE unclamped interval, then a clamped tail whose last step is a single row
    N = 1280   splits of 256: six unclamped intervals and four clamped steps whose rows are all valid
Inputs: (a) relu(normal) x normal * 1e-3 with ~10 % of the h_prev rows zero (the done mask), (b) log-normal magnitudes exp(3 normal) with
random signs, (c) all positive, (d) structure: whole feature columns of X1 and whole gate columns of dZ exactly zero, and the first
half of the rows cancelling in pairs (row n + N / 4 repeats row n with the opposite dZ).
Bound (the project's, for BOTH kernels): |out - ref64| <= 2e-5 * max|ref64| per tensor (dWx, dWh, dbl).  Outputs of all-zero columns
are exactly zero.  dbl: the split kernel adds a lane's dZ rows in the order 8h + j where dwxh_kernel adds 2 ks + h, so dbl is NOT
bit-equal between the two and is held to the same bound.  One Inf in dZ leaves every output of its gate column non-finite.
That bound alone cannot see the loss of one third-order piece product (2^-16 of a term; tests/test_split_mutants_host.py shows every
such mutant of the host restatement meeting it).  Two things pin the six-product arithmetic:
  * test_exact_probes_come_back_bit_for_bit: inputs whose six piece products sum exactly in any order, one product per output entry,
    both kernels np.array_equal to one expected array (tests/split_harness.py; the host test counts what the ownership maps own);
  * in test_both_kernels_match_float64 the split kernel's max error is held to a multiple of the f32 kernel's on the same case, per
    tensor: split_harness.RATIO, each threshold the geometric mean of the real kernels' largest ratio (measured here over all widths
    and sizes) and the weakest restated mutant's, with a factor 2 on each side.  dWx, dWh on kinds a and d (thresholds 7.3 .. 10.3;
    real kernels <= 2.27, mutants >= 31) and dWx on kind c (3.46; 1.69 / 7.1).  Not adopted, the gap being under 4: dWh on kind c
    (1.78 / 6.5) and the mean on kind c for both tensors (1.37 / 5.0) -- every cut of this kernel rounds to nearest, so on all-positive
    input a lost product is no bias.  Kind b has no ratio criterion (the f32 kernel is at times unusually good on heavy tails) and
    stays under the 2e-5 bound; dbl holds no piece product.  The figures are printed and recorded in profiles/dwxh_split_bench.json
    under `accuracy`.
test_split_path_equals_exact_f32_path keeps the bound 2e-5 max|g|: normalised per tower by the largest entry of Wx | Wh | bl the real
paths differ by up to 4.6e-7 (large_grid) and 1.3e-6 (real_net), and the weakest mutant restated on the rows the update read (towers
0, 1, 6, 7) by 1.5e-6 and 1.6e-6 -- gaps of 3.2 and 1.2, no room for a threshold at these small batches."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import split_harness as sh

pytestmark = pytest.mark.gpu

G, S, L, NZ = 2, 5, 64, 256
WIDTHS = (224, 192, 160, 128)
SIZES = (1, 21, 349, 409, 1280)
BOUND = 2e-5


def _run(H, N, X1, Hp, dZ, split, g=G, s=S):
    """-> [g][H + 64 + 1][256] float32 from device tensors"""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import _setup_lib
    lib = _lib.lib()
    _setup_lib(lib)
    out = torch.full((g, H + L + 1, NZ), float('nan'), dtype=torch.float32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.tsc_dwxh_f32(H, N, g, s, p(X1), p(Hp), p(dZ), p(out), split))
    return out.cpu().numpy()


def _inputs(kind, H, N, rng):
    shp = lambda w: (G, N, w)
    if kind == 'a':
        X1, Hp = np.maximum(rng.randn(*shp(H)), 0), np.tanh(rng.randn(*shp(L)))
        Hp[rng.rand(G, N) < 0.1] = 0
        dZ = rng.randn(*shp(NZ)) * 1e-3
    elif kind == 'b':
        ln = lambda w: np.exp(3 * rng.randn(*shp(w))) * rng.choice([-1.0, 1.0], shp(w))
        X1, Hp, dZ = ln(H), ln(L), ln(NZ)
    elif kind == 'c':
        X1, Hp, dZ = rng.rand(*shp(H)) + 0.5, rng.rand(*shp(L)) + 0.5, rng.rand(*shp(NZ)) + 0.5
    else:
        X1, Hp, dZ = rng.randn(*shp(H)), rng.randn(*shp(L)), rng.randn(*shp(NZ))
        X1[:, :, ::7] = 0; Hp[:, :, 5] = 0; dZ[:, :, 3::11] = 0
        q = N // 4                                              # rows n and n + q (n < q) cancel: same X1 | h_prev, opposite dZ
        X1[:, q:2 * q], Hp[:, q:2 * q], dZ[:, q:2 * q] = X1[:, :q], Hp[:, :q], -dZ[:, :q]
    return [np.ascontiguousarray(v, np.float32) for v in (X1, Hp, dZ)]


def _ref64(X1, Hp, dZ):
    A = np.concatenate([X1, Hp], 2).astype(np.float64)
    Z = dZ.astype(np.float64)
    with np.errstate(all='ignore'):
        return np.concatenate([np.einsum('gnk,gnc->gkc', A, Z), Z.sum(1, keepdims=True)], 1)


def _errors(out, ref, H):
    """-> per tensor (dWx, dWh, dbl): (max, mean) of |out - ref| / max|ref|"""
    res = []
    for lo, hi in ((0, H), (H, H + L), (H + L, H + L + 1)):
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
    for kind in 'abcd':
        host = _inputs(kind, H, N, rng)
        ref = _ref64(*host)
        dev = _device(host)
        outs = {split: _run(H, N, *dev, split) for split in (1, 0)}
        errs = {split: _errors(outs[split], ref, H) for split in (1, 0)}
        for i, name in enumerate(('dWx', 'dWh', 'dbl')):
            (ms, as_), (mf, af) = errs[1][i], errs[0][i]
            print('H=%d N=%d (%s) %s: split max %.3e mean %.3e | f32 max %.3e mean %.3e | ratio of max %.2f'
                  % (H, N, kind, name, ms, as_, mf, af, ms / mf if mf > 0 else float('nan')))
        for split in (1, 0):
            assert np.isfinite(outs[split]).all()
            for (mx, _), name in zip(errs[split], ('dWx', 'dWh', 'dbl')):
                assert mx <= BOUND, (H, N, kind, name, 'split' if split else 'f32', mx)
        named = [dict(zip(('dWx', 'dWh', 'dbl'), errs[split])) for split in (1, 0)]
        assert kind == 'b' or sh.accuracy_criteria('dwxh', kind)
        assert not sh.accuracy_failures('dwxh', kind, *named), (H, N, kind, sh.accuracy_failures('dwxh', kind, *named))
        if kind == 'd':
            for split in (1, 0):
                o = outs[split]
                assert (o[:, 0:H:7] == 0).all() and (o[:, H + 5] == 0).all() and (o[:, :, 3::11] == 0).all(), (H, N, split)
                assert (ref[:, 0:H:7] == 0).all() and (ref[:, :, 3::11] == 0).all()


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('H', WIDTHS)
def test_exact_probes_come_back_bit_for_bit(H, N):
    """tests/split_harness.dwxh_probe: every entry of dWx | dWh is ONE product whose six piece products sum exactly, in any order, to the
    f32 product -- the expected array is the same for both kernels and np.array_equal is the assertion.  Features nobody owns are
    exactly zero.  dbl is a plain f32 row sum of dZ, not exact under this construction: it keeps the bound."""
    for q0, boundary, seed in sh.probe_calls('dwxh', H, N):
        X1, Hp, dZ, exp, owner = sh.dwxh_probe(H, N, G, S, q0, boundary, seed)
        assert (owner < 0).any() and (exp[owner >= 0] != 0).all()
        dev = _device([X1, Hp, dZ])
        dbl = dZ.astype(np.float64).sum(1)
        for split in (1, 0):
            o = _run(H, N, *dev, split)
            bad = np.argwhere(o[:, :H + L] != exp)
            assert len(bad) == 0, (H, N, q0, boundary, 'split' if split else 'f32', len(bad), bad[0], owner[bad[0][0], bad[0][1]],
                                   float(o[tuple(bad[0])]), float(exp[tuple(bad[0])]))
            assert np.array_equal(o[:, :H + L], exp)
            assert (o[:, :H + L][owner < 0] == 0).all()
            assert np.abs(o[:, H + L] - dbl).max() <= BOUND * np.abs(dbl).max(), (H, N, q0, split)


@pytest.mark.parametrize('H', WIDTHS)
def test_an_inf_in_dz_poisons_its_gate_column(H):
    N = 409
    rng = np.random.RandomState(H)
    X1, Hp, dZ = _inputs('a', H, N, rng)
    col = 37 + H // 32
    dZ[1, 300, col] = np.inf                                    # a row of the fourth split, tower 1
    dev = _device([X1, Hp, dZ])
    for split in (1, 0):
        o = _run(H, N, *dev, split)
        assert not np.isfinite(o[1, :, col]).any(), (H, split, int(np.isfinite(o[1, :, col]).sum()))
        rest = np.delete(o[1], col, 1)
        assert np.isfinite(rest).all() and np.isfinite(o[0]).all()


def _rand_obs(scn, E, rng):
    obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
    for a, n in enumerate(scn.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


def _rollout_grads(scenario, E, T, monkeypatch, dw_split, towers=()):
    """The rollout of tests/test_update_staging_gpu._grads, then compute_grads -> (flat gradient, layout, H, {tower: (X1, Hp, dZ)}): the
    rows dwxh read, back from the activation cache (tsc_model_debug_read what = 0, 4, 1; Z holds the gate gradients after BPTT)."""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    if dw_split is None:
        monkeypatch.delenv('TSC_DW_SPLIT', raising=False)
    else:
        monkeypatch.setenv('TSC_DW_SPLIT', dw_split)
    scn = build_scenario(scenario, 'ma2c')
    cfg = dict(batch_size=T)
    if scenario == 'real_net':
        cfg['reward_norm'] = 1.0
    m = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, int(scn.green_tab.shape[1]), cfg, device=0, seed=5, name='ma2c')
    assert m.plan[1] == 1 and m.dw_split == (0 if dw_split == '0' else 1)
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
    lay = [int(x) for x in lay]
    H, N, rows = lay[2], E * T, {}
    for tw in towers:
        got = []
        for what, w in ((0, H), (4, L), (1, NZ)):
            out = np.zeros((N, w), np.float32)
            _lib.check(m._L.tsc_model_debug_read(m._h, what, tw, 0, N, out.ctypes.data_as(C.c_void_p)))
            got.append(out)
        rows[tw] = got
    m.close()
    return g, lay, H, rows


def test_benchmark_length_rollout_against_float64_of_the_kernels_own_inputs(monkeypatch):
    """T = 120, E = 160 (N = 19200: splits of 3840 rows, 118 unclamped intervals each): the dWx | dWh | dbl slices of the flat gradient
    against the float64 product of the very rows the kernel read, two towers."""
    towers = (3, 41)
    g, lay, H, rows = _rollout_grads('large_grid', 160, 120, monkeypatch, None, towers)
    stride, oWx = lay[1], lay[6]
    for tw in towers:
        X1, Hp, dZ = rows[tw]
        ref = _ref64(X1[None], Hp[None], dZ[None])
        out = g[tw * stride + oWx: tw * stride + oWx + (H + L + 1) * NZ].reshape(1, H + L + 1, NZ)
        errs = _errors(out, ref, H)
        print('tower %d: dWx %.3e dWh %.3e dbl %.3e of max|ref64|' % (tw, errs[0][0], errs[1][0], errs[2][0]))
        assert np.abs(ref).max() > 0
        for (mx, _), name in zip(errs, ('dWx', 'dWh', 'dbl')):
            assert mx <= BOUND, (tw, name, mx)


@pytest.mark.parametrize('scenario,E,T', [('large_grid', 33, 25), ('real_net', 40, 9)])
def test_split_path_equals_exact_f32_path(scenario, E, T, monkeypatch):
    new, _, _, _ = _rollout_grads(scenario, E, T, monkeypatch, None)
    ref, _, _, _ = _rollout_grads(scenario, E, T, monkeypatch, '0')
    scale = np.abs(ref).max()
    assert scale > 0
    print('%s E=%d T=%d: max |split - f32| = %.3e of max|g| = %.3e' % (scenario, E, T, np.abs(new - ref).max() / scale, scale))
    np.testing.assert_allclose(new, ref, atol=BOUND * scale, rtol=0)
    np.testing.assert_array_equal(new == 0, ref == 0)
