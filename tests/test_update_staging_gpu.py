"""The fused weight-gradient kernels of the LSTM update (dwxh_kernel: dWx | dWh | dbl; dx1w1_kernel2: dW1 | db1 with dX1 in
registers) at every boundary of their row loops, against the grouped GEMMs they replace (TSC_UNFUSED_DW=1 TSC_UNFUSED_DX=1).

Both kernels cut a tower's N = E * T rows into s_upd = 5 splits (50 towers on large_grid), rps = ceil(N / 5) rows each, rounded
up to even (dwxh) or to a multiple of 32 (dx1w1); R is a split's own length (the last one may be shorter).
dwxh streams a split in 16-row sub-chunks c = 0, 1, ...: four at a time without any row clamp while 16 (c + 9) <= R (the interval
and everything it stages ahead lie inside the split, so R >= 144 for the first), then one clamped sub-chunk at a time until the
rows are used up.  dx1w1 runs a 32-row chunk unclamped while row + 64 <= n1 (the chunk and its successor inside the split),
clamped otherwise.  What each shape drives (tests/test_update_staging_host.py restates the schedule and counts the same):
    E, T = 1, 1     N = 1: four of the five splits are empty, the fifth is a single row (one clamped sub-chunk / chunk)
    E, T = 3, 7     N = 21: dwxh (rps 6) only clamped sub-chunks shorter than 16 rows; dx1w1 (rps 32) one short clamped chunk and
                    four empty splits
    E, T = 33, 13   N = 429: dwxh (rps 86, last split 85: odd) six clamped sub-chunks across one barrier, no unclamped interval;
                    dx1w1 (rps 96) two unclamped chunks + one clamped, last split 45 rows = two clamped chunks
    E, T = 33, 25   N = 825: dwxh (rps 166) ONE unclamped interval, then seven clamped sub-chunks ending in a 6-row one; its last
                    split has 161 rows (odd, after an unclamped interval, last sub-chunk a single row); dx1w1 (rps 192) five
                    unclamped chunks + one clamped, last split 57 rows = two clamped chunks
    E, T = 64, 20   N = 1280: dwxh (rps 256) two unclamped intervals, then eight clamped sub-chunks whose rows are all valid;
                    dx1w1 seven unclamped chunks + one clamped per split, every row valid
and Monaco (real_net: H = 192, s_max = 52, heterogeneous towers, N = 360 in splits below 144 rows: clamped path only) at
E, T = 40, 9 for the other instantiation.  The unclamped loops at many intervals run in test_model_gpu's T = 120 cases.
fc_bwd_kernel (FcACPolicy: dWfc | dbfc | dW1 | db1, against TSC_UNFUSED_DX=1) has ONE row loop: 32-row chunks, every row index
clamped and rows past the split stored as zero dZ rows, rps = ceil(N / 5) rounded up to a multiple of 32 like dx1w1:
    large_grid IA2C fc (H = 160):  E, T = 1, 1 and 3, 7 (N = 1 and 21: empty splits, one short chunk), 33, 13 (N = 429: ragged last
                    chunk, last split 45 rows), 64, 20 (N = 1280: every row valid)
    large_grid MA2C fc (H = 224, the fourth X1 staging slot) at 33, 13;  real_net MA2C fc (H = 192) at 40, 9
Tolerance as in test_model_gpu.test_fused_update_kernels_equal_grouped_gemms: |d| <= 2e-5 * max|g| (fp32 summation order), and
the same entries exactly zero."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand_obs(scn, E, rng):
    obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
    for a, n in enumerate(scn.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


def _grads(scenario, E, T, unfused, monkeypatch, agent='ma2c', policy='lstm'):
    """One rollout through the trainer's path (fused forward + sampling, activations cached for the update; random dones),
    then compute_grads: the flat gradient."""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    monkeypatch.setenv('TSC_UNFUSED_DW', unfused)
    monkeypatch.setenv('TSC_UNFUSED_DX', unfused)
    scn = build_scenario(scenario, agent)
    cfg = dict(batch_size=T)
    if scenario == 'real_net':
        cfg['reward_norm'] = 1.0
    m = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, int(scn.green_tab.shape[1]), cfg, device=0, seed=5,
               name=agent, policy=policy)
    m.reset()
    rng = np.random.RandomState(123)
    obs, done = _rand_obs(scn, E, rng), np.ones(E, np.uint8)
    for t in range(T):
        d_obs, d_done = torch.from_numpy(obs).cuda(), torch.from_numpy(done).cuda()
        _, v, _ = m.forward_sample(d_obs, d_done)
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, scn.n_agent) * 3.0 * m.cfg['reward_norm']
        dpost = (rng.rand(E) < 0.1).astype(np.uint8)
        m.add_transition(d_obs, d_done, torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(), v.clone(),
                         torch.from_numpy(dpost).cuda())
        obs, done = _rand_obs(scn, E, rng), dpost
    Rb = m.forward(torch.from_numpy(obs).cuda(), False, 'v').clone()
    _lib.check(m._L.tsc_model_compute_grads(m._h, C.c_void_p(Rb.data_ptr()), 0.01))
    g = m.grad_tensor().cpu().numpy().copy()
    m.close()
    return g


@pytest.mark.parametrize('scenario,E,T', [('large_grid', 1, 1), ('large_grid', 3, 7), ('large_grid', 33, 13), ('large_grid', 33, 25),
                                          ('large_grid', 64, 20), ('real_net', 40, 9)])
def test_update_staging_equals_grouped_gemms(scenario, E, T, monkeypatch):
    fused = _grads(scenario, E, T, '0', monkeypatch)
    ref = _grads(scenario, E, T, '1', monkeypatch)
    scale = np.abs(ref).max()
    assert scale > 0
    print('%s E=%d T=%d: max |fused - grouped| = %.3e of max|g| = %.3e' % (scenario, E, T, np.abs(fused - ref).max() / scale, scale))
    np.testing.assert_allclose(fused, ref, atol=2e-5 * scale, rtol=0)
    np.testing.assert_array_equal(fused == 0, ref == 0)


@pytest.mark.parametrize('scenario,agent,E,T', [('large_grid', 'ia2c', 1, 1), ('large_grid', 'ia2c', 3, 7), ('large_grid', 'ia2c', 33, 13),
                                                ('large_grid', 'ia2c', 64, 20), ('large_grid', 'ma2c', 33, 13), ('real_net', 'ma2c', 40, 9)])
def test_fc_bwd_equals_grouped_gemms(scenario, agent, E, T, monkeypatch):
    fused = _grads(scenario, E, T, '0', monkeypatch, agent, 'fc')
    ref = _grads(scenario, E, T, '1', monkeypatch, agent, 'fc')
    scale = np.abs(ref).max()
    assert scale > 0
    print('%s %s fc E=%d T=%d: max |fused - grouped| = %.3e of max|g| = %.3e' % (scenario, agent, E, T, np.abs(fused - ref).max() / scale, scale))
    np.testing.assert_allclose(fused, ref, atol=2e-5 * scale, rtol=0)
    np.testing.assert_array_equal(fused == 0, ref == 0)
