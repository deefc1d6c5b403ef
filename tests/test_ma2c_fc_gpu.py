"""MA2C with the feed-forward fingerprint policy (FPFcACPolicy, agents/policies.py:259-282) on the HIP learner.

* The two episodes recorded from the reference's own learner (tools/make_golden_fpfc.py) replayed through VecA2C with the
  tolerances tests/test_refnet_gpu.py documents: large_grid (H = 224) at E = 1 and 33 through the reference's API order
  and at E = 1024 through the zero-copy rollout slots; Monaco (H = 192) at E = 1 and E = 512 through the slots, its
  gradients measured against their tower's largest gradient (_tower_scaled_check: two near-vanishing tensors).
* Which kernels ran (include/tsc.h tsc_model_path): policy_fwd_fc_mfma_kernel<7> / <6> for the rollout forward and
  fc_bwd_kernel<14> / <12> for the update.
* The update at the benchmarked batch (E = 1024 DISTINCT instances, T = 120) against the float64 oracle.
* The fast paths against their fallbacks, at float32 tolerance: the MFMA forward against TSC_FC_MFMA=0 (Monaco: the
  per-thread policy_fwd_fc_kernel; large_grid: the dense GEMMs + head kernel, since the per-thread kernel's LDS does not
  fit at H = 224) and the fused backward against the grouped split-K GEMMs (TSC_UNFUSED_DX=1)."""
import numpy as np
import pytest
import torch

from oracle import refnet
from tests.test_model_gpu import test_update_benchmarked_batch_E1024_T120 as _update_vs_oracle
from tests.test_refnet_gpu import test_hip_replays_reference_learner as _replay

pytestmark = pytest.mark.gpu

CASES = [('refnet_ma2c_fc_large', 1, 'api'), ('refnet_ma2c_fc_large', 33, 'api'), ('refnet_ma2c_fc_large', 1024, 'slots'),
         ('refnet_ma2c_fc_real', 1, 'api'), ('refnet_ma2c_fc_real', 512, 'slots')]


def _tower_scaled_check(got_towers, names, rows, tol, what, sums_only=False, sum_tol=None):
    """refnet.check_digests with every gradient tensor measured against its TOWER's largest gradient (what the clip and
    RMSProp see) instead of its own maximum.  Monaco's first update has two policy towers whose gradients nearly vanish
    (tower 6 out_b: max 5e-8, tower 32 fc_w: 6e-7 -- 1e-3 to 1e-5 of their towers): there float32 cancellation alone
    reaches 1.7e-2 (E = 1) and 1.2e-3 (E = 512) of the tensor's own maximum on EVERY path, the grouped-GEMM fallbacks
    (TSC_UNFUSED_DX=1, TSC_FC_MFMA=0) included, while the worst error relative to the tower is 1.9e-4 on all of them."""
    want = refnet.unpack_digests(names, rows)
    got = refnet.tower_digest(got_towers, sums_only=sums_only)
    assert set(got) == set(want), what
    sum_tol = tol if sum_tol is None else sum_tol
    tmax = {}
    for k, v in want.items():
        t = k.split('/')[0]
        tmax[t] = max(tmax.get(t, 0.0), v[3])
    worst = 0.0
    for k in want:
        scale = max(want[k][3], tmax[k.split('/')[0]], 1e-30)
        np.testing.assert_allclose(got[k][:refnet.N_SUMS], want[k][:refnet.N_SUMS], rtol=sum_tol, atol=sum_tol * scale,
                                   err_msg='%s %s sums' % (what, k))
        if len(want[k]) > refnet.N_SUMS:
            err = np.abs(got[k][refnet.N_SUMS:] - want[k][refnet.N_SUMS:]).max() / scale
            worst = max(worst, err)
            assert err <= tol, '%s %s: %.3g > %.3g' % (what, k, err, tol)
    return worst


@pytest.mark.parametrize('name,E,path', CASES)
def test_hip_replays_reference_ma2c_fc(name, E, path, monkeypatch):
    if name == 'refnet_ma2c_fc_real':
        monkeypatch.setattr(refnet, 'check_digests', _tower_scaled_check)
    _replay(name, E, path)


def _model(scenario, E, T, seed=5, **mc):
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(scenario, 'ma2c')
    cfg = dict(batch_size=T, reward_norm=1.0 if scenario == 'real_net' else 2000.0)
    cfg.update(mc)
    m = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, int(scn.green_tab.shape[1]), cfg, device=0,
               seed=seed, name='ma2c', policy='fc')
    return scn, m


@pytest.mark.parametrize('scenario,H', [('large_grid', 224), ('real_net', 192)])
def test_fast_paths_selected(scenario, H):
    """At the benchmarked batch the matrix-core forward and the one-pass backward are what runs (tsc_model_path)."""
    scn, m = _model(scenario, 1024 if scenario == 'large_grid' else 512, 120 if scenario == 'large_grid' else 40)
    assert m.H == H and m.n_fc == (128, 64, 32 if scenario == 'large_grid' else 0)
    assert m.fc_path == (2, 1), m.fc_path
    m.close()


def test_update_benchmarked_batch_E1024_T120_ma2c_fc():
    """E = 1024 distinct instances x T = 120 (122 880 rows per agent-tower, five row splits of fc_bwd_kernel<14>) through
    the rollout path with the activation cache, three agents against the float64 oracle at <= 1e-4 of max|g|."""
    _update_vs_oracle('large_grid', 'ma2c', 'fc', 1024, 120, None)


def _rand_obs(scn, E, rng):
    obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
    for a, n in enumerate(scn.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


@pytest.mark.parametrize('scenario,E,slow', [('large_grid', 1024, 0), ('real_net', 512, 1)])
def test_mfma_forward_equals_fallback(scenario, E, slow, monkeypatch):
    """policy_fwd_fc_mfma_kernel against the path TSC_FC_MFMA=0 selects, same weights, same observations."""
    scn, fast = _model(scenario, E, 4)
    monkeypatch.setenv('TSC_FC_MFMA', '0')
    _, ref = _model(scenario, E, 4)
    monkeypatch.delenv('TSC_FC_MFMA')
    assert fast.fc_path[0] == 2 and ref.fc_path[0] == slow
    ref.copy_from(fast)
    rng = np.random.RandomState(3)
    done = torch.zeros(E, dtype=torch.uint8, device='cuda')
    for _ in range(3):
        obs = torch.from_numpy(_rand_obs(scn, E, rng)).cuda()
        p1, v1 = (x.clone() for x in fast.forward(obs, done, 'pv'))
        p2, v2 = (x.clone() for x in ref.forward(obs, done, 'pv'))
        p1, v1, p2, v2 = (x.cpu().numpy() for x in (p1, v1, p2, v2))
        assert np.isfinite(p1).all() and np.isfinite(v1).all()
        np.testing.assert_allclose(p1, p2, rtol=0, atol=1e-5)
        np.testing.assert_allclose(v1, v2, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(v2).max())))
    fast.close(); ref.close()


def _rollout_grads(m, scn, E, T, seed):
    """T steps through forward_sample (activation cache) with a fixed stream of obs / actions / rewards, then the update."""
    rng = np.random.RandomState(seed)
    A = scn.n_agent
    m.reset()
    done = torch.ones(E, dtype=torch.uint8, device='cuda')
    for _ in range(T):
        obs = torch.from_numpy(_rand_obs(scn, E, rng)).cuda()
        _, v, _ = m.forward_sample(obs, done)
        act = torch.from_numpy(np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)).cuda()
        rew = torch.from_numpy(-rng.rand(E, A) * 3.0 * m.cfg['reward_norm']).cuda()
        dpost = torch.from_numpy((rng.rand(E) < 0.05).astype(np.uint8)).cuda()
        m.add_transition(obs, done, act, rew, v, dpost)
        done = dpost
    R = m.forward(torch.from_numpy(_rand_obs(scn, E, rng)).cuda(), False, 'v').clone()
    m.compute_grads(R)
    return m.unpack(m.grad_tensor().cpu().numpy())


@pytest.mark.parametrize('scenario,E,T', [('large_grid', 1024, 120), ('real_net', 512, 40)])
def test_fused_backward_equals_grouped_gemms(scenario, E, T, monkeypatch):
    """fc_bwd_kernel<14> / <12> (dWfc | dbfc | dW1 | db1 in one pass, dX1 in registers) against the grouped split-K GEMMs
    with dX1 through HBM: the same rollout (same weights, same sampled actions), every gradient tensor of every tower
    within 1e-4 of that tensor's largest entry, structural zeros of the three-block W1 exactly zero on both."""
    scn, fast = _model(scenario, E, T)
    monkeypatch.setenv('TSC_UNFUSED_DX', '1')
    _, ref = _model(scenario, E, T)
    monkeypatch.delenv('TSC_UNFUSED_DX')
    assert fast.fc_path == (2, 1) and ref.fc_path == (2, 0)
    ref.copy_from(fast)
    g1, g2 = _rollout_grads(fast, scn, E, T, 11), _rollout_grads(ref, scn, E, T, 11)
    worst = 0.0
    for t, (a, b) in enumerate(zip(g1, g2)):
        assert set(a) == set(b)
        for k in a:
            assert np.isfinite(a[k]).all(), (t, k)
            scale = max(float(np.abs(b[k]).max()), 1e-12)
            err = float(np.abs(a[k] - b[k]).max()) / scale
            worst = max(worst, err)
            assert err <= 1e-4, 'tower %d %s: %.2e of max|g|' % (t, k, err)
    lay = fast.layout
    for flat in (fast.grad_tensor().cpu().numpy(), ref.grad_tensor().cpu().numpy()):
        W1 = flat.reshape(lay.G, lay.stride)[:, lay.oW1:lay.ob1].reshape(lay.G, lay.s_max, lay.H)
        fw, fp, ft = lay.n_fc
        for g in range(lay.G):
            a = g // 2
            nw, nt, nf = lay.n_wave_ls[a], lay.n_w_ls[a], lay.n_f_ls[a]
            mask = np.zeros((lay.s_max, lay.H), bool)
            mask[:nw, :fw] = True
            mask[nw + nt:nw + nt + nf, fw:fw + fp] = True
            mask[nw:nw + nt, fw + fp:] = True
            assert (W1[g][~mask] == 0).all(), g
    print('%s E=%d T=%d fused vs grouped GEMMs: worst %.2e of max|g|' % (scenario, E, T, worst))
    fast.close(); ref.close()
