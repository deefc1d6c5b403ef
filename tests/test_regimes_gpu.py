"""GPU parity of both learners in the VALUE regimes of tests/layouts.py REGIMES, where training ends and no other module goes: policies
so peaked that taken actions sit below the 1e-10 clamp of log pi (head_bwd_kernel's `inr` branch, A2C and PPO), the softmax of all six
forward / backward copies at logits where expf underflows and pi holds exact zeros, sample_action on a cdf with flat stretches, the
hardware exp2 / rcp gates away from the origin, a per-agent clip factor that binds for some agents of a launch and not for others
(rmsprop_kernel, iql_adam_kernel), an exactly one-hot policy, and the first-maximum rule of the Q-learners' act / a* kernels on an exact
tie.  tests/test_regimes_host.py states, on the oracles alone and on these very draws, that each case IS in its regime and that a
correct float32 evaluation stays within half of every bound used here.

Shapes: the smallest that reach every route -- (E, T) = (5, 6) and (37, 7), forward at E = 37; head8 (Ws / FcMfma, n_a 2, 5, 7, 8), h96 (Tile
/ FcThread), h124 (Dense), edges192 (H = 192, n_a 2 - 6); every case first asserts the route against the layout table.
Tolerances are the project's: pi 2e-5, v 2e-5 max(1, max|v|), gradients 2e-5 max|g| per tensor and 2e-4 in the second round (ReLU-kink
columns as _grad_err treats them), losses and norms rtol 2e-3, parameters 3e-5.

half_clip runs RMSProp at lr = 2e-3 (LY.HALF_CLIP_LR): the parameter tolerance 3e-5 cannot tell a clip factor of 1 from 40 / norm at the
usual 5e-4.  At 2e-3 a clipped agent stepped with factor 1 moves some parameter by 3.0e-3 to 6.6e-3 over the cases here (the host module
asserts at least 100 x 3e-5 in every round of every half_clip case).

PPO (head8, `peaked`, K = 2, lr 5e-5): at epoch 1 on the oracle 33.0 % of the taken actions sit below the clamp (where they did at epoch
0 too the ratio is exactly 1 and there is no policy gradient) and 22.8 % of all samples are clipped."""
import itertools

import numpy as np
import pytest
import torch

from tests import iql_harness as H
from tests import layouts as LY
from tests.test_layouts_gpu import _plan_of
from tests.test_layouts_host import value_bound

pytestmark = pytest.mark.gpu


def _a2c(regime, name, policy, E, T):
    from tests.test_model_gpu import _make
    spec = LY.spec_of(name)
    lay, m, o = _make(spec['agent'], E, T, seed=LY.seed_of(name), policy=policy, scenario=spec['layout'], regime=regime, **spec['cfg'])
    plan, fc_path = _plan_of(spec, policy, E, m.G)
    assert m.H == spec['H'] and m.plan == plan and m.fc_path == fc_path, (name, policy, m.plan, m.fc_path)
    return lay, m, o


@pytest.mark.parametrize('sample', [True, False])
@pytest.mark.parametrize('regime,name,policy', LY.regime_forward_cases())
def test_regime_forward(regime, name, policy, sample):
    """Three advancing steps with random dones through forward_sample (sample) or forward: pi and v against the oracle, padded actions
    exactly 0, everything finite, rows of pi sum to 1 within 1e-5, the sampled action is np.random.choice on the kernel's own pi;
    onehot: pi exactly 1.0 at the chosen action and that action sampled for every (instance, agent)."""
    from oracle.nets_oracle import choice_from_uniform, sample_uniform
    E = LY.A2C_FORWARD_E
    lay, m, o = _a2c(regime, name, policy, E, 4)
    steps, boot = LY.forward_inputs(lay, E, LY.A2C_FORWARD_STEPS, np.random.RandomState(LY.data_seed(name, E)))
    hot = LY.onehot_action(lay)
    m.reset(); o.reset()
    for t, (obs, done) in enumerate(steps):
        d_obs, d_done = torch.from_numpy(obs).cuda(), torch.from_numpy(done).cuda()
        if sample:
            step = m.sample_step
            pi, v, act = m.forward_sample(d_obs, d_done, cache=False)
            act = act.cpu().numpy()
        else:
            pi, v = m.forward(d_obs, d_done, 'pv')
        pi, v = pi.cpu().numpy(), v.cpu().numpy()
        opi, ov = o.forward(obs, done, 'pv')
        assert np.isfinite(pi).all() and np.isfinite(v).all()
        for a, na in enumerate(lay.n_a_ls):
            np.testing.assert_allclose(pi[:, a, :na], opi[a], atol=2e-5, err_msg='pi t=%d a=%d' % (t, a))
            assert np.all(pi[:, a, na:] == 0)
            if regime == 'onehot':
                assert np.all(pi[:, a, hot[a]] == 1.0) and np.all(np.delete(pi[:, a, :na], hot[a], 1) == 0)
        np.testing.assert_allclose(v, ov, atol=value_bound(ov))
        assert np.abs(pi.sum(-1) - 1.0).max() <= 1e-5
        if sample:
            for e in range(E):
                for a, na in enumerate(lay.n_a_ls):
                    u = sample_uniform(m.sample_seed, step, e * lay.n_agent + a)
                    assert act[e, a] == choice_from_uniform(pi[e, a, :na], u), (t, e, a)
            if regime == 'onehot':
                np.testing.assert_array_equal(act, np.tile(np.asarray(hot, act.dtype), (E, 1)))
    vb = m.forward(torch.from_numpy(boot).cuda(), False, 'v').cpu().numpy()
    _, ovb = o.forward(boot, np.zeros(E), 'v')
    np.testing.assert_allclose(vb, ovb, atol=value_bound(ovb))
    m.close()


@pytest.mark.parametrize('use_cache', [True, False])
@pytest.mark.parametrize('regime,name,policy,E,T', LY.regime_cases())
def test_regime_update(regime, name, policy, E, T, use_cache):
    """Two update rounds (the body of test_backward_matches_oracle) in a regime: returns bit-exact, every gradient tensor, losses, norms,
    parameters after RMSProp.  half_clip: at LY.HALF_CLIP_LR, where a wrong clip factor moves a parameter by at least 100 x the
    parameter tolerance (module docstring).  onehot: every gradient entry of a policy tower is exactly 0.0 on the device (the softmax
    Jacobian of an exact one-hot vanishes), the value towers match the oracle, and the policy towers' parameters are bit-identical
    after the step."""
    from tests.test_model_gpu import _backward_vs_oracle
    lay, m, o = _a2c(regime, name, policy, E, T)
    before = m.get_flat().reshape(m.G, m.stride).copy()
    worst = {}
    flats = _backward_vs_oracle(lay, m, o, E, T, np.random.RandomState(LY.regime_data_seed(regime, name, policy, E, T)), False, use_cache,
                                worst=worst, lr=LY.HALF_CLIP_LR if regime == 'half_clip' else 5e-4)
    print('%s %s %s E=%d T=%d cache=%d: worst |dg| / max|g| %.1e / %.1e at %r / %r' % (regime, name, policy, E, T, use_cache, worst[0], worst[1],
                                                                                    worst['where', 0], worst['where', 1]))
    assert all(np.isfinite(f).all() for f in flats)
    if regime == 'onehot':
        after = m.get_flat().reshape(m.G, m.stride)
        for f in flats:
            assert np.all(f[0::2] == 0.0) and np.abs(f[1::2]).max() > 0
        np.testing.assert_array_equal(after[0::2], before[0::2])
        assert np.abs(after[1::2] - before[1::2]).max() > 0
    m.close()


def test_regime_ppo_peaked():
    """Two PPO epochs on head8 with a peaked policy against tests/ppo_oracle.py (the body of test_ppo_k2_on_a_ragged_split):
    head_bwd_kernel<true> where logp_old and logp are both log 1e-10 for a share of the samples.  Gradients (plus the ambiguous samples'
    own contributions, amb_slack) and parameters per epoch, clipped share, approximate KL.  tests/test_regimes_host.py states the case."""
    from tests.ppo_oracle import K3_REWARD_NORM, fill
    from tests.test_ppo_gpu import _check_grads, _check_params, _dev, _make, _put_copy
    spec = LY.A2C_LAYOUTS['head8']
    E, T, seed, rseed, lr = LY.REGIME_PPO
    lay, m, o = _make('ma2c', 'lstm', E, T, seed, layout=spec['layout'], regime='peaked', algo='ppo', ppo_epochs=2, reward_norm=K3_REWARD_NORM,
                      lr_init=lr, **spec['cfg'])
    assert m.plan == _plan_of(spec, 'lstm', E, m.G)[0]
    obs, _ = fill(lay, o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM, put=_put_copy(m))
    Rb = m.forward(_dev(obs), False, 'v').clone()
    for k in range(2):
        ograds, ostats = o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=k)
        m.compute_grads(Rb, k)
        worst = _check_grads(m, o, ograds, 2e-5 if k == 0 else 2e-4, slack=True, what='epoch %d' % k)
        stats = m.apply_grads(1.0, want_stats=True, epoch=k)
        onorm = o.apply_grads(ograds, lr, end_of_rollout=(k == 1))
        print('head8 peaked PPO epoch %d: worst |dg| / max|g| %.1e, clipped %.3f (gpu %.3f), kl %.4f (gpu %.4f)'
              % (k, worst, o.clip_share.mean(), stats[:, 4].mean(), o.approx_kl.mean(), stats[:, 5].mean()))
        if k == 1:
            assert 0.05 < o.clip_share.mean() < 0.95
        np.testing.assert_allclose(stats[:, 4], o.clip_share, rtol=2e-3, atol=o.amb_share.max() + 1e-12)
        np.testing.assert_allclose(stats[:, 5], o.approx_kl, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[:, 1:3], ostats[:, 1:], rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[:, 3], onorm, rtol=2e-3)
        _check_params(m, o, what='epoch %d' % k)
    m.close()


# ---- tsc_model_sample alone -----------------------------------------------------------------------------------------------------
def sampling_table(na):
    """Rows of n_a probabilities whose cdf has flat stretches: a single 1.0 at every position; two equal halves and an unequal pair
    (0.3, 0.7) at every pair of positions -- zeros before, between and after; a 1e-40 entry (a float32 denormal) on either side of a
    1.0; a row summing to 1 - 2e-7."""
    rows = []
    for i in range(na):
        rows.append({i: 1.0})
        for j in (i - 1, i + 1):
            if 0 <= j < na:
                rows.append({i: 1.0, j: 1e-40})
    for i, j in itertools.combinations(range(na), 2):
        rows += [{i: 0.5, j: 0.5}, {i: 0.3, j: 0.7}]
    out = np.zeros((len(rows) + 1, na), np.float32)
    for r, row in enumerate(rows):
        for k, p in row.items():
            out[r, k] = p
    out[-1] = 1.0 / na
    out[-1, -1] -= 2e-7
    assert 1 - 4e-7 < float(out[-1].astype(np.float64).sum()) < 1 - 5e-8          # (float32 entries: 1 - 2e-7 up to their rounding)
    return out


def test_sampling_table_is_numpy_choice_on_documented_uniform():
    """tsc_model_sample on the table above, every n_a from 2 to 8 (one agent each), at 64 step counters: exactly choice_from_uniform."""
    from deeprl_signal_control_amd.agents import VecA2C
    from oracle.nets_oracle import choice_from_uniform, sample_uniform
    lay = LY.Layout([(3, 1, 0, na) for na in range(2, 9)], 4)
    tabs = [sampling_table(na) for na in lay.n_a_ls]
    E, A = max(len(t) for t in tabs), lay.n_agent
    pi = np.zeros((E, A, 8), np.float32)
    for a, t in enumerate(tabs):
        pi[:, a, :t.shape[1]] = t[np.arange(E) % len(t)]
    m = VecA2C(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, lay.n_f_ls, E, lay.s_max, lay.a_max, dict(batch_size=2, num_fw=128, num_fp=0, num_ft=32), device=0,
               seed=17, name='ia2c')
    d_pi = torch.from_numpy(pi).cuda()
    seen = [set() for _ in range(A)]
    for step in list(range(60)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 3]:
        m.sample_step = step
        act = m.sample(d_pi).cpu().numpy()
        for e in range(E):
            for a, na in enumerate(lay.n_a_ls):
                u = sample_uniform(m.sample_seed, step, e * A + a)
                want = choice_from_uniform(pi[e, a, :na], u)
                assert act[e, a] == want and pi[e, a, want] > 0, (step, e, a, act[e, a], want)
                seen[a].add(want)
    assert all(seen[a] == set(range(na)) for a, na in enumerate(lay.n_a_ls))
    m.close()


# ---- the Q-learners (tests/layouts.py apply_iql_regime; one fused layout, one grouped, IQL-LR) -------------------------------------
def _iql(name, regime, monkeypatch, **cfg):
    spec = LY.IQL_LAYOUTS[name]
    monkeypatch.delenv('TSC_IQL_FUSED', raising=False)
    lay, m = H.model(spec['layout'], 'iql', spec['model_type'], LY.IQL_E, seed=LY.SEEDS[name], buffer_size=LY.IQL_CAP,
                    reward_norm=LY.IQL_REWARD_NORM, **spec['cfg'], **cfg)
    assert m.fused == spec['fused'], name
    m.set_agent_params(LY.apply_iql_regime(m.get_agent_params(), regime, name))
    if m.target_update:
        m.sync_target()
    return lay, m, H.oracle_for(m)


def _fill(lay, m, o, name):
    """LY.iql_transitions -- the draws of the host module -- into the handle's rings and the oracle's."""
    rng = np.random.RandomState(LY.data_seed(name, LY.IQL_E, LY.IQL_CAP))
    for obs, act, rew, nobs, done in LY.iql_transitions(lay, LY.IQL_E, LY.IQL_CAP, rng, LY.IQL_REWARD_NORM):
        m.add_transition(*[torch.from_numpy(x).cuda() for x in (obs, act, rew, nobs, done)])
        o.add_transition(obs, act, rew, nobs, done)


def _step(m, o, lr):
    """One minibatch step of the library's own draw on both sides: draw, loss, clip norm and every gradient tensor compared
    -> (agents on a ReLU kink, oracle norms, device parameters before / after, oracle parameters before / after, per agent)."""
    A = m.n_agent
    before = m.layout.unpack(m.get_flat())
    H.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = H.batch(m)
    flat_g = m.grad_tensor().cpu().numpy().copy()
    stats = np.zeros((A, 2))
    H.check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(H.C.c_void_p)))
    obefore = [{k: v.numpy().copy() for k, v in q.p.items()} for q in o.qs]
    params_before, rows_before = H.snapshot(o)
    losses, norms, og = o.minibatch_step(lr)
    np.testing.assert_array_equal(idx, o.last_idx)
    kinked = H.compare_grads(m, o, m.layout.unpack(flat_g), og, idx, params_before, rows_before)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
    return kinked, norms, before, m.layout.unpack(m.get_flat()), obefore, [{k: v.numpy().copy() for k, v in q.p.items()} for q in o.qs], flat_g


@pytest.mark.parametrize('name', LY.IQL_REGIME_LAYOUTS)
def test_iql_tied_first_maximum(name, monkeypatch):
    """Two head columns j < k of every agent identical, the others 50 below: the two Q values are bit-equal on the device, mode 'act'
    takes j on every row (iql_act_kernel / iql_fused_act_kernel: the first maximum, as np.argmax), Double DQN's a* is j on every sampled
    row (iql_qsel_kernel / the fused target kernel) and the TD target is the oracle's, which uses that value."""
    lay, m, o = _iql(name, 'tied', monkeypatch, target_update=100, double_q=1)
    E, A = LY.IQL_E, lay.n_agent
    rng = np.random.RandomState(LY.data_seed(name, E))
    pairs = [LY.tie_pair(a, na) for a, na in enumerate(lay.n_a_ls)]
    for t in range(3):
        obs = LY.rand_obs(lay, E, rng)
        act, q = m.forward(torch.from_numpy(obs).cuda())
        act, q = act.cpu().numpy(), q.cpu().numpy()
        oq = o.forward(obs)
        for a, (j, k) in enumerate(pairs):
            np.testing.assert_allclose(q[:, a, :lay.n_a_ls[a]], oq[a], atol=value_bound(oq[a]))     # the lowered columns sit near -50
            np.testing.assert_allclose(q[:, a, j], oq[a][:, j], atol=2e-5)
            assert np.array_equal(q[:, a, j], q[:, a, k]), 'agent %d: columns %d and %d differ on the device' % (a, j, k)
            assert (act[:, a] == j).all(), (a, j, act[:, a])
        H.explored(lay, m, obs, E)
    _fill(lay, m, o, name)
    H.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = H.batch(m)
    y, astar = H.targets(m)
    o.minibatch_step(1e-3)
    np.testing.assert_array_equal(idx, o.last_idx)
    for a, (j, k) in enumerate(pairs):
        # (the oracle's float64 matmul over the 100 rows of a minibatch blocks the head's columns and may round two identical columns an
        # ulp apart, so its own argmax is j or k; evaluated instance by instance they are bit-equal, tests/test_regimes_host.py.  Either
        # way its target is the tied value.)
        qa = o.qs[a]
        assert np.abs(qa.last_q1_online[:, j] - qa.last_q1_online[:, k]).max() <= 1e-14 and np.isin(qa.last_astar, (j, k)).all()
        assert (astar[a] == j).all(), (a, j, astar[a])
        np.testing.assert_allclose(y[a], qa.last_y, rtol=0, atol=2e-5)
    m.close()


@pytest.mark.parametrize('name', LY.IQL_REGIME_LAYOUTS)
def test_iql_flat_head(name, monkeypatch):
    """Head weights and bias zero: Q is exactly 0, the greedy action is 0 for every n_a (every action ties), and one minibatch step
    matches the oracle -- draw, loss, norm, every gradient tensor (the tensors below the head: exactly zero on both sides), and
    Adam's step on the entries whose gradient is not rounding noise (the rule of iql_harness.replay_vs_oracle)."""
    lay, m, o = _iql(name, 'flat', monkeypatch)
    E = LY.IQL_E
    rng = np.random.RandomState(LY.data_seed(name, E))
    for t in range(3):
        obs = LY.rand_obs(lay, E, rng)
        act, q = m.forward(torch.from_numpy(obs).cuda())
        assert (q.cpu().numpy() == 0).all() and (act.cpu().numpy() == 0).all()
        H.explored(lay, m, obs, E)
    _fill(lay, m, o, name)
    lr = 1e-3
    kinked, norms, b, a_, ob, oa, flat_g = _step(m, o, lr)
    g = m.layout.unpack(flat_g)
    for a in range(lay.n_agent):
        for k in g[a]:
            if k not in ('q_w', 'q_b'):
                assert (g[a][k] == 0).all(), (a, k)
            real = np.abs(g[a][k]) > 1e-2 * max(np.abs(x).max() for x in g[a].values())
            d_hip, d_orc = a_[a][k] - b[a][k], oa[a][k] - ob[a][k]
            assert np.abs(d_hip).max() <= 1.01 * lr
            if real.any() and a not in kinked:
                assert np.abs(d_hip - d_orc)[real].max() <= 2e-6, (a, k)
    m.close()


@pytest.mark.parametrize('name', LY.IQL_REGIME_LAYOUTS)
def test_iql_clip_binds_for_some_agents(name, monkeypatch):
    """iql_adam_kernel's per-agent factor clip / max(norm, clip) with agents on both sides of max_grad_norm in one launch, three Adam steps
    against the oracle.  Adam's normalisation hides a constant factor, so the second moments are preloaded with 1 (first moments 0,
    t = 0) on both sides: a step is then nearly linear in the clipped gradient, and a step taken with factor 1 is off by at least 100 x
    the bound used here (LY.adam_step_bound; tests/test_regimes_host.py measures 326 x to 20 331 x)."""
    lay, m, o = _iql(name, 'clip', monkeypatch)
    _fill(lay, m, o, name)
    z, ones = np.zeros(m.n_param, np.float32), np.ones(m.n_param, np.float32)
    H.check(m._L.tsc_iql_set_opt_state(m._h, z.ctypes.data_as(H.C.c_void_p), ones.ctypes.data_as(H.C.c_void_p), 0))
    for q in o.qs:
        q.v = {k: torch.ones_like(v) for k, v in q.p.items()}
    for step in range(LY.IQL_CLIP_STEPS):
        kinked, norms, b, a_, ob, oa, _ = _step(m, o, LY.IQL_CLIP_LR)
        assert (norms < 0.99 * 40).any() and (norms > 1.01 * 40).any()
        worst = 0.0
        for a in range(lay.n_agent):
            if a in kinked:
                continue
            for k in b[a]:
                d_hip, d_orc = a_[a][k].astype(np.float64) - b[a][k], oa[a][k] - ob[a][k]
                bound = LY.adam_step_bound(d_orc, b[a][k])
                worst = max(worst, float(np.abs(d_hip - d_orc).max()) / bound)
                assert np.abs(d_hip - d_orc).max() <= bound, 'step %d agent %d %s: %.2e > %.2e' % (step, a, k, np.abs(d_hip - d_orc).max(), bound)
        print('%s clip step %d: norms %.1f ... %.1f, worst step error %.2f of the bound' % (name, step, norms.min(), norms.max(), worst))
        assert H.sync_oracle(m, o) == step + 1
    m.close()
