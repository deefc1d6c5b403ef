"""Host-side conditions of tests/test_layouts_gpu.py, on the oracles alone (no GPU, no library): for every layout of tests/layouts.py
and the seeds of its table, the very inputs of the GPU module go through OracleA2C / OracleIQL and through their float32 restatement
(the same code in torch float32 on the CPU, layouts.f32_oracle_class), and

  * at most 4 hidden columns of a tower fall under the ReLU-kink exception of _grad_err / iql_harness.kinks in any round (and no second-layer
    unit of a Q-net sits on a kink: that would take every tensor below the head out of the comparison);
  * every action of every agent has an oracle probability in (1e-4, 1 - 1e-4) on some sample: no head is saturated, no gradient
    vacuous (a saturated softmax passes any kernel);
  * the second-round gradients of the float32 restatement, whose parameters carry the first update's float32 rounding exactly as the
    kernel's do, stay inside the 2e-4 allowance of the second round against float64 -- the allowance is wide enough for a correct
    float32 evaluation of these layouts, so a GPU failure there is the kernel's;
  * the float32 restatement's values stay inside the bound the GPU module uses for v and Q, 2e-5 max(1, max|oracle value|): layouts
    with up to 68 inputs in [0, 2) produce larger values than the reference's ranges do.

The seeds of tests/layouts.py were chosen so that this passes; the GPU module imports the same table."""
import numpy as np
import pytest
import torch

from tests import layouts as LY


def value_bound(ov):
    """The bound on |dv| / |dQ| of a layout: 2e-5 max(1, max|oracle value|) (tests/test_layouts_gpu.py uses the same function)."""
    return 2e-5 * max(1.0, float(np.abs(ov).max()))


def _a2c_pair(name, policy, E):
    from deeprl_signal_control_amd.agents import A2C_DEFAULTS, init_tower_params
    from oracle.nets_oracle import OracleA2C
    spec = LY.A2C_LAYOUTS[name]
    lay, c = spec['layout'], dict(A2C_DEFAULTS, **spec['cfg'])
    ma = spec['agent'] == 'ma2c'
    n_f = lay.n_f_ls if ma else [0] * lay.n_agent
    n_fc = (c['num_fw'], c['num_fp'] if ma else 0, c['num_ft'] if max(lay.n_w_ls) > 0 else 0)
    towers = init_tower_params(lay.n_wave_ls, lay.n_w_ls, n_f, lay.n_a_ls, n_fc, 64, policy, np.random.RandomState(LY.SEEDS[name]))
    kw = dict(gamma=c['gamma'], reward_norm=c['reward_norm'], reward_clip=c['reward_clip'], value_coef=c['value_coef'],
              max_grad_norm=c['max_grad_norm'])
    o64 = OracleA2C(towers, lay.n_wave_ls, lay.n_w_ls, n_f, lay.n_a_ls, E, **kw)
    o32 = LY.f32_oracle_class(OracleA2C)(towers, lay.n_wave_ls, lay.n_w_ls, n_f, lay.n_a_ls, E, **kw)
    assert o32.p[0]['fcw_w'].dtype == torch.float32 and o64.p[0]['fcw_w'].dtype == torch.float64
    return lay, c, o64, o32


def _open_heads(lay, pis):
    """Every action of every agent: an oracle probability in (1e-4, 1 - 1e-4) on some sample of pis (list over steps of list[A])."""
    for a in range(lay.n_agent):
        p = np.concatenate([step[a] for step in pis], 0)
        ok = ((p > 1e-4) & (p < 1 - 1e-4)).any(0)
        assert ok.all(), 'agent %d: actions %s are saturated on every sample' % (a, np.nonzero(~ok)[0])


A2C_CASES = [(n, p) for n in LY.A2C_LAYOUTS for p in ('lstm', 'fc')]


@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_forward_conditions(name, policy):
    E = LY.A2C_FORWARD_E
    lay, c, o64, o32 = _a2c_pair(name, policy, E)
    steps, boot = LY.forward_inputs(lay, E, LY.A2C_FORWARD_STEPS, np.random.RandomState(LY.data_seed(name, E)))
    pis, worst, vmax = [], 0.0, 0.0
    for obs, done in steps:
        pi, v = o64.forward(obs, done, 'pv')
        pi32, v32 = o32.forward(obs, done, 'pv')
        pis.append(pi)
        assert np.abs(v32 - v).max() <= value_bound(v)
        assert max(np.abs(a - b).max() for a, b in zip(pi, pi32)) <= 2e-5
        worst, vmax = max(worst, np.abs(v32 - v).max()), max(vmax, np.abs(v).max())
    _, vb = o64.forward(boot, np.zeros(E), 'v')
    _, vb32 = o32.forward(boot, np.zeros(E), 'v')
    assert np.abs(vb32 - vb).max() <= value_bound(vb)
    print('%s %s: max|v| %.2f, float32 restatement |dv| %.1e (bound %.1e)' % (name, policy, vmax, worst, 2e-5 * max(1.0, vmax)))
    _open_heads(lay, pis)


@pytest.mark.parametrize('E,T', LY.A2C_BATCHES)
@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_update_conditions(name, policy, E, T):
    from tests.test_model_gpu import _grad_err
    lay, c, o64, o32 = _a2c_pair(name, policy, E)
    rng = np.random.RandomState(LY.data_seed(name, E, T))
    pis = []
    for it in range(2):
        obs, done, p = LY.fill_host(lay, [o64, o32], E, T, rng, c['reward_norm'])
        pis += p
        _, Rb = o64.forward(obs, np.zeros(E), 'v')
        o32.forward(obs, np.zeros(E), 'v')
        Rb = Rb.astype(np.float32)
        g64, _ = o64.compute_grads(Rb, 0.01)
        g32, _ = o32.compute_grads(Rb, 0.01)
        np.testing.assert_array_equal(o64.Rs, o32.Rs)
        worst = 0.0
        for t, kc in enumerate(o64.kink_cols):
            n_kink = sum(int(cols.sum()) for cols in kc.values())
            assert n_kink <= 4, 'round %d tower %d: %d hidden columns on a ReLU kink' % (it, t, n_kink)
            for k, og in g64[t].items():
                assert float(og.abs().max()) > 0, 'round %d tower %d %s: the oracle gradient is zero' % (it, t, k)
                err = _grad_err(o64, t, k, g32[t][k].double().numpy(), og.numpy())
                worst = max(worst, err)
                assert err <= (2e-5 if it == 0 else 2e-4), 'round %d tower %d %s: float32 restatement |dg| / max|g| = %.2e' % (it, t, k, err)
        print('%s %s E=%d T=%d round %d: float32 restatement worst |dg| / max|g| %.1e' % (name, policy, E, T, it, worst))
        o64.apply_grads(g64, 5e-4)
        o32.apply_grads(g32, 5e-4)
    _open_heads(lay, pis)


def _iql_pair(name):
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, QParamLayout, init_agent_params
    from oracle.iql_oracle import OracleIQL
    spec = LY.IQL_LAYOUTS[name]
    lay, c = spec['layout'], dict(IQL_DEFAULTS, **spec['cfg'])
    ql = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, spec['model_type'], c['num_fc'], c['num_h'])
    params = init_agent_params(ql, np.random.RandomState(LY.SEEDS[name]))
    kw = dict(batch_size=20, buffer_size=LY.IQL_CAP, gamma=c['gamma'], reward_norm=LY.IQL_REWARD_NORM, reward_clip=c['reward_clip'],
              max_grad_norm=c['max_grad_norm'], replay_seed=LY.SEEDS[name] ^ 0x5DEECE66D)
    o64 = OracleIQL(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, LY.IQL_E, **kw)
    o32 = LY.f32_oracle_class(OracleIQL)(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, LY.IQL_E, **kw)
    return lay, o64, o32


@pytest.mark.parametrize('name', list(LY.IQL_LAYOUTS))
def test_iql_conditions(name):
    from tests.iql_harness import kinks
    lay, o64, o32 = _iql_pair(name)
    E, A = LY.IQL_E, lay.n_agent
    rng = np.random.RandomState(LY.data_seed(name, E))
    qmax, worst = 0.0, 0.0
    for t in range(3):                                                  # forward_and_act's observations
        obs = LY.rand_obs(lay, E, rng)
        for q, q32 in zip(o64.forward(obs), o32.forward(obs)):
            assert np.abs(q32 - q).max() <= value_bound(q)
            qmax, worst = max(qmax, np.abs(q).max()), max(worst, np.abs(q32 - q).max())
    print('%s: max|Q| %.2f, float32 restatement |dQ| %.1e (bound %.1e)' % (name, qmax, worst, 2e-5 * max(1.0, qmax)))
    rng = np.random.RandomState(LY.data_seed(name, E, LY.IQL_CAP))
    for tr in LY.iql_transitions(lay, E, LY.IQL_CAP, rng, LY.IQL_REWARD_NORM):
        o64.add_transition(*tr)
        o32.add_transition(*tr)
    for step in range(LY.IQL_STEPS):
        rows = [[o64.rings[e][a].buffer for e in range(E)] for a in range(A)]
        before = [{k: v.clone() for k, v in q.p.items()} for q in o64.qs]
        _, _, g64 = o64.minibatch_step(1e-3)
        _, _, g32 = o32.minibatch_step(1e-3)
        np.testing.assert_array_equal(o64.last_idx, o32.last_idx)
        for a in range(A):
            saved, o64.qs[a].p = o64.qs[a].p, before[a]
            cols, deep = kinks(o64, [rows[a][e][s][0] for e in range(E) for s in o64.last_idx[e, a]], a)
            o64.qs[a].p = saved
            assert not deep, 'step %d agent %d: a second-layer unit on a ReLU kink' % (step, a)
            assert cols is None or cols.sum() <= 4, 'step %d agent %d: %d first-layer columns on a ReLU kink' % (step, a, cols.sum())
            for k, ref in g64[a].items():
                err, scale = np.abs(g32[a][k] - ref), max(np.abs(ref).max(), 1e-9)
                assert np.abs(ref).max() > 0, (step, a, k)
                if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                    n0 = before[a]['fcw_b'].shape[0]
                    sel = cols[:n0] if k.startswith('fcw') else cols[n0:]
                    err = err[..., ~sel] if err.ndim == 2 else err[~sel]
                assert err.size == 0 or err.max() <= 2e-5 * scale, 'step %d agent %d %s: float32 restatement %.2e' % (step, a, k, err.max() / scale)
        for q64, q32 in zip(o64.qs, o32.qs):        # the next step starts from one state on both sides, as on the GPU
            for k in q64.p:
                q32.p[k], q32.m[k], q32.v[k] = q64.p[k].float(), q64.m[k].float(), q64.v[k].float()


def test_ppo_head8_conditions():
    """The K = 3 case of the GPU module on head8 (MA2C, LSTM): the clip branch is exercised and few samples sit on a clip bound
    (tests/ppo_oracle.py k3_conditions), on the oracle alone."""
    from tests.ppo_oracle import K3_REWARD_NORM, fill, k3_conditions, make_oracle
    spec = LY.A2C_LAYOUTS['head8']
    E, T, seed, rseed, lr = LY.PPO_HEAD8
    o = make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=dict(spec['cfg'], reward_norm=K3_REWARD_NORM), layout=spec['layout'])
    o.reset()
    obs, _ = fill(spec['layout'], o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM)
    _, Rb = o.forward(obs, np.zeros(E), 'v')
    for k in range(3):
        g, _ = o.compute_grads(Rb.astype(np.float32), 0.01, epoch=k, slack=False)
        clip, amb = k3_conditions(o, k)
        print('head8 epoch %d: clipped share %.3f, ambiguous %.4f' % (k, clip, amb))
        o.apply_grads(g, lr, end_of_rollout=(k == 2))


def test_layout_tables_are_consistent():
    for name, spec in LY.A2C_LAYOUTS.items():
        lay = spec['layout']
        assert 3 <= lay.n_agent <= 6 and lay.a_max <= 8 and spec['H'] % 4 == 0, name
        if spec['agent'] == 'ma2c':
            assert min(lay.n_f_ls) >= 1, name
        else:
            assert max(lay.n_f_ls) == 0, name
    assert LY.A2C_REFUSED['H'] % 4 != 0
    for name, spec in LY.IQL_LAYOUTS.items():
        lay = spec['layout']
        fits = max(lay.n_w_ls) == 0 or (max(lay.n_wave_ls) <= 32 and max(lay.n_w_ls) <= 16)
        want = spec['model_type'] == 'dqn' and spec['cfg'] == dict(num_fc=128, num_h=64) and lay.s_max <= 48 and fits
        assert spec['fused'] == want, name
    assert set(LY.SEEDS) == set(LY.A2C_LAYOUTS) | set(LY.IQL_LAYOUTS)
