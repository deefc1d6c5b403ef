"""Host-side checks of the opt-in dueling head of IQL-DNN ([MODEL_CONFIG] dueling; deeprl_signal_control_amd/iql.py dueling_config,
QParamLayout(dueling=True)) and self-checks of its float64 oracle (tests/iql_ext_oracle.py) -- no GPU."""
import configparser

import numpy as np
import pytest
import torch

from deeprl_signal_control_amd.agents import coerce_config
from deeprl_signal_control_amd.iql import IQL_DEFAULTS, QParamLayout, init_agent_params

# a tiny net with heterogeneous action counts: wave widths, wait widths, actions
N_WAVE, N_WAIT, N_A = [5, 3, 7], [2, 1, 4], [2, 4, 6]
S_MAX, N_FC0, N_H = 12, 8, 4


def _layout(dueling):
    return QParamLayout(N_WAVE, N_WAIT, N_A, S_MAX, 'dqn', N_FC0, N_H, dueling=dueling)


def test_dueling_config_defaults_strings_and_bad_values():
    from deeprl_signal_control_amd.iql import dueling_config
    assert IQL_DEFAULTS['dueling'] == 0
    assert dueling_config(coerce_config(None, IQL_DEFAULTS)) == 0
    assert dueling_config(coerce_config({'dueling': 1}, IQL_DEFAULTS)) == 1
    cp = configparser.ConfigParser()
    cp.read_string('[MODEL_CONFIG]\ndueling = 1\ndouble_q = 1\ntarget_update = 10\nprioritized_replay = 1\n')
    assert dueling_config(coerce_config(cp['MODEL_CONFIG'], IQL_DEFAULTS)) == 1
    cp.read_string('[MODEL_CONFIG]\nDUELING = 0\n')
    assert dueling_config(coerce_config(cp['MODEL_CONFIG'], IQL_DEFAULTS)) == 0
    for bad in (2, -1, '3', 0.5, 'yes'):
        with pytest.raises(ValueError, match='dueling'):
            dueling_config(coerce_config({'dueling': bad}, IQL_DEFAULTS) if not isinstance(bad, str) or bad.isdigit()
                           else dict(coerce_config(None, IQL_DEFAULTS), dueling=bad))


def test_layout_tuple_is_the_same_with_and_without_dueling():
    plain, duel = _layout(False), _layout(True)
    assert plain.as_tuple() == duel.as_tuple() and plain.n_param == duel.n_param
    for a in range(3):
        sp, sd = plain.shapes(a), duel.shapes(a)
        assert list(sd)[:len(sp)] == list(sp) and list(sd)[len(sp):] == ['v_w', 'v_b']          # the value stream is created after q
        assert sd['v_w'] == (N_H, 1) and sd['v_b'] == (1,)


def test_dueling_layout_refuses_lr_and_eight_actions():
    with pytest.raises(ValueError, match='dueling'):
        QParamLayout(N_WAVE, N_WAIT, N_A, S_MAX, 'lr', N_FC0, N_H, dueling=True)
    with pytest.raises(ValueError, match='dueling'):
        QParamLayout(N_WAVE, N_WAIT, [2, 8, 6], S_MAX, 'dqn', N_FC0, N_H, dueling=True)


def test_pack_unpack_round_trip_with_the_value_stream_in_column_7():
    lay = _layout(True)
    rng = np.random.RandomState(1)
    agents = [{k: rng.randn(*sh).astype(np.float32) for k, sh in lay.shapes(a).items()} for a in range(lay.A)]
    flat = lay.pack(agents)
    back = lay.unpack(flat)
    for p, q in zip(agents, back):
        assert sorted(p) == sorted(q)
        for k in p:
            np.testing.assert_array_equal(p[k], q[k])
    f = flat.reshape(lay.A, lay.stride)
    for a, p in enumerate(agents):
        Wq = f[a, lay.oWq:lay.obq].reshape(lay.H2, 8)
        np.testing.assert_array_equal(Wq[:, 7], p['v_w'][:, 0])
        assert f[a, lay.obq + 7] == p['v_b'][0]
        assert (Wq[:, N_A[a]:7] == 0).all() and (f[a, lay.obq + N_A[a]:lay.obq + 7] == 0).all()
        np.testing.assert_array_equal(Wq[:, :N_A[a]], p['q_w'])
    # a plain layout reads the same buffer without the value stream, and packs column 7 as zeros
    plain = _layout(False)
    for p, q in zip(agents, plain.unpack(flat)):
        assert 'v_w' not in q and all(np.array_equal(q[k], p[k]) for k in q)
    assert (plain.pack(agents).reshape(lay.A, lay.stride)[:, lay.obq + 7] == 0).all()


def test_one_seed_draws_the_same_existing_tensors_with_and_without_dueling():
    plain = init_agent_params(_layout(False), np.random.RandomState(7))
    duel = init_agent_params(_layout(True), np.random.RandomState(7))
    # the value streams are drawn behind all agents' existing tensors, so every one of those is bit-identical
    for p, d in zip(plain, duel):
        assert list(d)[:len(p)] == list(p) and list(d)[len(p):] == ['v_w', 'v_b']
        for k, v in p.items():
            np.testing.assert_array_equal(d[k], v)
        assert d['v_w'].shape == (N_H, 1) and np.abs(d['v_w']).max() > 0 and (d['v_b'] == 0).all()
    assert not np.array_equal(duel[0]['v_w'], duel[1]['v_w'])


def _oracle_and_rows(rng):
    from tests.iql_ext_oracle import ExtOracleIQL
    lay = _layout(True)
    agents = [{k: rng.randn(*sh) * 0.5 for k, sh in lay.shapes(a).items()} for a in range(lay.A)]
    o = ExtOracleIQL(agents, N_WAVE, N_WAIT, N_A, 1, batch_size=6, buffer_size=8, reward_norm=1.0, reward_clip=0.0)
    return lay, agents, o


def test_oracle_gradient_structure():
    """sum_{j < n_a} dq_w[:, j] = 0 (the mean is subtracted), dv_b = sum over rows of g = dLoss/dQ[a]."""
    rng = np.random.RandomState(2)
    lay, agents, o = _oracle_and_rows(rng)
    for a, q in enumerate(o.qs):
        n, R = N_WAVE[a] + N_WAIT[a], 9
        obs, nobs = rng.rand(R, n) * 2, rng.rand(R, n) * 2
        acts, rs, dones = rng.randint(0, N_A[a], R), -rng.rand(R), rng.rand(R) < 0.3
        loss, g = q.loss_and_grads(obs, acts, nobs, dones, rs)
        assert set(g) == set(agents[a]) and g['q_w'].shape == (N_H, N_A[a]) and g['v_w'].shape == (N_H, 1)
        assert g['q_w'].sum(1).abs().max() <= 1e-12 and abs(g['q_b'].sum().item()) <= 1e-12
        grow = 2.0 * q.last_delta / R
        np.testing.assert_allclose(g['v_b'].numpy(), [grow.sum()], rtol=0, atol=1e-12)
        assert abs(loss - (q.last_delta ** 2).mean()) <= 1e-12
        assert np.abs(g['v_w'].numpy()).max() > 0


def test_oracle_q_is_invariant_to_a_constant_on_the_advantage_biases():
    from oracle.iql_oracle import DT
    from tests.iql_ext_oracle import q_net_duel
    rng = np.random.RandomState(4)
    lay, agents, o = _oracle_and_rows(rng)
    for a, q in enumerate(o.qs):
        S = torch.as_tensor(rng.rand(11, N_WAVE[a] + N_WAIT[a]) * 2, dtype=DT)
        base = q_net_duel(q.p, S, q.n_s, q.n_w)
        shifted = dict(q.p, q_b=q.p['q_b'] + 0.37)
        assert (q_net_duel(shifted, S, q.n_s, q.n_w) - base).abs().max() <= 1e-12
        moved = dict(q.p, v_b=q.p['v_b'] + 0.37)                    # ... while the value bias moves every action alike
        assert ((q_net_duel(moved, S, q.n_s, q.n_w) - base) - 0.37).abs().max() <= 1e-12
        assert base.shape == (11, N_A[a])


def _fill_rings(oracles, E, rng, n=11):
    for t in range(n):
        tr = (rng.rand(E, 3, S_MAX) * 2, np.stack([rng.randint(0, k, E) for k in N_A], 1), -rng.rand(E, 3) * 3, rng.rand(E, 3, S_MAX) * 2,
              rng.rand(E) < 0.2)
        for o in oracles:
            o.add_transition(*tr)


def test_every_option_off_is_the_reference_oracle_bit_for_bit():
    """ExtOracleIQL without target network, Double DQN, prioritized replay and value stream against oracle.iql_oracle.OracleIQL over three
    minibatch steps: a weight of exactly 1 and theta- = theta change no bit of the losses, norms, gradients and parameters."""
    from oracle.iql_oracle import OracleIQL
    from tests.iql_ext_oracle import ExtOracleIQL
    rng = np.random.RandomState(5)
    lay = _layout(False)
    agents = [{k: rng.randn(*sh) * 0.5 for k, sh in lay.shapes(a).items()} for a in range(lay.A)]
    kw = dict(batch_size=6, buffer_size=8, reward_norm=1.0, reward_clip=0.0, replay_seed=3)
    ref, ext = OracleIQL(agents, N_WAVE, N_WAIT, N_A, 2, **kw), ExtOracleIQL(agents, N_WAVE, N_WAIT, N_A, 2, **kw)
    _fill_rings([ref, ext], 2, rng)
    for step in range(3):
        l0, n0, g0 = ref.minibatch_step(1e-2)
        l1, n1, g1 = ext.minibatch_step(1e-2)
        np.testing.assert_array_equal(l0, l1)
        np.testing.assert_array_equal(n0, n1)
        np.testing.assert_array_equal(ref.last_idx, ext.last_idx)
        for a in range(lay.A):
            assert list(g0[a]) == list(g1[a])
            for k in g0[a]:
                np.testing.assert_array_equal(g0[a][k], g1[a][k])
                assert torch.equal(ref.qs[a].p[k], ext.qs[a].p[k]), (step, a, k)
        assert (ext.last_w == 1).all() and (ext.prio == 0).all()


def test_float32_restatement_runs_with_every_option_on():
    """layouts.f32_oracle_class(ExtOracleIQL) with target network + Double DQN + prioritized replay + dueling head: one step in float32
    throughout, and its parameters at float32 distance of the float64 run.  The first Adam step of a component with gradient g is
    lr f(g), f(x) = x / (|x| + c), c = 1e-8 / sqrt(1 - beta2) (m = (1 - beta1) g, v = (1 - beta2) g^2 and Adam's bias correction), f
    increasing; with the float32 gradient within e = 2e-5 max|g| of g (the first-round allowance of tests/test_layouts_host.py, asserted
    here too), the step moves by at most lr max(f(g + e) - f(g), f(g) - f(g - e)), plus a few float32 roundings of the parameter."""
    from tests import layouts as LY
    from tests.iql_ext_oracle import ExtOracleIQL
    rng = np.random.RandomState(6)
    lay, lr, E = _layout(True), 1e-3, 2
    agents = [{k: rng.randn(*sh) * 0.5 for k, sh in lay.shapes(a).items()} for a in range(lay.A)]
    other = [{k: v + rng.randn(*v.shape) * 0.1 for k, v in p.items()} for p in agents]
    kw = dict(per=True, alpha=0.6, eps=0.01, target_update=2, double_q=True, batch_size=6, buffer_size=8, reward_norm=1.0, reward_clip=0.0,
              replay_seed=3)
    o64 = ExtOracleIQL(agents, N_WAVE, N_WAIT, N_A, E, **kw)
    o32 = LY.f32_oracle_class(ExtOracleIQL)(agents, N_WAVE, N_WAIT, N_A, E, **kw)
    assert o64.qs[0].p['q_w'].dtype == torch.float64 and o32.qs[0].p['q_w'].dtype == torch.float32
    _fill_rings([o64, o32], E, rng)
    prio = (rng.rand(E, lay.A, 8) + 0.05).astype(np.float32)
    for o in (o64, o32):
        o.set_target_params(other)
        o.prio[:] = prio
    before = [{k: v.clone() for k, v in q.p.items()} for q in o64.qs]
    _, n64, g64 = o64.minibatch_step(lr, beta=0.4)
    _, n32, g32 = o32.minibatch_step(lr, beta=0.4)
    np.testing.assert_array_equal(o64.last_idx, o32.last_idx)
    assert o64.last_w.min() < 1 and n64.max() < 40.0 and n32.max() < 40.0                     # weighted rows, no clipping on either side
    c = 1e-8 / np.sqrt(1e-3)
    f = lambda x: x / (np.abs(x) + c)
    for a, (q64, q32) in enumerate(zip(o64.qs, o32.qs)):
        assert q32.target['v_w'].dtype == torch.float32 and q32.last_y.dtype == np.float32 and q32.last_astar is not None
        for k, g in g64[a].items():
            assert g32[a][k].dtype == np.float32 and q32.p[k].dtype == torch.float32
            e = 2e-5 * np.abs(g).max()
            assert e > 0 and np.abs(g32[a][k] - g).max() <= e, (a, k)
            bound = 2.0 ** -22 * max(1.0, float(before[a][k].abs().max())) + lr * np.maximum(f(g + e) - f(g), f(g) - f(g - e))
            assert (np.abs(q32.p[k].double().numpy() - q64.p[k].numpy()) <= bound).all(), (a, k)
            assert float((q64.p[k] - before[a][k]).abs().max()) > 0.5 * lr                    # ... and the step was taken
