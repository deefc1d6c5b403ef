"""GPU tests of the opt-in target network / Double DQN of the Q-learners ([MODEL_CONFIG] target_update / double_q; include/tsc.h
tsc_iql_set_target; csrc/tsc_iql_fused.h iql_fused_target_kernel and iql_fused_grad_kernel<.., true>, csrc/tsc_iql.hip for the
grouped-GEMM path) against the float64 restatement of tests/iql_ext_oracle.py.

Shapes: the smallest at which each path can go wrong, by the reasoning of tests/test_iql_gpu.py -- E = 70 x batch 20 = 1400 rows =
21 x 64 + 56 (several row splits, a ragged last chunk), E = 3 one partial chunk, the grouped-GEMM path for IQL-DNN (TSC_IQL_FUSED=0)
and IQL-LR, small_grid for the instantiation without a wait tile, real_net for heterogeneous action counts.

Tolerances are the project's (tests/test_iql_gpu.py): Q values, hence y = r + gamma Q, |d| <= 2e-5; gradients |d| <= 2e-5 max|g| per
tensor with hidden units within 1e-6 of a ReLU kink excepted; loss and clip norm rtol 1e-4; a* exact on every row (rows whose two
best online values lie within 1e-4 of each other in float64 are re-drawn before they enter the rings, and none may remain)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_iql_gpu import _kinks, _rand_obs

pytestmark = pytest.mark.gpu

# scenario, agent, model_type, E, ring capacity, TSC_IQL_FUSED
CASES = [('large_grid', 'iqld', 'dqn', 70, 22, '1'), ('large_grid', 'iqld', 'dqn', 3, 25, '1'), ('large_grid', 'iqld', 'dqn', 6, 30, '0'),
         ('large_grid', 'iqll', 'lr', 9, 1000, '0'), ('small_grid', 'iqld', 'dqn', 7, 40, '1'), ('real_net', 'iqld', 'dqn', 4, 64, '1')]
GAP = 1e-4


def _model(scenario, agent, model_type, E, seed=5, **cfg):
    """scenario: the name of a built-in scenario, or a layout object (tests/layouts.py: the attributes read below and nothing else)."""
    from deeprl_signal_control_amd.iql import VecIQL
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(scenario, agent) if isinstance(scenario, str) else scenario
    mc = dict(batch_size=20, buffer_size=1000, reward_norm=3000.0 if scenario == 'large_grid' else 1.0 if scenario == 'real_net' else 100.0)
    mc.update(cfg)
    a_max = int(scn.green_tab.shape[1]) if hasattr(scn, 'green_tab') else scn.a_max
    m = VecIQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, E, scn.s_max, a_max, mc, total_step=10000, seed=seed,
               model_type=model_type)
    return scn, m


def _oracle(m, target_update, double_q):
    from tests.iql_ext_oracle import ExtOracleIQL
    return ExtOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, target_update=target_update, double_q=double_q,
                           batch_size=m.n_step, buffer_size=int(m.cfg['buffer_size']), gamma=m.cfg['gamma'],
                           reward_norm=m.cfg['reward_norm'], reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'],
                           replay_seed=m.replay_seed)


def _online_gap(o, obs, a):
    """top-two gap of agent a's float64 online Q over the rows obs [n, n_s]."""
    from oracle.iql_oracle import DT, q_net
    with torch.no_grad():
        q = q_net(o.qs[a].p, torch.as_tensor(obs.astype(np.float64), dtype=DT), o.qs[a].n_s, o.qs[a].n_w).numpy()
    if q.shape[1] < 2:
        return np.full(len(q), np.inf)
    top = np.sort(q, 1)
    return top[:, -1] - top[:, -2]


def _rand_obs_decided(scn, E, rng, o):
    """_rand_obs with every row re-drawn until its agent's two best online values are at least GAP apart (float64): Double DQN's
    pick on such a row is the same in float32, so a* is compared on every row (the manner of _rand_obs_off_the_kinks)."""
    obs = _rand_obs(scn, E, rng)
    for a, n in enumerate(scn.n_s_ls):
        rows = np.arange(E)
        while rows.size:
            rows = rows[_online_gap(o, obs[rows, a, :n], a) < GAP]
            if rows.size:
                obs[rows, a, :n] = rng.rand(rows.size, n).astype(np.float32) * 2
    return obs


def _fill(models, o, scn, E, cap, rng, draw_next=None):
    """test_replay_minibatch_gradient_and_adam's transitions into every model's rings (and the oracle's): past the capacity."""
    A = scn.n_agent
    rn = models[0].cfg['reward_norm']
    n_add = cap + 7 if cap < 100 else 45
    draw = draw_next or (lambda: _rand_obs(scn, E, rng))
    obs = draw()
    for t in range(n_add):
        nobs = draw()
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, A) * 3.0 * rn
        done = (rng.rand(E) < 0.1).astype(np.uint8)
        for m in models:
            m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(),
                             torch.from_numpy(nobs).cuda(), torch.from_numpy(done).cuda())
        if o is not None:
            o.add_transition(obs, act, rew, nobs, done)
        obs = nobs
    return min(cap, n_add)


def _grads_at(m, idx_dev, lr=1e-3):
    from deeprl_signal_control_amd import _lib
    _lib.check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(idx_dev.data_ptr())))
    g = m.grad_tensor().cpu().numpy().copy()
    stats = np.zeros((m.n_agent, 2))
    _lib.check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(C.c_void_p)))
    return g, stats


def _set_target(m, period, double_q):
    from deeprl_signal_control_amd import _lib
    _lib.check(m._L.tsc_iql_set_target(m._h, period, double_q))


def _targets(m):
    from deeprl_signal_control_amd import _lib
    R = m.E * m.n_step
    y, astar = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.int32)
    _lib.check(m._L.tsc_iql_debug_targets(m._h, y.ctypes.data_as(C.c_void_p), astar.ctypes.data_as(C.c_void_p)))
    return y, astar


def _draw_idx(rng, E, A, B, size):
    return torch.from_numpy(np.stack([np.stack([rng.permutation(size)[:B] for _ in range(A)]) for _ in range(E)]).astype(np.int32)).cuda()


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_armed_with_target_equal_to_parameters_is_the_unarmed_step_bit_for_bit(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """theta- = theta: per row set the same MFMA sequence on the same operands, max is order-free and the value at the first argmax
    is the max -- gradient buffer and loss of one fixed draw are equal bit for bit, unarmed / target / target + double."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=100)
    _, m2 = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=100, double_q=1)
    assert m0.fused == m1.fused == m2.fused == (fused == '1')
    np.testing.assert_array_equal(m0.get_flat(), m1.get_flat())
    np.testing.assert_array_equal(m1.get_flat(), m1.get_target_flat())
    np.testing.assert_array_equal(m2.get_flat(), m2.get_target_flat())
    rng = np.random.RandomState(cap + E)
    size = _fill([m0, m1, m2], None, scn, E, cap, rng)
    idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    (g0, s0), (g1, s1), (g2, s2) = (_grads_at(m, idx) for m in (m0, m1, m2))
    assert np.abs(g0).max() > 0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(g2, g0)
    np.testing.assert_array_equal(s1[:, 0], s0[:, 0])
    np.testing.assert_array_equal(s2[:, 0], s0[:, 0])
    y1, a1 = _targets(m1)
    y2, a2 = _targets(m2)
    np.testing.assert_array_equal(y1, y2)
    assert (a1 == -1).all() and (a2 >= 0).all() and all((a2[a] < n).all() for a, n in enumerate(scn.n_a_ls))
    for m in (m0, m1, m2):
        m.close()


@pytest.mark.parametrize('double_q', [0, 1])
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, double_q, monkeypatch):
    """theta- != theta (two seeded initialisations): y and a* of every sampled row, loss, clip norm and every gradient tensor."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=100, double_q=double_q)
    assert m.fused == (fused == '1')
    o = _oracle(m, 100, bool(double_q))
    A, B = scn.n_agent, m.n_step
    rng = np.random.RandomState(cap + E + double_q)
    _fill([m], o, scn, E, cap, rng, draw_next=lambda: _rand_obs_decided(scn, E, rng, o))
    m.set_target_flat(m.layout.pack(_disagreeing_target(m, o)))
    o.set_target_params(m.layout.unpack(m.get_target_flat()))
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0.01
    params_before = [{k: v.clone() for k, v in q.p.items()} for q in o.qs]
    rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
    _lib.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = np.zeros((E, A, B), np.int32)
    _lib.check(m._L.tsc_iql_debug_batch(m._h, idx.ctypes.data_as(C.c_void_p)))
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    y, astar = _targets(m)
    stats = np.zeros((A, 2))
    _lib.check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3)
    np.testing.assert_array_equal(idx, o.last_idx)
    tol = 2e-5
    for a in range(A):
        q = o.qs[a]
        print('agent %d: max|dy| %.2e, smallest online gap %.2e' % (a, np.abs(y[a] - q.last_y).max(),
                                                                   _gap_of(q.last_q1_online)))
        assert _gap_of(q.last_q1_online) >= GAP, 'agent %d: a sampled row with undecided online argmax remains' % a
        np.testing.assert_allclose(y[a], q.last_y, rtol=0, atol=2e-5)
        if double_q:
            np.testing.assert_array_equal(astar[a], q.last_astar)
            differ = q.last_astar != np.argmax(q.last_q1_target, 1)
            assert differ.any(), 'agent %d: the online argmax is the target argmax on every sampled row' % a
        else:
            assert (astar[a] == -1).all()
        # ReLU kinks of this minibatch (the online net on s), as in test_replay_minibatch_gradient_and_adam
        saved, q.p = q.p, params_before[a]
        cols, deep = _kinks(o, [rows_before[a][e][s][0] for e in range(E) for s in idx[e, a]], a)
        q.p = saved
        for k, ref in og[a].items():
            if deep and k not in ('q_w', 'q_b'):
                continue
            got, scale = g[a][k], max(np.abs(ref).max(), 1e-9)
            err = np.abs(got - ref)
            if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                sel = cols[:m.layout.n_fc0] if k.startswith('fcw') else cols[m.layout.n_fc0:]
                err = err[..., ~sel] if err.ndim == 2 else err[~sel]
            assert err.size == 0 or err.max() <= tol * scale, 'agent %d %s: %.2e' % (a, k, err.max() / scale)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
    m.close()


def _disagreeing_target(m, o, seed=1234):
    """theta-: a second seeded initialisation, re-drawn per agent until its argmax differs from the online net's on a fifth of the
    next states in the agent's rings (an agent with two or three actions and a one-sided pair of nets would otherwise never
    exercise Double DQN); the test still asserts a disagreeing row among the SAMPLED ones."""
    from deeprl_signal_control_amd.iql import init_agent_params
    from oracle.iql_oracle import DT, q_net
    tp = init_agent_params(m.layout, np.random.RandomState(seed))
    for a, q in enumerate(o.qs):
        S1 = torch.as_tensor(np.asarray([t[3] for e in range(o.E) for t in o.rings[e][a].buffer]), dtype=DT)
        with torch.no_grad():
            on = q_net(q.p, S1, q.n_s, q.n_w).argmax(1)
            for trial in range(1, 40):
                cand = {k: torch.as_tensor(np.asarray(v), dtype=DT) for k, v in tp[a].items()}
                if (q_net(cand, S1, q.n_s, q.n_w).argmax(1) != on).double().mean() >= 0.2:
                    break
                tp[a] = init_agent_params(m.layout, np.random.RandomState(seed + trial))[a]
            else:
                pytest.fail('agent %d: no target initialisation disagrees with the online net' % a)
    return tp


def _gap_of(q):
    if q.shape[1] < 2:
        return np.inf
    top = np.sort(q, 1)
    return float((top[:, -1] - top[:, -2]).min())


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[1], CASES[3]])
def test_refresh_schedule(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """target_update = 2: theta- is the parameters as they stood after Adam steps 2 and 4 and does not move at steps 1, 3, 5."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=2, double_q=1)
    _fill([m], None, scn, E, cap, np.random.RandomState(3))
    p0 = m.get_flat()
    np.testing.assert_array_equal(m.get_target_flat(), p0)
    params, targets = [p0], [p0]
    for step in range(1, 6):
        m.minibatch_step(1e-3)
        params.append(m.get_flat()); targets.append(m.get_target_flat())
        assert m.get_opt_state()[2] == step                       # adam_t: one per Adam step, as before
        assert np.abs(params[step] - params[step - 1]).max() > 0
        np.testing.assert_array_equal(targets[step], params[step] if step % 2 == 0 else targets[step - 1])
    np.testing.assert_array_equal(targets[5], params[4])
    # set_flat does not touch theta-; sync_target does
    m.set_flat(p0)
    np.testing.assert_array_equal(m.get_target_flat(), params[4])
    m.sync_target()
    np.testing.assert_array_equal(m.get_target_flat(), p0)
    m.close()


def _target_launches():
    from deeprl_signal_control_amd import _lib
    ms, cnt = C.c_double(), C.c_int64()
    _lib.check(_lib.lib().tsc_profile_read(_lib.profile_names().index('iql_target'), C.byref(ms), C.byref(cnt)))
    return int(cnt.value)


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_default_path_is_untouched(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that was never armed and one that was armed and disarmed again: equal gradients and parameters over two steps, and
    no launch of the target kernel from either."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(11)
    size = _fill([m0, m1], None, scn, E, cap, rng)
    idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    _set_target(m1, 3, 1)
    ga, _ = _grads_at(m1, idx)                                     # one armed step in between, undone below
    m1.set_flat(m0.get_flat())
    z = np.zeros(m1.n_param, np.float32)
    _lib.check(m1._L.tsc_iql_set_opt_state(m1._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    _set_target(m1, 0, 0)
    with pytest.raises(RuntimeError, match='double_q'):
        _set_target(m1, 0, 1)
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
            (g0, s0), (g1, s1) = _grads_at(m0, idx), _grads_at(m1, idx)
            np.testing.assert_array_equal(g1, g0)
            np.testing.assert_array_equal(s1, s0)
            np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        assert _target_launches() == 0
        if m1.fused:                                               # (the counter does count: an armed fused step launches the kernel)
            _set_target(m1, 3, 0)
            _grads_at(m1, idx)
            assert _target_launches() == 1
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m0.close(); m1.close()


def test_checkpoint_round_trip(tmp_path):
    scn, m = _model('large_grid', 'iqld', 'dqn', 3, buffer_size=25, target_update=3, double_q=1)
    _fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(4):                                             # theta- = the parameters after step 3, one step behind
        m.minibatch_step(1e-3)
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0
    m.save(str(tmp_path / 'armed'), 7)
    z = np.load(str(tmp_path / 'armed' / 'checkpoint-7.npz'))
    np.testing.assert_array_equal(z['target'], m.get_target_flat())
    _, f = _model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, target_update=3, double_q=1)
    assert f.load(str(tmp_path / 'armed'))
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    np.testing.assert_array_equal(f.get_target_flat(), m.get_target_flat())
    for x, y_ in zip(f.get_opt_state(), m.get_opt_state()):
        np.testing.assert_array_equal(x, y_)
    assert (f.act_step, f.update_step) == (m.act_step, m.update_step) and f.get_opt_state()[2] == 4
    # an unarmed model: exactly the keys a checkpoint had before there was a target network; an armed model loads it with theta- = theta
    _, u = _model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
    u.save(str(tmp_path / 'plain'), 1)
    zu = np.load(str(tmp_path / 'plain' / 'checkpoint-1.npz'))
    assert sorted(zu.files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params']
    assert f.load(str(tmp_path / 'plain'))
    np.testing.assert_array_equal(f.get_flat(), u.get_flat())
    np.testing.assert_array_equal(f.get_target_flat(), u.get_flat())
    with pytest.raises(RuntimeError, match='target'):
        u.get_target_flat()
    # the other way round: an unarmed model takes an armed file's parameters and ignores its target
    assert u.load(str(tmp_path / 'armed'))
    np.testing.assert_array_equal(u.get_flat(), m.get_flat())
    for x in (m, f, u):
        x.close()


def test_double_q_without_a_target_network_is_refused():
    from deeprl_signal_control_amd.iql import IQL
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario('small_grid', 'iqld')
    with pytest.raises(ValueError, match='double_q'):
        _model('small_grid', 'iqld', 'dqn', 2, double_q=1)
    # the E = 1 adaptor arms its handle from the config too
    one = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20, buffer_size=40, reward_norm=100.0, target_update=4), seed=1)
    np.testing.assert_array_equal(one.get_target_flat(), one.vec.get_flat())
    one.set_target_flat(one.get_target_flat() * 2)
    assert np.abs(one.get_target_flat() - one.vec.get_flat()).max() > 0
    one.sync_target()
    np.testing.assert_array_equal(one.get_target_flat(), one.vec.get_flat())
    one.vec.close()


INI = """
[MODEL_CONFIG]
max_grad_norm = 40
gamma = 0.99
lr_init = 1e-4
lr_decay = constant
epsilon_init = 1.0
epsilon_min = 0.01
epsilon_decay = linear
epsilon_ratio = 0.5
num_fc = 128
num_h = 64
batch_size = 20
buffer_size = 1000
reward_norm = 100.0
reward_clip = 2.0
target_update = 5
double_q = 1

[TRAIN_CONFIG]
total_step = 120
test_interval = 60
log_interval = 60

[ENV_CONFIG]
clip_wave = 2.0
clip_wait = 2.0
control_interval_sec = 5
agent = iqld
coop_gamma = 0.9
data_path = ./small_grid/data/
episode_length_sec = 300
norm_wave = 5.0
norm_wait = 100.0
coef_wait = 0.2
num_extra_car_per_hour = 1000
objective = hybrid
scenario = small_grid
seed = 12
test_seeds = 10000,20000
yellow_interval_sec = 2
"""


def test_train_then_evaluate_with_target_network(tmp_path):
    """`train` with target_update / double_q in the INI needs nothing else: it runs, its checkpoint carries theta-, `evaluate` loads it."""
    from deeprl_signal_control_amd import main as cli
    cfg = tmp_path / 'config_iqld.ini'
    cfg.write_text(INI)
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/iqld', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', '4'])
    assert len(rows) > 0
    ck = base + '/iqld/model/checkpoint-120.npz'
    assert os.path.exists(ck)
    z = np.load(ck)
    assert 'target' in z.files and z['target'].shape == z['params'].shape
    t = int(z['counters'][0])
    assert t > 0 and (np.array_equal(z['target'], z['params']) == (t % 5 == 0))
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'iqld', '--evaluation-seeds', '10000'])
    mean, std = out['iqld']
    assert mean.shape == (1,) and mean[0] < 0
