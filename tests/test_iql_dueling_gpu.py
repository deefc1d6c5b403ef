"""GPU tests of the opt-in dueling head of the IQL-DNN learner ([MODEL_CONFIG] dueling; include/tsc.h tsc_iql_set_dueling; csrc/tsc_iql_fused.h
q_duel and the QDuel instantiations of the act, target and gradient kernels; csrc/tsc_iql.hip iql_duel_combine_kernel and iql_td_duel_kernel
on the grouped-GEMM path) against the float64 restatement of tests/iql_ext_oracle.py.

Shapes: the dqn rows of tests/test_iql_target_gpu.py::CASES, the smallest at which each path can go wrong -- large_grid E = 70 (width-10
instantiation, several row splits, ragged last chunk 1400 = 21 x 64 + 56), E = 3 (one partial chunk), E = 6 on the grouped-GEMM path,
small_grid (width 8, no wait tile), real_net (n_a from 2 to 6 in one handle: per-agent 1 / n_a, V in a lane group that holds no action).

Tolerances are the project's (tests/test_iql_gpu.py): Q values and y |d| <= 2e-5; gradients |d| <= 2e-5 max|g| per tensor with hidden units
within 1e-6 of a ReLU kink excepted; loss and clip norm rtol 1e-4; a* and greedy actions exact (rows whose two best combined online values
lie within 1e-4 of each other in float64 are re-drawn before they are used, and none may remain)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_iql_gpu import _kinks, _rand_obs
from tests.test_iql_per_gpu import _batch, _expected_after, _launches, _per_debug, _random_priorities, _set_beta, _set_per
from tests.test_iql_target_gpu import CASES as TARGET_CASES
from tests.test_iql_target_gpu import GAP, _disagreeing_target, _draw_idx, _fill, _gap_of, _grads_at, _model, _set_target, _targets

pytestmark = pytest.mark.gpu

CASES = [c for c in TARGET_CASES if c[2] == 'dqn']
TARGETS = [(0, 0), (100, 0), (100, 1)]
N_UPDATE = 10


def _check(rc):
    from deeprl_signal_control_amd import _lib
    _lib.check(rc)


def _set_dueling(m, enable):
    _check(m._L.tsc_iql_set_dueling(m._h, enable))


def _get_dueling(m):
    v = C.c_int32(-1)
    _check(m._L.tsc_iql_get_dueling(m._h, C.byref(v)))
    return int(v.value)


def _nontrivial(agents, rng):
    """Biases of both streams away from their zero initialisation (the weights are orthogonal draws already)."""
    for p in agents:
        p['q_b'] = (rng.randn(*p['q_b'].shape) * 0.3).astype(np.float32)
        p['v_b'] = (rng.randn(1) * 0.3 + 0.5).astype(np.float32)
    return agents


def _duel_model(scenario, E, cap, seed=5, **cfg):
    scn, m = _model(scenario, 'iqld', 'dqn', E, seed=seed, buffer_size=cap, dueling=1, **cfg)
    assert _get_dueling(m) == 1 and m.layout.dueling
    m.set_agent_params(_nontrivial(m.get_agent_params(), np.random.RandomState(seed + 100)))
    if m.target_update:
        m.sync_target()
    p = m.get_agent_params()
    assert all(np.abs(x['v_w']).max() > 0 and x['v_b'][0] != 0 and np.abs(x['q_b']).min() > 0 for x in p)
    return scn, m


def _oracle(m, per=False):
    from tests.iql_ext_oracle import ExtOracleIQL
    return ExtOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, per=per, alpha=m.per_alpha, eps=m.per_eps,
                         target_update=m.target_update, double_q=bool(m.double_q), batch_size=m.n_step,
                         buffer_size=int(m.cfg['buffer_size']), gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'],
                         reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'], replay_seed=m.replay_seed)


def _rand_obs_decided(scn, E, rng, o):
    """tests/test_iql_target_gpu.py's _rand_obs_decided with the dueling net: every row re-drawn until its agent's two best COMBINED online
    values are at least GAP apart in float64, so the greedy action and Double DQN's pick are the same in float32."""
    from oracle.iql_oracle import DT
    from tests.iql_ext_oracle import q_net_duel
    obs = _rand_obs(scn, E, rng)
    for a, n in enumerate(scn.n_s_ls):
        rows = np.arange(E)
        while rows.size:
            with torch.no_grad():
                q = q_net_duel(o.qs[a].p, torch.as_tensor(obs[rows, a, :n].astype(np.float64), dtype=DT), o.qs[a].n_s, o.qs[a].n_w).numpy()
            top = np.sort(q, 1)
            rows = rows[top[:, -1] - top[:, -2] < GAP]
            if rows.size:
                obs[rows, a, :n] = rng.rand(rows.size, n).astype(np.float32) * 2
    return obs


def _compare_grads(m, o, g, og, idx, params_before, rows_before, what=''):
    """tests/test_iql_gpu.py's gradient comparison, every tensor of every agent (v_w / v_b included) -> agents that met a ReLU kink."""
    tol, kinked = 2e-5, set()
    for a in range(m.n_agent):
        q = o.qs[a]
        saved, q.p = q.p, params_before[a]
        cols, deep = _kinks(o, [rows_before[a][e][s][0] for e in range(m.E) for s in idx[e, a]], a)
        q.p = saved
        if deep or cols.any():
            kinked.add(a)
        assert set(og[a]) == set(g[a]) and 'v_w' in og[a] and 'v_b' in og[a]
        for k, ref in og[a].items():
            if deep and k not in ('q_w', 'q_b', 'v_w', 'v_b'):
                continue
            got, scale = g[a][k], max(np.abs(ref).max(), 1e-9)
            err = np.abs(got - ref)
            if k.startswith(('fcw', 'fct')) and cols.any():
                sel = cols[:m.layout.n_fc0] if k.startswith('fcw') else cols[m.layout.n_fc0:]
                err = err[..., ~sel] if err.ndim == 2 else err[~sel]
            assert err.size == 0 or err.max() <= tol * scale, '%s agent %d %s: %.2e' % (what, a, k, err.max() / scale)
    return kinked


def _dead_columns_are_zero(m, flat_g):
    """columns n_a <= j < 7 of dWq and dbq: exactly 0."""
    lay = m.layout
    f = flat_g.reshape(lay.A, lay.stride)
    for a, na in enumerate(m.n_a_ls):
        Wq = f[a, lay.oWq:lay.obq].reshape(lay.H2, 8)
        assert (Wq[:, na:7] == 0).all() and (f[a, lay.obq + na:lay.obq + 7] == 0).all(), a
        assert np.abs(Wq[:, 7]).max() > 0 and f[a, lay.obq + 7] != 0 and np.abs(Wq[:, :na]).max() > 0


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
def _forward_vs_oracle(scn, m, o, E, rng):
    from oracle.iql_oracle import act_epsilon_greedy
    from oracle.nets_oracle import sample_uniform
    A = scn.n_agent
    for t in range(2):
        obs = _rand_obs_decided(scn, E, rng, o)
        act, q = m.forward(torch.from_numpy(obs).cuda())
        act, q = act.cpu().numpy(), q.cpu().numpy()
        oq = o.forward(obs)
        worst = 0.0
        for a in range(A):
            na = scn.n_a_ls[a]
            worst = max(worst, np.abs(q[:, a, :na] - oq[a]).max())
            np.testing.assert_allclose(q[:, a, :na], oq[a], rtol=0, atol=2e-5)
            assert np.all(q[:, a, na:] == 0)
            np.testing.assert_array_equal(act[:, a], np.argmax(q[:, a, :na], 1))
            assert _gap_of(oq[a]) >= GAP
            np.testing.assert_array_equal(act[:, a], np.argmax(oq[a], 1))
        print('max |dQ| %.2e' % worst)
        eps_before = m.eps_scheduler.n
        act, q = m.forward(torch.from_numpy(obs).cuda(), mode='explore')
        eps = max(m.cfg['epsilon_min'], m.cfg['epsilon_init'] * (1 - (eps_before + 1) / (10000 * m.cfg['epsilon_ratio'])))
        act, q = act.cpu().numpy(), q.cpu().numpy()
        for e in range(E):
            for a in range(A):
                u0 = sample_uniform(m.sample_seed, m.act_step - 1, 2 * (e * A + a))
                u1 = sample_uniform(m.sample_seed, m.act_step - 1, 2 * (e * A + a) + 1)
                assert act[e, a] == act_epsilon_greedy(q[e, a, :scn.n_a_ls[a]], eps, u0, u1)


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_forward_against_the_oracle(scenario, agent, model_type, E, cap, fused, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _duel_model(scenario, E, cap, seed=3)
    assert m.fused == (fused == '1')
    _forward_vs_oracle(scn, m, _oracle(m), E, np.random.RandomState(E))
    m.close()


# ---- 2. targets and gradient -----------------------------------------------------------------------------------------------------
def _arm_disagreeing_target(m, o):
    # (_disagreeing_target compares the argmax of the advantage streams, which is the argmax of the combined values: V and the mean are
    # common to a row's actions; so theta- keeps the advantage biases it was chosen with and only its value bias leaves zero)
    tp, rng = _disagreeing_target(m, o), np.random.RandomState(77)
    for p in tp:
        p['v_b'] = (rng.randn(1) * 0.3 - 0.4).astype(np.float32)
    m.set_target_flat(m.layout.pack(tp))
    o.set_target_params(m.layout.unpack(m.get_target_flat()))
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0.01


def _targets_and_gradient_vs_oracle(scn, m, o, E, cap, rng, target_update, double_q):
    """-> the flat gradient buffer of the step (the caller may look at single columns)."""
    A, B = scn.n_agent, m.n_step
    _fill([m], o, scn, E, cap, rng, draw_next=lambda: _rand_obs_decided(scn, E, rng, o))
    if target_update:
        _arm_disagreeing_target(m, o)
    params_before = [{k: v.clone() for k, v in q.p.items()} for q in o.qs]
    rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
    _check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = _batch(m)
    flat_g = m.grad_tensor().cpu().numpy().copy()
    g = m.layout.unpack(flat_g)
    y, astar = _targets(m)                                        # (answers on a dueling handle without a target network too)
    stats = np.zeros((A, 2))
    _check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3)
    np.testing.assert_array_equal(idx, o.last_idx)
    for a in range(A):
        q = o.qs[a]
        print('agent %d: max|dy| %.2e, smallest online gap %.2e' % (a, np.abs(y[a] - q.last_y).max(), _gap_of(q.last_q1_online)))
        assert _gap_of(q.last_q1_online) >= GAP, 'agent %d: a sampled row with undecided online argmax remains' % a
        np.testing.assert_allclose(y[a], q.last_y, rtol=0, atol=2e-5)
        if double_q:
            np.testing.assert_array_equal(astar[a], q.last_astar)
            assert (q.last_astar != np.argmax(q.last_q1_target, 1)).any(), 'agent %d: the online argmax is the target argmax on every sampled row' % a
        else:
            assert (astar[a] == -1).all()
    _compare_grads(m, o, g, og, idx, params_before, rows_before)
    _dead_columns_are_zero(m, flat_g)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
    return flat_g


@pytest.mark.parametrize('target_update,double_q', TARGETS)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, target_update, double_q, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    assert m.fused == (fused == '1')
    _targets_and_gradient_vs_oracle(scn, m, _oracle(m), E, cap, np.random.RandomState(cap + E + double_q + target_update), target_update, double_q)
    m.close()


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[4], CASES[2]])
def test_prioritized_dueling_step_against_the_oracle(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """The full 3DQN step (dueling + Double DQN + prioritized replay): weights, |delta| written back, new priorities, loss, gradient."""
    from tests.iql_ext_oracle import per_weights
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    beta = 0.4
    scn, m = _duel_model(scenario, E, cap, target_update=100, double_q=1, prioritized_replay=1)
    assert m.fused == (fused == '1')
    o = _oracle(m, per=True)
    A, B = scn.n_agent, m.n_step
    rng = np.random.RandomState(cap + E)
    size = _fill([m], o, scn, E, cap, rng, draw_next=lambda: _rand_obs_decided(scn, E, rng, o))
    _arm_disagreeing_target(m, o)
    q = _random_priorities(m, size, rng)
    before, qmax_before = m.get_priorities()
    o.prio[:], o.qmax[:] = q, qmax_before
    _set_beta(m, beta)
    params_before = [{k: v.clone() for k, v in x.p.items()} for x in o.qs]
    rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
    _check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = _batch(m)
    flat_g = m.grad_tensor().cpu().numpy().copy()
    g = m.layout.unpack(flat_g)
    w, td = _per_debug(m)
    y, astar = _targets(m)
    stats = np.zeros((A, 2))
    _check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3, beta=beta, idx_given=idx)
    wr = w.reshape(A, E, B)
    assert (wr.max(2) == 1).all() and (w > 0).all() and w.min() < 0.5
    for e in range(E):
        for a in range(A):
            np.testing.assert_allclose(wr[a, e], per_weights(q[e, a], size, idx[e, a], beta), rtol=1e-6, atol=0)
    np.testing.assert_allclose(w, o.last_w, rtol=1e-6, atol=0)
    print('max |d|delta|| %.2e' % np.abs(td - o.last_td).max())
    np.testing.assert_allclose(td, o.last_td, rtol=0, atol=2e-5)
    for a in range(A):
        np.testing.assert_allclose(y[a], o.qs[a].last_y, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(astar[a], o.qs[a].last_astar)
    after, qmax = m.get_priorities()
    want, wmax, hit = _expected_after(before, qmax_before, idx, td, size, m.per_alpha, m.per_eps)
    np.testing.assert_allclose(after[hit], want[hit], rtol=1e-6, atol=0)
    np.testing.assert_array_equal(after[~hit], before[~hit])
    np.testing.assert_allclose(qmax, wmax, rtol=1e-6, atol=0)
    _compare_grads(m, o, g, og, idx, params_before, rows_before)
    _dead_columns_are_zero(m, flat_g)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
    m.close()


# ---- 3. Adam steps ---------------------------------------------------------------------------------------------------------------
def _adam_step_bound(t, lr, b1=0.9, b2=0.999):
    """The largest move Adam's step t can make on one weight.  With m_t = (1 - b1) sum_k b1^k g_{t-k} and v_t = (1 - b2) sum_k b2^k g_{t-k}^2
    (k < t), Cauchy-Schwarz gives |m_t| / sqrt(v_t) <= (1 - b1) / sqrt(1 - b2) sqrt(sum_{k < t} (b1^2 / b2)^k), and the step is
    lr sqrt(1 - b2^t) / (1 - b1^t) times that: exactly lr at t = 1 (the bound tests/test_iql_gpu.py uses for its first three steps, where it is
    at most 1.004 lr), 1.043 lr at t = 10."""
    s = sum((b1 * b1 / b2) ** k for k in range(t))
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) * (1.0 - b1) / np.sqrt(1.0 - b2) * np.sqrt(s)


def test_adam_steps_against_the_oracle():
    """N_UPDATE minibatch steps on the 70-instance case, each by tests/test_iql_gpu.py's rule for Adam: entries whose gradient is well
    above the gradient tolerance move alike to 2e-6, every entry by at most Adam's bound for that step, and every step is checked from the same state (the oracle
    takes the device's parameters and moments after each one)."""
    scenario, agent, model_type, E, cap, fused = CASES[0]
    scn, m = _duel_model(scenario, E, cap)
    assert m.fused
    o = _oracle(m)
    A, lr = scn.n_agent, 1e-3
    rng = np.random.RandomState(cap + E)
    _fill([m], o, scn, E, cap, rng)
    for step in range(N_UPDATE):
        before = m.get_flat().reshape(A, -1).copy()
        _check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
        m.update_step += 1
        idx = _batch(m)
        flat_g = m.grad_tensor().cpu().numpy().reshape(A, -1).copy()
        g = m.layout.unpack(flat_g)
        _check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, None))
        obefore = m.layout.pack(o.agent_params()).reshape(A, -1)
        rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
        params_before = [{k: v.clone() for k, v in q.p.items()} for q in o.qs]
        losses, norms, og = o.minibatch_step(lr)
        np.testing.assert_array_equal(idx, o.last_idx)
        kinked = _compare_grads(m, o, g, og, idx, params_before, rows_before, 'step %d' % step)
        after = m.get_flat().reshape(A, -1)
        oflat = m.layout.pack(o.agent_params()).reshape(A, -1)
        d_hip, d_orc = after - before, oflat - obefore
        real = np.abs(flat_g) > 1e-2 * np.abs(flat_g).max(1, keepdims=True)
        real[sorted(kinked)] = False
        assert step > 0 or real.any()
        if real.any():
            assert np.abs(d_hip - d_orc)[real].max() <= 2e-6, (step, np.abs(d_hip - d_orc)[real].max())
        bound = 1.01 * _adam_step_bound(step + 1, lr)                            # (1 %: float32 rounding, as in tests/test_iql_gpu.py)
        assert np.abs(d_hip).max() <= bound and np.abs(d_hip - d_orc).max() <= 2 * bound, (step, np.abs(d_hip).max(), bound)
        if step == 0:
            assert np.array_equal(after == before, flat_g == 0)                  # structural zeros and the dead head columns never move
        hm, hv, ht = m.get_opt_state()
        assert ht == step + 1 == o.qs[0].t
        for a, (pp, mm, vv) in enumerate(zip(m.get_agent_params(), m.layout.unpack(hm), m.layout.unpack(hv))):
            for k in o.qs[a].p:
                o.qs[a].p[k] = torch.as_tensor(pp[k].astype(np.float64))
                o.qs[a].m[k] = torch.as_tensor(mm[k].astype(np.float64))
                o.qs[a].v[k] = torch.as_tensor(vv[k].astype(np.float64))
    m.close()


# ---- 4. the two paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update,double_q', [(0, 0), (100, 1)])
def test_fused_and_grouped_paths_agree(target_update, double_q, monkeypatch):
    scenario, E, cap = 'large_grid', 6, 30
    monkeypatch.setenv('TSC_IQL_FUSED', '1')
    scn, mf = _duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    monkeypatch.setenv('TSC_IQL_FUSED', '0')
    _, mg = _duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    assert mf.fused and not mg.fused
    np.testing.assert_array_equal(mf.get_flat(), mg.get_flat())
    rng = np.random.RandomState(9)
    size = _fill([mf, mg], None, scn, E, cap, rng)
    if target_update:
        tp = mf.layout.pack(_nontrivial(mf.layout.unpack(np.random.RandomState(1).randn(mf.n_param).astype(np.float32) * 0.1 + mf.get_flat()),
                                        np.random.RandomState(2)))
        mf.set_target_flat(tp); mg.set_target_flat(tp)
    idx = _draw_idx(rng, E, scn.n_agent, mf.n_step, size)
    (gf, sf), (gg, sg) = _grads_at(mf, idx), _grads_at(mg, idx)
    uf, ug = mf.layout.unpack(gf), mg.layout.unpack(gg)
    for a in range(scn.n_agent):
        for k in uf[a]:
            scale = max(np.abs(uf[a][k]).max(), np.abs(ug[a][k]).max(), 1e-9)
            assert np.abs(uf[a][k] - ug[a][k]).max() <= 2e-5 * scale, (a, k)
    _dead_columns_are_zero(mf, gf); _dead_columns_are_zero(mg, gg)
    np.testing.assert_allclose(sf[:, 0], sg[:, 0], rtol=1e-4)
    np.testing.assert_allclose(sf[:, 1], sg[:, 1], rtol=1e-4)
    yf, yg = _targets(mf)[0], _targets(mg)[0]
    np.testing.assert_allclose(yf, yg, rtol=0, atol=2e-5)
    mf.close(); mg.close()


# ---- 5. disarm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_disarm_restores_the_default_step_bit_for_bit(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that was armed, given a non-zero V column, stepped and disarmed, and a never-armed handle with the same parameters (V column
    kept: the default kernels ignore it): one fixed draw through tsc_iql_compute_grads_at, gradient buffers and losses equal."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m1 = _duel_model(scenario, E, cap)
    _, m0 = _model(scenario, agent, model_type, E, buffer_size=cap)
    assert m0.fused == m1.fused == (fused == '1') and _get_dueling(m0) == 0
    rng = np.random.RandomState(11)
    size = _fill([m0, m1], None, scn, E, cap, rng)
    idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    p = m1.get_flat()
    f = p.reshape(m1.n_agent, -1)
    assert np.abs(f[:, m1.layout.obq + 7]).min() > 0
    ga, _ = _grads_at(m1, idx)                                     # one armed step in between, undone below
    m1.set_flat(p); m0.set_flat(p)
    z = np.zeros(m1.n_param, np.float32)
    for m in (m0, m1):
        _check(m._L.tsc_iql_set_opt_state(m._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    _set_dueling(m1, 0)
    assert _get_dueling(m1) == 0
    with pytest.raises(RuntimeError, match='tsc_iql_debug_targets'):
        _targets(m1)
    (g0, s0), (g1, s1) = _grads_at(m0, idx), _grads_at(m1, idx)
    assert np.abs(g0).max() > 0 and np.abs(ga - g0).max() > 0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
    lay = m0.layout
    assert (g0.reshape(lay.A, lay.stride)[:, lay.obq + 7] == 0).all()           # the default step leaves the V column without a gradient
    act0, q0 = m0.forward(torch.from_numpy(_rand_obs(scn, E, np.random.RandomState(1))).cuda())
    act1, q1 = m1.forward(torch.from_numpy(_rand_obs(scn, E, np.random.RandomState(1))).cuda())
    np.testing.assert_array_equal(q1.cpu().numpy(), q0.cpu().numpy())
    np.testing.assert_array_equal(act1.cpu().numpy(), act0.cpu().numpy())
    m0.close(); m1.close()


# ---- 6. routes -------------------------------------------------------------------------------------------------------------------
KERNELS = ('iql_sample', 'iql_per_sample', 'iql_target', 'iql_grad', 'iql_reduce', 'iql_per_update', 'iql_per_add')


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[1], CASES[3], CASES[2]])
def test_routes(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A dueling step on the fused path: one iql_target, one iql_grad, one iql_reduce, with or without a target network; on the grouped path
    none of the three; after disarming the unarmed counts."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _duel_model(scenario, E, cap)
    on = m.fused
    assert on == (fused == '1')
    _fill([m], None, scn, E, cap, np.random.RandomState(E + cap))
    _lib.profile(enable=True)
    try:
        for duel, period, double_q, fused_counts in [(1, 0, 0, [1, 0, 1, 1, 1, 0, 0]), (1, 100, 0, [1, 0, 1, 1, 1, 0, 0]),
                                                     (1, 100, 1, [1, 0, 1, 1, 1, 0, 0]), (0, 0, 0, [1, 0, 0, 1, 1, 0, 0])]:
            _set_dueling(m, duel)
            _set_target(m, period, double_q)
            _lib.profile(reset=True)
            stats = m.minibatch_step(1e-3, want_stats=True)
            got = [_launches(k) for k in KERNELS]
            want = [c if on or k not in ('iql_target', 'iql_grad', 'iql_reduce') else 0 for k, c in zip(KERNELS, fused_counts)]
            print((duel, period, double_q), dict(zip(KERNELS, got)))
            assert got == want, (duel, period, double_q)
            assert np.isfinite(stats).all() and (stats[:, 1] > 0).all()
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from deeprl_signal_control_amd.iql import VecIQL
    scn, lr = _model('large_grid', 'iqll', 'lr', 2, buffer_size=30)
    with pytest.raises(RuntimeError, match='tsc_iql_set_dueling'):
        _set_dueling(lr, 1)
    assert _get_dueling(lr) == 0
    with pytest.raises(RuntimeError, match='tsc_iql_set_dueling'):
        _check(lr._L.tsc_iql_set_dueling(lr._h, 2))
    lr.close()
    with pytest.raises(ValueError, match='dueling'):
        _model('large_grid', 'iqll', 'lr', 2, buffer_size=30, dueling=1)
    # a synthetic handle with an agent of eight actions: refused, never clamped; seven are fine
    n_s, n_w = [12, 12, 12], [4, 4, 4]
    cfg = dict(batch_size=20, buffer_size=30, reward_norm=100.0)
    wide = VecIQL(n_s, [3, 8, 5], n_w, 2, 12, 8, cfg, total_step=100, seed=1, model_type='dqn')
    with pytest.raises(RuntimeError, match='8 actions'):
        _set_dueling(wide, 1)
    assert _get_dueling(wide) == 0
    wide.close()
    with pytest.raises((RuntimeError, ValueError), match='actions'):
        VecIQL(n_s, [3, 8, 5], n_w, 2, 12, 8, dict(cfg, dueling=1), total_step=100, seed=1, model_type='dqn')
    seven = VecIQL(n_s, [3, 7, 5], n_w, 2, 12, 7, dict(cfg, dueling=1), total_step=100, seed=1, model_type='dqn')
    assert _get_dueling(seven) == 1
    obs = torch.rand(2, 3, 12, device='cuda')
    act, q = seven.forward(obs)
    assert q.shape == (2, 3, 7) and (q[:, 0, 3:] == 0).all() and (q[:, 1] != 0).all() and (act[:, 1] == q[:, 1].argmax(1)).all()
    seven.close()


# ---- 8. checkpoint ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    scn, m = _duel_model('large_grid', 3, 25)
    _fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(2):
        m.minibatch_step(1e-3)
    m.save(str(tmp_path / 'duel'), 7)
    z = np.load(str(tmp_path / 'duel' / 'checkpoint-7.npz'))
    assert sorted(z.files) == ['adam_m', 'adam_v', 'counters', 'dueling', 'format', 'layout', 'params'] and int(z['dueling']) == 1
    _, f = _model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, dueling=1)
    assert f.load(str(tmp_path / 'duel'))
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    for a, b in zip(f.get_agent_params(), m.get_agent_params()):
        np.testing.assert_array_equal(a['v_w'], b['v_w'])
        np.testing.assert_array_equal(a['v_b'], b['v_b'])
        assert np.abs(b['v_w']).max() > 0 and b['v_b'][0] != 0
    for x, y_ in zip(f.get_opt_state(), m.get_opt_state()):
        np.testing.assert_array_equal(x, y_)
    # an unarmed model's file keeps exactly its keys; neither kind of model loads the other's file
    _, u = _model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
    u.save(str(tmp_path / 'plain'), 1)
    assert sorted(np.load(str(tmp_path / 'plain' / 'checkpoint-1.npz')).files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params']
    before = u.get_flat()
    with pytest.raises(ValueError, match='dueling'):
        u.load(str(tmp_path / 'duel'))
    np.testing.assert_array_equal(u.get_flat(), before)
    with pytest.raises(ValueError, match='dueling'):
        f.load(str(tmp_path / 'plain'))
    for x in (m, f, u):
        x.close()
