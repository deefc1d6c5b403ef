"""GPU tests of the opt-in dueling head of the IQL-DNN learner ([MODEL_CONFIG] dueling; include/tsc.h tsc_iql_set_dueling; csrc/tsc_iql_fused.h
q_duel and the QDuel instantiations of the act, target and gradient kernels; csrc/tsc_iql.hip iql_duel_combine_kernel and iql_td_kernel's dense
dQ row on the grouped-GEMM path) against the float64 restatement of tests/iql_ext_oracle.py.

Shapes: the dqn rows of tests/iql_harness.py::CASES, the smallest at which each path can go wrong -- large_grid E = 70 (width-10
instantiation, several row splits, ragged last chunk 1400 = 21 x 64 + 56), E = 3 (one partial chunk), E = 6 on the grouped-GEMM path,
small_grid (width 8, no wait tile), real_net (n_a from 2 to 6 in one handle: per-agent 1 / n_a, V in a lane group that holds no action).

Tolerances are the project's (tests/test_iql_gpu.py): Q values and y |d| <= 2e-5; gradients |d| <= 2e-5 max|g| per tensor with hidden units
within 1e-6 of a ReLU kink excepted; loss and clip norm rtol 1e-4; a* and greedy actions exact (rows whose two best combined online values
lie within 1e-4 of each other in float64 are re-drawn before they are used, and none may remain)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import iql_harness as H

pytestmark = pytest.mark.gpu

CASES = [c for c in H.CASES if c[2] == 'dqn']
TARGETS = [(0, 0), (100, 0), (100, 1)]
N_UPDATE = 10


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_forward_against_the_oracle(scenario, agent, model_type, E, cap, fused, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.duel_model(scenario, E, cap, seed=3)
    assert m.fused == (fused == '1')
    H.duel_forward_vs_oracle(scn, m, H.oracle_for(m), E, np.random.RandomState(E))
    m.close()


# ---- 2. targets and gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update,double_q', TARGETS)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, target_update, double_q, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    assert m.fused == (fused == '1')
    H.targets_and_gradient_vs_oracle(scn, m, H.oracle_for(m), E, cap, np.random.RandomState(cap + E + double_q + target_update))
    m.close()


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[4], CASES[2]])
def test_prioritized_dueling_step_against_the_oracle(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """The full 3DQN step (dueling + Double DQN + prioritized replay): weights, |delta| written back, new priorities, loss, gradient."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    beta = 0.4
    scn, m = H.duel_model(scenario, E, cap, target_update=100, double_q=1, prioritized_replay=1)
    assert m.fused == (fused == '1')
    o = H.oracle_for(m)
    A, B = scn.n_agent, m.n_step
    rng = np.random.RandomState(cap + E)
    size = H.fill([m], o, scn, E, cap, rng, draw_next=lambda: H.rand_obs_decided(scn, E, rng, o))[0]
    H.arm_disagreeing_target(m, o)
    q = H.random_priorities(m, size, rng)
    before, qmax_before = m.get_priorities()
    o.prio[:], o.qmax[:] = q, qmax_before
    H.set_beta(m, beta)
    params_before, rows_before = H.snapshot(o)
    H.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = H.batch(m)
    flat_g = m.grad_tensor().cpu().numpy().copy()
    g = m.layout.unpack(flat_g)
    w, td = H.per_debug(m)
    y, astar = H.targets(m)
    stats = np.zeros((A, 2))
    H.check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3, beta=beta, idx_given=idx)
    H.check_weights(w, td, o, q, size, idx, beta)
    for a in range(A):
        np.testing.assert_allclose(y[a], o.qs[a].last_y, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(astar[a], o.qs[a].last_astar)
    H.check_write_back(m, before, qmax_before, idx, td, size)
    H.compare_grads(m, o, g, og, idx, params_before, rows_before)
    H.dead_columns_are_zero(m, flat_g)
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
    scn, m = H.duel_model(scenario, E, cap)
    assert m.fused
    o = H.oracle_for(m)
    A, lr = scn.n_agent, 1e-3
    rng = np.random.RandomState(cap + E)
    H.fill([m], o, scn, E, cap, rng)
    for step in range(N_UPDATE):
        before = m.get_flat().reshape(A, -1).copy()
        H.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
        m.update_step += 1
        idx = H.batch(m)
        flat_g = m.grad_tensor().cpu().numpy().reshape(A, -1).copy()
        g = m.layout.unpack(flat_g)
        H.check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, None))
        obefore = m.layout.pack(o.agent_params()).reshape(A, -1)
        params_before, rows_before = H.snapshot(o)
        losses, norms, og = o.minibatch_step(lr)
        np.testing.assert_array_equal(idx, o.last_idx)
        kinked = H.compare_grads(m, o, g, og, idx, params_before, rows_before, 'step %d' % step)
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
        assert H.sync_oracle(m, o) == step + 1 == o.qs[0].t
    m.close()


# ---- 4. the two paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update,double_q', [(0, 0), (100, 1)])
def test_fused_and_grouped_paths_agree(target_update, double_q, monkeypatch):
    scenario, E, cap = 'large_grid', 6, 30
    monkeypatch.setenv('TSC_IQL_FUSED', '1')
    scn, mf = H.duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    monkeypatch.setenv('TSC_IQL_FUSED', '0')
    _, mg = H.duel_model(scenario, E, cap, target_update=target_update, double_q=double_q)
    assert mf.fused and not mg.fused
    np.testing.assert_array_equal(mf.get_flat(), mg.get_flat())
    rng = np.random.RandomState(9)
    size = H.fill([mf, mg], None, scn, E, cap, rng)[0]
    if target_update:
        tp = mf.layout.pack(H.nontrivial(mf.layout.unpack(np.random.RandomState(1).randn(mf.n_param).astype(np.float32) * 0.1 + mf.get_flat()),
                                        np.random.RandomState(2)))
        mf.set_target_flat(tp); mg.set_target_flat(tp)
    idx = H.draw_idx(rng, E, scn.n_agent, mf.n_step, size)
    (gf, sf), (gg, sg) = H.grads_at(mf, idx), H.grads_at(mg, idx)
    uf, ug = mf.layout.unpack(gf), mg.layout.unpack(gg)
    for a in range(scn.n_agent):
        for k in uf[a]:
            scale = max(np.abs(uf[a][k]).max(), np.abs(ug[a][k]).max(), 1e-9)
            assert np.abs(uf[a][k] - ug[a][k]).max() <= 2e-5 * scale, (a, k)
    H.dead_columns_are_zero(mf, gf); H.dead_columns_are_zero(mg, gg)
    np.testing.assert_allclose(sf[:, 0], sg[:, 0], rtol=1e-4)
    np.testing.assert_allclose(sf[:, 1], sg[:, 1], rtol=1e-4)
    yf, yg = H.targets(mf)[0], H.targets(mg)[0]
    np.testing.assert_allclose(yf, yg, rtol=0, atol=2e-5)
    mf.close(); mg.close()


# ---- 5. disarm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_disarm_restores_the_default_step_bit_for_bit(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that was armed, given a non-zero V column, stepped and disarmed, and a never-armed handle with the same parameters (V column
    kept: the default kernels ignore it): one fixed draw through tsc_iql_compute_grads_at, gradient buffers and losses equal."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m1 = H.duel_model(scenario, E, cap)
    _, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    assert m0.fused == m1.fused == (fused == '1') and H.get_dueling(m0) == 0
    rng = np.random.RandomState(11)
    size = H.fill([m0, m1], None, scn, E, cap, rng)[0]
    idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    p = m1.get_flat()
    f = p.reshape(m1.n_agent, -1)
    assert np.abs(f[:, m1.layout.obq + 7]).min() > 0
    ga, _ = H.grads_at(m1, idx)                                     # one armed step in between, undone below
    m1.set_flat(p); m0.set_flat(p)
    z = np.zeros(m1.n_param, np.float32)
    for m in (m0, m1):
        H.check(m._L.tsc_iql_set_opt_state(m._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    H.set_dueling(m1, 0)
    assert H.get_dueling(m1) == 0
    with pytest.raises(RuntimeError, match='tsc_iql_debug_targets'):
        H.targets(m1)
    (g0, s0), (g1, s1) = H.grads_at(m0, idx), H.grads_at(m1, idx)
    assert np.abs(g0).max() > 0 and np.abs(ga - g0).max() > 0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
    lay = m0.layout
    assert (g0.reshape(lay.A, lay.stride)[:, lay.obq + 7] == 0).all()           # the default step leaves the V column without a gradient
    act0, q0 = m0.forward(torch.from_numpy(H.rand_obs(scn, E, np.random.RandomState(1))).cuda())
    act1, q1 = m1.forward(torch.from_numpy(H.rand_obs(scn, E, np.random.RandomState(1))).cuda())
    np.testing.assert_array_equal(q1.cpu().numpy(), q0.cpu().numpy())
    np.testing.assert_array_equal(act1.cpu().numpy(), act0.cpu().numpy())
    m0.close(); m1.close()


# ---- 6. routes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[1], CASES[3], CASES[2]])
def test_routes(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A dueling step on the fused path: one iql_target, one iql_grad, one iql_reduce, with or without a target network; on the grouped path
    none of the three; after disarming the unarmed counts.  (A handle made with dueling = 1 and a head away from its initialisation;
    tests/test_iql_plan_gpu.py arms a plain handle through every route.)"""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.duel_model(scenario, E, cap)
    on = m.fused
    assert on == (fused == '1')
    H.fill([m], None, scn, E, cap, np.random.RandomState(E + cap))
    _lib.profile(enable=True)
    try:
        # launches of H.KERNELS: iql_sample, iql_per_sample, iql_nstep, iql_target, iql_grad, iql_reduce, iql_per_update, iql_per_add
        for duel, period, double_q, fused_counts in [(1, 0, 0, [1, 0, 0, 1, 1, 1, 0, 0]), (1, 100, 0, [1, 0, 0, 1, 1, 1, 0, 0]),
                                                     (1, 100, 1, [1, 0, 0, 1, 1, 1, 0, 0]), (0, 0, 0, [1, 0, 0, 0, 1, 1, 0, 0])]:
            H.set_dueling(m, duel)
            H.set_target(m, period, double_q)
            _lib.profile(reset=True)
            stats = m.minibatch_step(1e-3, want_stats=True)
            got = [H.launches(k) for k in H.KERNELS]
            want = [c if on or k not in ('iql_target', 'iql_grad', 'iql_reduce') else 0 for k, c in zip(H.KERNELS, fused_counts)]
            print((duel, period, double_q), dict(zip(H.KERNELS, got)))
            assert got == want, (duel, period, double_q)
            assert np.isfinite(stats).all() and (stats[:, 1] > 0).all()
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from deeprl_signal_control_amd.iql import VecIQL
    scn, lr = H.model('large_grid', 'iqll', 'lr', 2, buffer_size=30)
    with pytest.raises(RuntimeError, match='tsc_iql_set_dueling'):
        H.set_dueling(lr, 1)
    assert H.get_dueling(lr) == 0
    with pytest.raises(RuntimeError, match='tsc_iql_set_dueling'):
        H.check(lr._L.tsc_iql_set_dueling(lr._h, 2))
    lr.close()
    with pytest.raises(ValueError, match='dueling'):
        H.model('large_grid', 'iqll', 'lr', 2, buffer_size=30, dueling=1)
    # a synthetic handle with an agent of eight actions: refused, never clamped; seven are fine
    n_s, n_w = [12, 12, 12], [4, 4, 4]
    cfg = dict(batch_size=20, buffer_size=30, reward_norm=100.0)
    wide = VecIQL(n_s, [3, 8, 5], n_w, 2, 12, 8, cfg, total_step=100, seed=1, model_type='dqn')
    with pytest.raises(RuntimeError, match='8 actions'):
        H.set_dueling(wide, 1)
    assert H.get_dueling(wide) == 0
    wide.close()
    with pytest.raises((RuntimeError, ValueError), match='actions'):
        VecIQL(n_s, [3, 8, 5], n_w, 2, 12, 8, dict(cfg, dueling=1), total_step=100, seed=1, model_type='dqn')
    seven = VecIQL(n_s, [3, 7, 5], n_w, 2, 12, 7, dict(cfg, dueling=1), total_step=100, seed=1, model_type='dqn')
    assert H.get_dueling(seven) == 1
    obs = torch.rand(2, 3, 12, device='cuda')
    act, q = seven.forward(obs)
    assert q.shape == (2, 3, 7) and (q[:, 0, 3:] == 0).all() and (q[:, 1] != 0).all() and (act[:, 1] == q[:, 1].argmax(1)).all()
    seven.close()


# ---- 8. checkpoint ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    scn, m = H.duel_model('large_grid', 3, 25)
    H.fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(2):
        m.minibatch_step(1e-3)
    m.save(str(tmp_path / 'duel'), 7)
    z = np.load(str(tmp_path / 'duel' / 'checkpoint-7.npz'))
    assert sorted(z.files) == ['adam_m', 'adam_v', 'counters', 'dueling', 'format', 'layout', 'params'] and int(z['dueling']) == 1
    _, f = H.model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, dueling=1)
    assert f.load(str(tmp_path / 'duel'))
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    for a, b in zip(f.get_agent_params(), m.get_agent_params()):
        np.testing.assert_array_equal(a['v_w'], b['v_w'])
        np.testing.assert_array_equal(a['v_b'], b['v_b'])
        assert np.abs(b['v_w']).max() > 0 and b['v_b'][0] != 0
    for x, y_ in zip(f.get_opt_state(), m.get_opt_state()):
        np.testing.assert_array_equal(x, y_)
    # an unarmed model's file keeps exactly its keys; neither kind of model loads the other's file
    _, u = H.model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
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
