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

from tests import iql_harness as H
from tests.iql_harness import CASES, INI

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_armed_with_target_equal_to_parameters_is_the_unarmed_step_bit_for_bit(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """theta- = theta: per row set the same MFMA sequence on the same operands, max is order-free and the value at the first argmax
    is the max -- gradient buffer and loss of one fixed draw are equal bit for bit, unarmed / target / target + double."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=100)
    _, m2 = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=100, double_q=1)
    assert m0.fused == m1.fused == m2.fused == (fused == '1')
    np.testing.assert_array_equal(m0.get_flat(), m1.get_flat())
    np.testing.assert_array_equal(m1.get_flat(), m1.get_target_flat())
    np.testing.assert_array_equal(m2.get_flat(), m2.get_target_flat())
    rng = np.random.RandomState(cap + E)
    size = H.fill([m0, m1, m2], None, scn, E, cap, rng)[0]
    idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    (g0, s0), (g1, s1), (g2, s2) = (H.grads_at(m, idx) for m in (m0, m1, m2))
    assert np.abs(g0).max() > 0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(g2, g0)
    np.testing.assert_array_equal(s1[:, 0], s0[:, 0])
    np.testing.assert_array_equal(s2[:, 0], s0[:, 0])
    y1, a1 = H.targets(m1)
    y2, a2 = H.targets(m2)
    np.testing.assert_array_equal(y1, y2)
    assert (a1 == -1).all() and (a2 >= 0).all() and all((a2[a] < n).all() for a, n in enumerate(scn.n_a_ls))
    for m in (m0, m1, m2):
        m.close()


@pytest.mark.parametrize('double_q', [0, 1])
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, double_q, monkeypatch):
    """theta- != theta (two seeded initialisations): y and a* of every sampled row, loss, clip norm and every gradient tensor."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=100, double_q=double_q)
    assert m.fused == (fused == '1')
    H.targets_and_gradient_vs_oracle(scn, m, H.oracle_for(m), E, cap, np.random.RandomState(cap + E + double_q))
    m.close()


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[1], CASES[3]])
def test_refresh_schedule(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """target_update = 2: theta- is the parameters as they stood after Adam steps 2 and 4 and does not move at steps 1, 3, 5."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=2, double_q=1)
    H.fill([m], None, scn, E, cap, np.random.RandomState(3))
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


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_default_path_is_untouched(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that was never armed and one that was armed and disarmed again: equal gradients and parameters over two steps, and
    no launch of the target kernel from either."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(11)
    size = H.fill([m0, m1], None, scn, E, cap, rng)[0]
    idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    H.set_target(m1, 3, 1)
    ga, _ = H.grads_at(m1, idx)                                     # one armed step in between, undone below
    m1.set_flat(m0.get_flat())
    z = np.zeros(m1.n_param, np.float32)
    _lib.check(m1._L.tsc_iql_set_opt_state(m1._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    H.set_target(m1, 0, 0)
    with pytest.raises(RuntimeError, match='double_q'):
        H.set_target(m1, 0, 1)
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
            (g0, s0), (g1, s1) = H.grads_at(m0, idx), H.grads_at(m1, idx)
            np.testing.assert_array_equal(g1, g0)
            np.testing.assert_array_equal(s1, s0)
            np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        assert H.launches('iql_target') == 0
        if m1.fused:                                               # (the counter does count: an armed fused step launches the kernel)
            H.set_target(m1, 3, 0)
            H.grads_at(m1, idx)
            assert H.launches('iql_target') == 1
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m0.close(); m1.close()


def test_checkpoint_round_trip(tmp_path):
    scn, m = H.model('large_grid', 'iqld', 'dqn', 3, buffer_size=25, target_update=3, double_q=1)
    H.fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(4):                                             # theta- = the parameters after step 3, one step behind
        m.minibatch_step(1e-3)
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0
    m.save(str(tmp_path / 'armed'), 7)
    z = np.load(str(tmp_path / 'armed' / 'checkpoint-7.npz'))
    np.testing.assert_array_equal(z['target'], m.get_target_flat())
    _, f = H.model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, target_update=3, double_q=1)
    assert f.load(str(tmp_path / 'armed'))
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    np.testing.assert_array_equal(f.get_target_flat(), m.get_target_flat())
    for x, y_ in zip(f.get_opt_state(), m.get_opt_state()):
        np.testing.assert_array_equal(x, y_)
    assert (f.act_step, f.update_step) == (m.act_step, m.update_step) and f.get_opt_state()[2] == 4
    # an unarmed model: exactly the keys a checkpoint had before there was a target network; an armed model loads it with theta- = theta
    _, u = H.model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
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
        H.model('small_grid', 'iqld', 'dqn', 2, double_q=1)
    # the E = 1 adaptor arms its handle from the config too
    one = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20, buffer_size=40, reward_norm=100.0, target_update=4), seed=1)
    np.testing.assert_array_equal(one.get_target_flat(), one.vec.get_flat())
    one.set_target_flat(one.get_target_flat() * 2)
    assert np.abs(one.get_target_flat() - one.vec.get_flat()).max() > 0
    one.sync_target()
    np.testing.assert_array_equal(one.get_target_flat(), one.vec.get_flat())
    one.vec.close()


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
