"""GPU tests of the opt-in prioritized replay of the Q-learners ([MODEL_CONFIG] prioritized_replay / per_alpha / per_beta / per_eps;
include/tsc.h tsc_iql_set_per; csrc/tsc_iql.hip iql_per_sample_kernel, iql_per_update_kernel, iql_per_add_kernel, iql_td_kernel<true> and
csrc/tsc_iql_fused.h iql_fused_grad_kernel<.., true, true>) against the float64 restatement of tests/iql_ext_oracle.py.

Shapes: tests/iql_harness.py::CASES, the smallest at which each gradient path can go wrong, plus two IQL-LR rings for the sampler
alone: buffer_size 150 filled past its capacity (size = 150 = 2 x 64 + 22: the 64 lanes' blocks are ragged, the last lanes own nothing)
and buffer_size 1000 filled to 1000 (the benchmarked ring: 16 slots per lane, the last block partial).

Tolerances are the project's (tests/test_iql_gpu.py): Q values, hence y and |delta|, within 2e-5; gradients within 2e-5 max|g| per tensor
with hidden units within 1e-6 of a ReLU kink excepted; loss and clip norm rtol 1e-4.  Weights and written-back priorities are float32
roundings of float64 expressions of the device's own float32 inputs: rtol 1e-6 (float32 epsilon is 1.2e-7; pow in float64 is good to a
few ulp of float64).  The draw: C in extended precision from the device's float32 priorities, slack d = 1e-9 total (a float64 sum of 1000
float32 terms is good to about 1e-13 relative)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import iql_harness as H
from tests.iql_harness import CASES, INI

pytestmark = pytest.mark.gpu

SAMPLER_CASES = [('large_grid', 'iqll', 'lr', 2, 150, '0'), ('large_grid', 'iqll', 'lr', 2, 1000, '0')]
TARGETS = [(0, 0), (100, 0), (100, 1)]


def _check_draw(idx, prio, size, seed, upd):
    """Check 2 of the draw on every ring: pick i of ring p = e A + a against t_i = (i + U(seed, upd, p B + i)) total / B."""
    from oracle.nets_oracle import sample_uniform
    E, A, B = idx.shape
    i = np.arange(B)
    for e in range(E):
        for a in range(A):
            q = prio[e, a, :size]
            Cs = np.cumsum(q.astype(np.longdouble))
            total = Cs[-1]
            d = 1e-9 * total
            k = idx[e, a].astype(np.int64)
            assert (k >= 0).all() and (k < size).all() and (q[k] > 0).all(), (e, a, k)
            u = np.array([sample_uniform(seed, upd, (e * A + a) * B + j) for j in range(B)], np.longdouble)
            t = (i + u) * total / B
            below = np.where(k > 0, Cs[np.maximum(k - 1, 0)], 0)
            assert (below - d <= t).all() and (t <= Cs[k] + d).all(), (e, a, k, t, Cs[k])
            # pick i lies in stratum i of the cumulative mass
            assert (below <= (i + 1) * total / B + d).all() and (Cs[k] >= i * total / B - d).all(), (e, a)


# ---- 1. a fresh armed handle is the unarmed step ---------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update,double_q', [(0, 0), (100, 1)])
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_fresh_armed_handle_is_the_unarmed_step_bit_for_bit(scenario, agent, model_type, E, cap, fused, target_update, double_q, monkeypatch):
    """All q = 1: size q / total is exactly 1, every weight exactly 1, and 2 d w / R, d d w / R round like 2 d / R, d d / R -- gradient
    buffer, loss, clip norm and the parameters after Adam are those of the unarmed handle on the same draw.  alpha = 0 writes 1 back, so it
    stays so over three steps; alpha = 0.6 is compared on its first."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    tk = dict(target_update=target_update, double_q=double_q)
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap, **tk)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=0.0, **tk)
    _, m2 = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=0.6, **tk)
    assert m0.fused == m1.fused == m2.fused == (fused == '1')
    H.set_beta(m1, 0.4)
    H.set_beta(m2, 1.0)
    rng = np.random.RandomState(cap + E)
    size = H.fill([m0, m1, m2], None, scn, E, cap, rng)[0]
    prio, qmax = m2.get_priorities()
    assert (prio[:, :, :size] == 1).all() and (qmax == 1).all()
    for step in range(3):
        idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
        (g0, s0), (g1, s1) = H.grads_at(m0, idx), H.grads_at(m1, idx)
        assert np.abs(g0).max() > 0
        np.testing.assert_array_equal(g1, g0)
        np.testing.assert_array_equal(s1, s0)
        np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        w, td = H.per_debug(m1)
        assert (w == 1).all() and td.max() > 0
        prio, qmax = m1.get_priorities()
        assert (prio[:, :, :size] == 1).all() and (qmax == 1).all()
        if step == 0:
            g2, s2 = H.grads_at(m2, idx)
            np.testing.assert_array_equal(g2, g0)
            np.testing.assert_array_equal(s2, s0)
            np.testing.assert_array_equal(m2.get_flat(), m0.get_flat())
            assert (m2.get_priorities()[0][:, :, :size] != 1).any()
    for m in (m0, m1, m2):
        m.close()


# ---- 2. the draw -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES + SAMPLER_CASES)
def test_draw(scenario, agent, model_type, E, cap, fused, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    rng = np.random.RandomState(cap + 3 * E)
    if (agent, E) == ('iqll', 2):                   # the sampler's own rings: cap 150 filled past its capacity, cap 1000 filled to it
        z = torch.zeros(E, scn.n_agent, scn.s_max, device='cuda')
        act, rew = torch.zeros(E, scn.n_agent, dtype=torch.int32, device='cuda'), -torch.ones(E, scn.n_agent, dtype=torch.float64, device='cuda')
        done = torch.zeros(E, dtype=torch.uint8, device='cuda')
        for t in range(157 if cap == 150 else 1000):
            m.add_transition(z, act, rew, z, done)
        size = cap
    else:
        size = H.fill([m], None, scn, E, cap, rng)[0]
    assert m.replay_size()[0] == size
    q = H.random_priorities(m, size, rng)
    H.check(m._L.tsc_iql_compute_grads(m._h, 77, 5))
    idx = H.batch(m)
    _check_draw(idx, q, size, 77, 5)
    assert (idx[0, 0] == size - 1).all() and (idx[0, 1] == 0).all()
    assert (np.diff(idx, axis=2) >= 0).all()                                   # strata are ordered, so the picks are
    # the same (seed, update_index) on the same priorities: the same draw
    m.set_priorities(q, m.get_priorities()[1])
    H.check(m._L.tsc_iql_compute_grads(m._h, 77, 5))
    np.testing.assert_array_equal(H.batch(m), idx)
    H.check(m._L.tsc_iql_compute_grads(m._h, 77, 6))
    assert (H.batch(m) != idx).any()
    # three minibatch steps, each checked against the priorities read before it (the write-back of one step feeds the next draw)
    for step in range(3):
        before, _ = m.get_priorities()
        upd = m.update_step
        m.minibatch_step(1e-3)
        _check_draw(H.batch(m), before, size, m.replay_seed, upd)
        assert (m.get_priorities()[0] != before).any()
    m.close()


# ---- 3. weights, loss, gradient --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.4, 1.0])
@pytest.mark.parametrize('target_update,double_q', TARGETS)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_weights_loss_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, target_update, double_q, beta, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, target_update=target_update, double_q=double_q)
    assert m.fused == (fused == '1')
    H.per_step_vs_oracle(scn, m, E, cap, np.random.RandomState(cap + E + double_q + target_update), beta)
    m.close()


# ---- 4. write-back ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_write_back(scenario, agent, model_type, E, cap, fused, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    alpha, eps = 0.6, 0.01
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=alpha, per_eps=eps)
    rng = np.random.RandomState(2 * cap + E)
    size = H.fill([m], None, scn, E, cap, rng)[0]
    wrapped = m.replay_size()[1] > cap
    assert wrapped == (cap < 100)
    H.random_priorities(m, size, rng)
    A, B = scn.n_agent, m.n_step

    def step_and_check(run):
        before, qmax_before = m.get_priorities()
        run()
        idx = H.batch(m)
        w, td = H.per_debug(m)
        hit = H.check_write_back(m, before, qmax_before, idx, td, size)        # (unsampled slots: bit for bit)
        assert (m.get_priorities()[1] >= qmax_before).all()                    # a running maximum: it never falls
        return idx, hit

    idx, hit = step_and_check(lambda: H.check(m._L.tsc_iql_compute_grads(m._h, 3, 9)))
    assert hit.any(2).all() and (idx < size).all()
    # a caller's draw with repeated slots: each ring draws 3 slots only, in scrambled order
    rep = np.stack([np.stack([rng.choice(rng.permutation(size)[:3], B) for _ in range(A)]) for _ in range(E)]).astype(np.int32)
    assert all(len(set(rep[e, a])) < B for e in range(E) for a in range(A))
    rep_dev = torch.from_numpy(rep).cuda()
    idx2, hit2 = step_and_check(lambda: H.check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(rep_dev.data_ptr()))))
    np.testing.assert_array_equal(idx2, rep)
    assert (hit2.sum(2) <= 3).all()
    # a new transition enters every ring at the ring's running maximum (here it overwrites an old one where the ring has wrapped)
    before, qmax = m.get_priorities()
    slot = m.replay_size()[1] % cap
    H.fill_one(m, scn, E, rng)
    after, qmax2 = m.get_priorities()
    np.testing.assert_array_equal(qmax2, qmax)
    np.testing.assert_array_equal(after[:, :, slot], qmax)
    keep = np.ones(cap, bool); keep[slot] = False
    np.testing.assert_array_equal(after[:, :, keep], before[:, :, keep])
    m.close()


# ---- 5. the default path ---------------------------------------------------------------------------------------------------------
PER_KERNELS = ('iql_per_sample', 'iql_per_update', 'iql_per_add')


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_default_path_is_untouched(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that never arms and one that was armed and disarmed again: equal gradients and parameters over two steps and an add, and
    no launch of a prioritized-replay kernel from either."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(11)
    size = H.fill([m0, m1], None, scn, E, cap, rng)[0]
    idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    H.set_per(m1, 1, 0.6, 0.01)
    H.grads_at(m1, idx)                                              # one armed step in between, undone below
    m1.set_flat(m0.get_flat())
    z = np.zeros(m1.n_param, np.float32)
    H.check(m1._L.tsc_iql_set_opt_state(m1._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    H.set_per(m1, 0)
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = H.draw_idx(rng, E, scn.n_agent, m0.n_step, size)
            (g0, s0), (g1, s1) = H.grads_at(m0, idx), H.grads_at(m1, idx)
            np.testing.assert_array_equal(g1, g0)
            np.testing.assert_array_equal(s1, s0)
            np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        # the library's own draw: Floyd's on both
        H.check(m0._L.tsc_iql_compute_grads(m0._h, 5, 1)); H.check(m1._L.tsc_iql_compute_grads(m1._h, 5, 1))
        np.testing.assert_array_equal(H.batch(m1), H.batch(m0))
        np.testing.assert_array_equal(m1.grad_tensor().cpu().numpy(), m0.grad_tensor().cpu().numpy())
        assert all(len(set(r)) == m0.n_step for r in H.batch(m0).reshape(-1, m0.n_step))
        for m in (m0, m1):
            H.fill_one(m, scn, E, np.random.RandomState(1))
        assert [H.launches(k) for k in PER_KERNELS] == [0, 0, 0]
        H.set_per(m1, 1, 0.6, 0.01)                                  # (the counters do count)
        H.grads_at(m1, idx)
        H.fill_one(m1, scn, E, rng)
        assert [H.launches(k) for k in PER_KERNELS] == [1, 1, 1]
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m0.close(); m1.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    scenario, agent, model_type, E, cap, fused = CASES[1]
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    _, twin = H.model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    _, plain = H.model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(6)
    size = H.fill([m, twin, plain], None, scn, E, cap, rng)[0]
    q = H.random_priorities(m, size, np.random.RandomState(7))
    H.random_priorities(twin, size, np.random.RandomState(7))
    H.set_beta(m, 0.7); H.set_beta(twin, 0.7)
    with pytest.raises(RuntimeError, match='no tsc_iql_compute_grads'):
        H.per_debug(m)
    with pytest.raises(RuntimeError, match='alpha'):
        H.set_per(m, 1, -0.1, 0.01)
    for eps in (0.0, -1.0):
        with pytest.raises(RuntimeError, match='eps'):
            H.set_per(m, 1, 0.6, eps)
    for beta in (-0.01, 1.5, float('nan')):
        with pytest.raises(RuntimeError, match='beta'):
            H.set_beta(m, beta)
    bad = q.copy(); bad[1, 2, :size] = 0
    with pytest.raises(RuntimeError, match='no positive priority'):
        m.set_priorities(bad, np.ones((E, scn.n_agent), np.float32))
    bad = q.copy(); bad[0, 3, 1] = -1.0
    with pytest.raises(RuntimeError, match='>= 0'):
        m.set_priorities(bad, np.ones((E, scn.n_agent), np.float32))
    # nothing has changed: priorities, and the next step (draw, weights, gradient) is the twin's that saw none of this
    np.testing.assert_array_equal(m.get_priorities()[0], q)
    for x in (m, twin):
        H.check(x._L.tsc_iql_compute_grads(x._h, 1, 2))
    np.testing.assert_array_equal(H.batch(m), H.batch(twin))
    np.testing.assert_array_equal(H.per_debug(m)[0], H.per_debug(twin)[0])
    np.testing.assert_array_equal(m.grad_tensor().cpu().numpy(), twin.grad_tensor().cpu().numpy())
    np.testing.assert_array_equal(m.get_priorities()[0], twin.get_priorities()[0])
    # an unarmed handle
    g_before = H.grads_at(plain, H.draw_idx(np.random.RandomState(1), E, scn.n_agent, plain.n_step, size))[0]
    for call in (plain.get_priorities, lambda: plain.set_priorities(q, np.ones((E, scn.n_agent), np.float32)), lambda: H.per_debug(plain)):
        with pytest.raises(RuntimeError, match='tsc_iql_set_per'):
            call()
    assert np.abs(g_before).max() > 0
    # a ring the sampler cannot stage: refused by name when the model arms
    with pytest.raises(RuntimeError, match='TSC_IQL_PER_MAX_BUFFER'):
        H.model('large_grid', 'iqll', 'lr', 1, buffer_size=4097, prioritized_replay=1)
    # ... and the bound itself is accepted and draws (45 of its 4096 slots filled)
    sb, big = H.model('large_grid', 'iqll', 'lr', 1, buffer_size=4096, prioritized_replay=1)
    nb = H.fill([big], None, sb, 1, 4096, rng)[0]
    qb = H.random_priorities(big, nb, rng)
    H.check(big._L.tsc_iql_compute_grads(big._h, 4, 4))
    _check_draw(H.batch(big), qb, nb, 4, 4)
    for x in (m, twin, plain, big):
        x.close()


# ---- 7. through the CLI -----------------------------------------------------------------------------------------------------------
def test_train_then_evaluate_with_prioritized_replay(tmp_path):
    """`train` with prioritized_replay in the INI needs nothing else: it runs and says so, its checkpoint carries the beta counter,
    `evaluate` loads it."""
    from deeprl_signal_control_amd import main as cli
    cfg = tmp_path / 'config_iqld.ini'
    cfg.write_text(INI.replace('target_update = 5\ndouble_q = 1\n', 'prioritized_replay = 1\nper_alpha = 0.5\nper_beta = 0.3\nper_eps = 0.02\n'))
    assert 'prioritized_replay = 1' in cfg.read_text()
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/iqld', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', '4'])
    assert len(rows) > 0
    logs = ''.join(open(os.path.join(base, 'iqld', 'log', f)).read() for f in os.listdir(os.path.join(base, 'iqld', 'log')))
    assert 'Training: prioritized replay, alpha 0.5, beta 0.3 -> 1, eps 0.02' in logs
    ck = base + '/iqld/model/checkpoint-120.npz'
    assert os.path.exists(ck)
    z = np.load(ck)
    assert 'target' not in z.files and int(z['per_n']) == int(z['counters'][4]) > 0
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'iqld', '--evaluation-seeds', '10000'])
    mean, std = out['iqld']
    assert mean.shape == (1,) and mean[0] < 0


def test_checkpoint_round_trip_restores_the_beta_counter(tmp_path):
    from deeprl_signal_control_amd.iql import per_beta_at
    scn, m = H.model('large_grid', 'iqld', 'dqn', 3, buffer_size=25, prioritized_replay=1, per_beta=0.4)
    H.fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(3):
        m.backward()
    assert m.per_n == 3 * m.n_step == m.lr_scheduler.n and m.current_per_beta() == per_beta_at(0.4, 60, 10000) > 0.4
    m.save(str(tmp_path / 'armed'), 7)
    z = np.load(str(tmp_path / 'armed' / 'checkpoint-7.npz'))
    assert sorted(z.files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params', 'per_n'] and int(z['per_n']) == 60
    _, f = H.model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, prioritized_replay=1, per_beta=0.4)
    assert f.per_n == 0 and f.load(str(tmp_path / 'armed'))
    assert f.per_n == 60 and f.current_per_beta() == m.current_per_beta()
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    # the rings are not checkpointed, so neither are their priorities: a resumed run refills both
    assert f.replay_size() == (0, 0)
    # an unarmed model's file keeps its keys, and an armed model loads it with the learning rate's counter
    _, u = H.model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
    u.lr_scheduler.n = 40
    u.save(str(tmp_path / 'plain'), 1)
    assert sorted(np.load(str(tmp_path / 'plain' / 'checkpoint-1.npz')).files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params']
    assert f.load(str(tmp_path / 'plain')) and f.per_n == 40
    assert u.load(str(tmp_path / 'armed'))
    with pytest.raises(RuntimeError, match='tsc_iql_set_per'):
        u.get_priorities()
    for x in (m, f, u):
        x.close()
