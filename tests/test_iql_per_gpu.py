"""GPU tests of the opt-in prioritized replay of the Q-learners ([MODEL_CONFIG] prioritized_replay / per_alpha / per_beta / per_eps;
include/tsc.h tsc_iql_set_per; csrc/tsc_iql.hip iql_per_sample_kernel, iql_per_update_kernel, iql_per_add_kernel, iql_td_kernel<true> and
csrc/tsc_iql_fused.h iql_fused_grad_kernel<.., true, true>) against the float64 restatement of tests/iql_ext_oracle.py.

Shapes: tests/test_iql_target_gpu.py::CASES, the smallest at which each gradient path can go wrong, plus two IQL-LR rings for the sampler
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

from tests.test_iql_gpu import _kinks
from tests.test_iql_target_gpu import (CASES, INI, _disagreeing_target, _draw_idx, _fill, _grads_at, _model,
                                       _rand_obs_decided)

pytestmark = pytest.mark.gpu

SAMPLER_CASES = [('large_grid', 'iqll', 'lr', 2, 150, '0'), ('large_grid', 'iqll', 'lr', 2, 1000, '0')]
TARGETS = [(0, 0), (100, 0), (100, 1)]


def _check(rc):
    from deeprl_signal_control_amd import _lib
    _lib.check(rc)


def _set_per(m, enable, alpha=0.6, eps=0.01):
    _check(m._L.tsc_iql_set_per(m._h, enable, alpha, eps))


def _set_beta(m, beta):
    _check(m._L.tsc_iql_set_per_beta(m._h, beta))


def _per_debug(m):
    R = m.E * m.n_step
    w, td = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.float32)
    _check(m._L.tsc_iql_debug_per(m._h, w.ctypes.data_as(C.c_void_p), td.ctypes.data_as(C.c_void_p)))
    return w, td


def _batch(m):
    idx = np.zeros((m.E, m.n_agent, m.n_step), np.int32)
    _check(m._L.tsc_iql_debug_batch(m._h, idx.ctypes.data_as(C.c_void_p)))
    return idx


def _launches(name):
    from deeprl_signal_control_amd import _lib
    ms, cnt = C.c_double(), C.c_int64()
    _lib.check(_lib.lib().tsc_profile_read(_lib.profile_names().index(name), C.byref(ms), C.byref(cnt)))
    return int(cnt.value)


def _random_priorities(m, size, rng):
    """Random priorities over four decades with a fifth of the filled slots at 0; ring (0, 0) keeps its whole mass in its last filled
    slot, ring (0, 1) in its first; the slots behind `size` hold a large value that must never be drawn."""
    prio, qmax = m.get_priorities()
    cap = prio.shape[2]
    q = (10.0 ** rng.uniform(-2, 2, prio.shape)).astype(np.float32)
    q[rng.rand(*prio.shape) < 0.2] = 0
    q[0, 0, :] = 0; q[0, 0, size - 1] = 3.5
    q[0, 1, :] = 0; q[0, 1, 0] = 0.25
    dead = q[:, :, :size].max(2) == 0
    q[dead, 0] = 1.0
    q[:, :, size:] = 1e6
    assert cap >= size
    m.set_priorities(q, np.maximum(qmax, q[:, :, :size].max(2)))
    got, _ = m.get_priorities()
    np.testing.assert_array_equal(got, q)
    return q


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
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap, **tk)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=0.0, **tk)
    _, m2 = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=0.6, **tk)
    assert m0.fused == m1.fused == m2.fused == (fused == '1')
    _set_beta(m1, 0.4)
    _set_beta(m2, 1.0)
    rng = np.random.RandomState(cap + E)
    size = _fill([m0, m1, m2], None, scn, E, cap, rng)
    prio, qmax = m2.get_priorities()
    assert (prio[:, :, :size] == 1).all() and (qmax == 1).all()
    for step in range(3):
        idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
        (g0, s0), (g1, s1) = _grads_at(m0, idx), _grads_at(m1, idx)
        assert np.abs(g0).max() > 0
        np.testing.assert_array_equal(g1, g0)
        np.testing.assert_array_equal(s1, s0)
        np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        w, td = _per_debug(m1)
        assert (w == 1).all() and td.max() > 0
        prio, qmax = m1.get_priorities()
        assert (prio[:, :, :size] == 1).all() and (qmax == 1).all()
        if step == 0:
            g2, s2 = _grads_at(m2, idx)
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
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    rng = np.random.RandomState(cap + 3 * E)
    if (agent, E) == ('iqll', 2):                   # the sampler's own rings: cap 150 filled past its capacity, cap 1000 filled to it
        z = torch.zeros(E, scn.n_agent, scn.s_max, device='cuda')
        act, rew = torch.zeros(E, scn.n_agent, dtype=torch.int32, device='cuda'), -torch.ones(E, scn.n_agent, dtype=torch.float64, device='cuda')
        done = torch.zeros(E, dtype=torch.uint8, device='cuda')
        for t in range(157 if cap == 150 else 1000):
            m.add_transition(z, act, rew, z, done)
        size = cap
    else:
        size = _fill([m], None, scn, E, cap, rng)
    assert m.replay_size()[0] == size
    q = _random_priorities(m, size, rng)
    _check(m._L.tsc_iql_compute_grads(m._h, 77, 5))
    idx = _batch(m)
    _check_draw(idx, q, size, 77, 5)
    assert (idx[0, 0] == size - 1).all() and (idx[0, 1] == 0).all()
    assert (np.diff(idx, axis=2) >= 0).all()                                   # strata are ordered, so the picks are
    # the same (seed, update_index) on the same priorities: the same draw
    m.set_priorities(q, m.get_priorities()[1])
    _check(m._L.tsc_iql_compute_grads(m._h, 77, 5))
    np.testing.assert_array_equal(_batch(m), idx)
    _check(m._L.tsc_iql_compute_grads(m._h, 77, 6))
    assert (_batch(m) != idx).any()
    # three minibatch steps, each checked against the priorities read before it (the write-back of one step feeds the next draw)
    for step in range(3):
        before, _ = m.get_priorities()
        upd = m.update_step
        m.minibatch_step(1e-3)
        _check_draw(_batch(m), before, size, m.replay_seed, upd)
        assert (m.get_priorities()[0] != before).any()
    m.close()


# ---- 3. weights, loss, gradient --------------------------------------------------------------------------------------------------
def _per_step_vs_oracle(scn, m, E, cap, rng, target_update, double_q, beta):
    from tests.iql_ext_oracle import ExtOracleIQL, per_weights
    o = ExtOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, per=True, alpha=0.6, eps=0.01, target_update=target_update,
                     double_q=bool(double_q), batch_size=m.n_step, buffer_size=cap, gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'],
                     reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'], replay_seed=m.replay_seed)
    A, B = scn.n_agent, m.n_step
    size = _fill([m], o, scn, E, cap, rng, draw_next=lambda: _rand_obs_decided(scn, E, rng, o))
    if target_update:
        m.set_target_flat(m.layout.pack(_disagreeing_target(m, o)))
        o.set_target_params(m.layout.unpack(m.get_target_flat()))
        assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0.01
    q = _random_priorities(m, size, rng)
    o.prio[:], o.qmax[:] = q, m.get_priorities()[1]
    _set_beta(m, beta)
    params_before = [{k: v.clone() for k, v in x.p.items()} for x in o.qs]
    rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
    _check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = _batch(m)
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    w, td = _per_debug(m)
    stats = np.zeros((A, 2))
    _check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3, beta=beta, idx_given=idx)        # the device's draw (check 2 is test_draw's)
    wr = w.reshape(A, E, B)
    assert (wr.max(2) == 1).all() and (w > 0).all() and w.min() < 0.5
    for e in range(E):
        for a in range(A):
            np.testing.assert_allclose(wr[a, e], per_weights(q[e, a], size, idx[e, a], beta), rtol=1e-6, atol=0)
    np.testing.assert_allclose(w, o.last_w, rtol=1e-6, atol=0)
    print('max |d|delta|| %.2e' % np.abs(td - o.last_td).max())
    np.testing.assert_allclose(td, o.last_td, rtol=0, atol=2e-5)
    tol = 2e-5
    for a in range(A):
        x = o.qs[a]
        saved, x.p = x.p, params_before[a]
        cols, deep = _kinks(o, [rows_before[a][e][s][0] for e in range(E) for s in idx[e, a]], a)
        x.p = saved
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


@pytest.mark.parametrize('beta', [0.4, 1.0])
@pytest.mark.parametrize('target_update,double_q', TARGETS)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_weights_loss_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, target_update, double_q, beta, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, target_update=target_update, double_q=double_q)
    assert m.fused == (fused == '1')
    _per_step_vs_oracle(scn, m, E, cap, np.random.RandomState(cap + E + double_q + target_update), target_update, double_q, beta)
    m.close()


# ---- 4. write-back ---------------------------------------------------------------------------------------------------------------
def _expected_after(before, qmax_before, idx, td, size, alpha, eps):
    """The priorities after the write-back of one step from the device's own |delta|: picks in order, the last pick of a slot stays."""
    E, A, B = idx.shape
    want, wmax = before.copy(), qmax_before.copy()
    hit = np.zeros(before.shape, bool)
    for e in range(E):
        for a in range(A):
            for i, s in enumerate(np.clip(idx[e, a], 0, size - 1)):
                v = np.float32((np.float64(td[a, e * B + i]) + eps) ** alpha)
                want[e, a, s], hit[e, a, s] = v, True
                wmax[e, a] = max(wmax[e, a], v)
    return want, wmax, hit


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_write_back(scenario, agent, model_type, E, cap, fused, monkeypatch):
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    alpha, eps = 0.6, 0.01
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1, per_alpha=alpha, per_eps=eps)
    rng = np.random.RandomState(2 * cap + E)
    size = _fill([m], None, scn, E, cap, rng)
    wrapped = m.replay_size()[1] > cap
    assert wrapped == (cap < 100)
    _random_priorities(m, size, rng)
    A, B = scn.n_agent, m.n_step

    def step_and_check(run):
        before, qmax_before = m.get_priorities()
        run()
        idx = _batch(m)
        w, td = _per_debug(m)
        after, qmax = m.get_priorities()
        want, wmax, hit = _expected_after(before, qmax_before, idx, td, size, alpha, eps)
        np.testing.assert_allclose(after[hit], want[hit], rtol=1e-6, atol=0)
        np.testing.assert_array_equal(after[~hit], before[~hit])               # unsampled slots: bit for bit
        np.testing.assert_allclose(qmax, wmax, rtol=1e-6, atol=0)
        assert (qmax >= qmax_before).all()                                     # a running maximum: it never falls
        return idx, hit

    idx, hit = step_and_check(lambda: _check(m._L.tsc_iql_compute_grads(m._h, 3, 9)))
    assert hit.any(2).all() and (idx < size).all()
    # a caller's draw with repeated slots: each ring draws 3 slots only, in scrambled order
    rep = np.stack([np.stack([rng.choice(rng.permutation(size)[:3], B) for _ in range(A)]) for _ in range(E)]).astype(np.int32)
    assert all(len(set(rep[e, a])) < B for e in range(E) for a in range(A))
    rep_dev = torch.from_numpy(rep).cuda()
    idx2, hit2 = step_and_check(lambda: _check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(rep_dev.data_ptr()))))
    np.testing.assert_array_equal(idx2, rep)
    assert (hit2.sum(2) <= 3).all()
    # a new transition enters every ring at the ring's running maximum (here it overwrites an old one where the ring has wrapped)
    before, qmax = m.get_priorities()
    slot = m.replay_size()[1] % cap
    _fill_one(m, scn, E, rng)
    after, qmax2 = m.get_priorities()
    np.testing.assert_array_equal(qmax2, qmax)
    np.testing.assert_array_equal(after[:, :, slot], qmax)
    keep = np.ones(cap, bool); keep[slot] = False
    np.testing.assert_array_equal(after[:, :, keep], before[:, :, keep])
    m.close()


def _fill_one(m, scn, E, rng):
    from tests.test_iql_gpu import _rand_obs
    obs, nobs = _rand_obs(scn, E, rng), _rand_obs(scn, E, rng)
    act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
    rew = -rng.rand(E, scn.n_agent) * m.cfg['reward_norm']
    m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(), torch.from_numpy(nobs).cuda(),
                     torch.zeros(E, dtype=torch.uint8, device='cuda'))


# ---- 5. the default path ---------------------------------------------------------------------------------------------------------
PER_KERNELS = ('iql_per_sample', 'iql_per_update', 'iql_per_add')


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_default_path_is_untouched(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """A handle that never arms and one that was armed and disarmed again: equal gradients and parameters over two steps and an add, and
    no launch of a prioritized-replay kernel from either."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(11)
    size = _fill([m0, m1], None, scn, E, cap, rng)
    idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
    _set_per(m1, 1, 0.6, 0.01)
    _grads_at(m1, idx)                                              # one armed step in between, undone below
    m1.set_flat(m0.get_flat())
    z = np.zeros(m1.n_param, np.float32)
    _check(m1._L.tsc_iql_set_opt_state(m1._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    _set_per(m1, 0)
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = _draw_idx(rng, E, scn.n_agent, m0.n_step, size)
            (g0, s0), (g1, s1) = _grads_at(m0, idx), _grads_at(m1, idx)
            np.testing.assert_array_equal(g1, g0)
            np.testing.assert_array_equal(s1, s0)
            np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        # the library's own draw: Floyd's on both
        _check(m0._L.tsc_iql_compute_grads(m0._h, 5, 1)); _check(m1._L.tsc_iql_compute_grads(m1._h, 5, 1))
        np.testing.assert_array_equal(_batch(m1), _batch(m0))
        np.testing.assert_array_equal(m1.grad_tensor().cpu().numpy(), m0.grad_tensor().cpu().numpy())
        assert all(len(set(r)) == m0.n_step for r in _batch(m0).reshape(-1, m0.n_step))
        for m in (m0, m1):
            _fill_one(m, scn, E, np.random.RandomState(1))
        assert [_launches(k) for k in PER_KERNELS] == [0, 0, 0]
        _set_per(m1, 1, 0.6, 0.01)                                  # (the counters do count)
        _grads_at(m1, idx)
        _fill_one(m1, scn, E, rng)
        assert [_launches(k) for k in PER_KERNELS] == [1, 1, 1]
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m0.close(); m1.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    scenario, agent, model_type, E, cap, fused = CASES[1]
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    _, twin = _model(scenario, agent, model_type, E, buffer_size=cap, prioritized_replay=1)
    _, plain = _model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(6)
    size = _fill([m, twin, plain], None, scn, E, cap, rng)
    q = _random_priorities(m, size, np.random.RandomState(7))
    _random_priorities(twin, size, np.random.RandomState(7))
    _set_beta(m, 0.7); _set_beta(twin, 0.7)
    with pytest.raises(RuntimeError, match='no tsc_iql_compute_grads'):
        _per_debug(m)
    with pytest.raises(RuntimeError, match='alpha'):
        _set_per(m, 1, -0.1, 0.01)
    for eps in (0.0, -1.0):
        with pytest.raises(RuntimeError, match='eps'):
            _set_per(m, 1, 0.6, eps)
    for beta in (-0.01, 1.5, float('nan')):
        with pytest.raises(RuntimeError, match='beta'):
            _set_beta(m, beta)
    bad = q.copy(); bad[1, 2, :size] = 0
    with pytest.raises(RuntimeError, match='no positive priority'):
        m.set_priorities(bad, np.ones((E, scn.n_agent), np.float32))
    bad = q.copy(); bad[0, 3, 1] = -1.0
    with pytest.raises(RuntimeError, match='>= 0'):
        m.set_priorities(bad, np.ones((E, scn.n_agent), np.float32))
    # nothing has changed: priorities, and the next step (draw, weights, gradient) is the twin's that saw none of this
    np.testing.assert_array_equal(m.get_priorities()[0], q)
    for x in (m, twin):
        _check(x._L.tsc_iql_compute_grads(x._h, 1, 2))
    np.testing.assert_array_equal(_batch(m), _batch(twin))
    np.testing.assert_array_equal(_per_debug(m)[0], _per_debug(twin)[0])
    np.testing.assert_array_equal(m.grad_tensor().cpu().numpy(), twin.grad_tensor().cpu().numpy())
    np.testing.assert_array_equal(m.get_priorities()[0], twin.get_priorities()[0])
    # an unarmed handle
    g_before = _grads_at(plain, _draw_idx(np.random.RandomState(1), E, scn.n_agent, plain.n_step, size))[0]
    for call in (plain.get_priorities, lambda: plain.set_priorities(q, np.ones((E, scn.n_agent), np.float32)), lambda: _per_debug(plain)):
        with pytest.raises(RuntimeError, match='tsc_iql_set_per'):
            call()
    assert np.abs(g_before).max() > 0
    # a ring the sampler cannot stage: refused by name when the model arms
    with pytest.raises(RuntimeError, match='TSC_IQL_PER_MAX_BUFFER'):
        _model('large_grid', 'iqll', 'lr', 1, buffer_size=4097, prioritized_replay=1)
    # ... and the bound itself is accepted and draws (45 of its 4096 slots filled)
    sb, big = _model('large_grid', 'iqll', 'lr', 1, buffer_size=4096, prioritized_replay=1)
    nb = _fill([big], None, sb, 1, 4096, rng)
    qb = _random_priorities(big, nb, rng)
    _check(big._L.tsc_iql_compute_grads(big._h, 4, 4))
    _check_draw(_batch(big), qb, nb, 4, 4)
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
    scn, m = _model('large_grid', 'iqld', 'dqn', 3, buffer_size=25, prioritized_replay=1, per_beta=0.4)
    _fill([m], None, scn, 3, 25, np.random.RandomState(4))
    for _ in range(3):
        m.backward()
    assert m.per_n == 3 * m.n_step == m.lr_scheduler.n and m.current_per_beta() == per_beta_at(0.4, 60, 10000) > 0.4
    m.save(str(tmp_path / 'armed'), 7)
    z = np.load(str(tmp_path / 'armed' / 'checkpoint-7.npz'))
    assert sorted(z.files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params', 'per_n'] and int(z['per_n']) == 60
    _, f = _model('large_grid', 'iqld', 'dqn', 3, seed=9, buffer_size=25, prioritized_replay=1, per_beta=0.4)
    assert f.per_n == 0 and f.load(str(tmp_path / 'armed'))
    assert f.per_n == 60 and f.current_per_beta() == m.current_per_beta()
    np.testing.assert_array_equal(f.get_flat(), m.get_flat())
    # the rings are not checkpointed, so neither are their priorities: a resumed run refills both
    assert f.replay_size() == (0, 0)
    # an unarmed model's file keeps its keys, and an armed model loads it with the learning rate's counter
    _, u = _model('large_grid', 'iqld', 'dqn', 3, seed=2, buffer_size=25)
    u.lr_scheduler.n = 40
    u.save(str(tmp_path / 'plain'), 1)
    assert sorted(np.load(str(tmp_path / 'plain' / 'checkpoint-1.npz')).files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params']
    assert f.load(str(tmp_path / 'plain')) and f.per_n == 40
    assert u.load(str(tmp_path / 'armed'))
    with pytest.raises(RuntimeError, match='tsc_iql_set_per'):
        u.get_priorities()
    for x in (m, f, u):
        x.close()
