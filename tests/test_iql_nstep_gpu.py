"""GPU tests of the opt-in multi-step returns of the Q-learners ([MODEL_CONFIG] return_steps; include/tsc.h tsc_iql_set_return_steps;
csrc/tsc_iql.hip iql_nstep_kernel, iql_gather_nstep_kernel, iql_td_nstep_kernel<>, csrc/tsc_iql_fused.h iql_fused_target_kernel<.., QNStep>)
against the float64 restatement of tests/iql_nstep_oracle.py.

Shapes: tests/test_iql_target_gpu.py::CASES, for the reasons given there.  The rings are filled like that module's _fill (the same draws in
the same order, done at probability 0.1) past their capacity -- cap + 7 adds, so the newest slot w = 6 sits mid-ring -- except the IQL-LR
ring of 1000 slots, which takes 45 adds: the size < cap branch, where no window can wrap.  One thing is added to _fill: the fourth-newest
transition is made terminal in every instance that would otherwise keep no terminal slot, so that EVERY ring has one to draw.

Draws are the caller's (tsc_iql_compute_grads_at).  Every (instance, agent) draws w, w - 1, cap - 1 when the ring has wrapped, one slot
whose own done flag is set, and distinct random slots besides.  Before anything is compared the oracle's windows must show, among every
agent's rows: a full horizon (k = n), a window ended by done, a window ended by the newest slot, and -- where the ring has wrapped -- a
window that crossed cap - 1 -> 0.  These are conditions on the test's own inputs, not tolerances.  A full horizon cannot exist for n = 32
on these rings (22 to 64 slots; in the unfilled ring an episode of 32 steps without an end is a 3 % event), so n = 32 is held to the
other three.

Tolerances are the project's: the pre-pass outputs are exact (slot, k; G and gamma^k are one float32 rounding of the float64 value the
oracle forms with the same operations in the same order -- the build forbids contraction, so no fused multiply-add enters the device's
loop); y within 2e-5 + 2^-23 |G| per row (the Q-value tolerance of tests/test_iql_gpu.py scaled by gamma^k <= 1, plus the one rounding of
G); a* exact on every row; loss and clip norm rtol 1e-4; gradients within 2e-5 max|g| per tensor with the ReLU-kink exception of _kinks;
|delta| within 2e-5 and weights / written-back priorities rtol 1e-6 as in tests/test_iql_per_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.iql_nstep_oracle import nstep_window
from tests.test_iql_gpu import _kinks, _rand_obs
from tests.test_iql_target_gpu import CASES, GAP, _disagreeing_target, _gap_of, _grads_at, _model, _targets
from tests.test_iql_target_gpu import _rand_obs_decided as _decided_plain

pytestmark = pytest.mark.gpu


def _check(rc):
    from deeprl_signal_control_amd import _lib
    _lib.check(rc)


def _set_steps(m, n):
    _check(m._L.tsc_iql_set_return_steps(m._h, n))


def _get_steps(m):
    v = C.c_int32(-1)
    _check(m._L.tsc_iql_get_return_steps(m._h, C.byref(v)))
    return int(v.value)


def _nstep_debug(m):
    R = m.E * m.n_step
    slot = np.zeros((m.E, m.n_agent, m.n_step), np.int32)
    ret, disc, k = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.int32)
    _check(m._L.tsc_iql_debug_nstep(m._h, *[x.ctypes.data_as(C.c_void_p) for x in (slot, ret, disc, k)]))
    return slot, ret, disc, k


def _launches(name):
    from deeprl_signal_control_amd import _lib
    ms, cnt = C.c_double(), C.c_int64()
    _lib.check(_lib.lib().tsc_profile_read(_lib.profile_names().index(name), C.byref(ms), C.byref(cnt)))
    return int(cnt.value)


def _fill(models, o, scn, E, cap, rng, draw_next=None, p_done=0.1):
    """tests/test_iql_target_gpu.py::_fill (module docstring) -> (size, cum, rewards as stored [E][cap][A] float32, done [E][cap])."""
    A = scn.n_agent
    cfg = models[0].cfg
    n_add = cap + 7 if cap < 100 else 45
    draw = draw_next or (lambda: _rand_obs(scn, E, rng))
    rews, dones = np.zeros((E, cap, A), np.float32), np.zeros((E, cap), bool)
    kept = np.ones(cap, bool)                      # slots that the adds after n_add - 4 do not overwrite
    for u in range(n_add - 3, n_add):
        kept[u % cap] = False
    obs = draw()
    for t in range(n_add):
        nobs = draw()
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, A) * 3.0 * cfg['reward_norm']
        done = (rng.rand(E) < p_done).astype(np.uint8)
        if t == n_add - 4:
            kept_t = kept.copy()
            kept_t[t % cap] = False
            done[~(dones & kept_t).any(1)] = 1
        for m in models:
            m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(),
                             torch.from_numpy(nobs).cuda(), torch.from_numpy(done).cuda())
        if o is not None:
            o.add_transition(obs, act, rew, nobs, done)
        r = rew / cfg['reward_norm'] if cfg['reward_norm'] else rew
        rews[:, t % cap] = (np.clip(r, -cfg['reward_clip'], cfg['reward_clip']) if cfg['reward_clip'] else r).astype(np.float32)
        dones[:, t % cap] = done.astype(bool)
        obs = nobs
    size = min(cap, n_add)
    assert dones[:, :size].any(1).all()
    return size, n_add, rews, dones


def _given_draw(rng, dones, A, B, size, cap, cum):
    """[E][A][B] int32: per ring w, w - 1, cap - 1 when wrapped, one terminal slot, distinct random slots besides; in random order."""
    E = dones.shape[0]
    w = (cum - 1) % cap
    idx = np.zeros((E, A, B), np.int32)
    for e in range(E):
        terminal = np.nonzero(dones[e, :size])[0]
        for a in range(A):
            must = list(dict.fromkeys([w, (w - 1) % cap] + ([cap - 1] if cum > cap else []) + [int(rng.choice(terminal))]))
            rest = [int(s) for s in rng.permutation(size) if s not in must][:B - len(must)]
            idx[e, a] = rng.permutation(must + rest)
    assert idx.min() >= 0 and idx.max() < size
    return idx


def _windows(idx, rews, dones, size, cap, cum, n, gamma):
    """nstep_window on every row of a draw -> slot [E][A][B], G, disc (float64), k [A][R] and the sampled slot s [A][R]."""
    E, A, B = idx.shape
    slot = np.zeros((E, A, B), np.int32)
    G, disc, k, s_ = np.zeros((A, E * B)), np.zeros((A, E * B)), np.zeros((A, E * B), np.int32), np.zeros((A, E * B), np.int64)
    for e in range(E):
        for a in range(A):
            for i, s in enumerate(idx[e, a]):
                r = e * B + i
                slot[e, a, i], G[a, r], disc[a, r], k[a, r] = nstep_window(rews[e, :, a], dones[e], int(s), size, cap, cum, n, gamma)
                s_[a, r] = s
    return slot, G, disc, k, s_


def _require_categories(cat, cum, cap, n):
    """cat: name -> bool [A][R] from the oracle.  Every agent's rows hold at least one of each (module docstring)."""
    need = ['done', 'newest'] + (['full'] if n < 32 else []) + (['wrapped'] if cum > cap else [])
    for name in need:
        missing = [a for a in range(cat[name].shape[0]) if not cat[name][a].any()]
        assert not missing, 'no %s window among the rows of agents %s (n = %d)' % (name, missing, n)
    if cum <= cap:
        assert not cat['wrapped'].any()


def _categories_of(slot, k, s_, dones, cum, cap, n):
    E, A, B = slot.shape
    j = slot.transpose(1, 0, 2).reshape(A, -1)
    done_j = np.array([[dones[r // B, j[a, r]] for r in range(E * B)] for a in range(A)], bool)
    return dict(full=k == n, done=done_j, newest=(j == (cum - 1) % cap) & ~done_j, wrapped=j < s_)


def _reset_like(m, ref):
    m.set_flat(ref.get_flat())
    z = np.zeros(m.n_param, np.float32)
    _check(m._L.tsc_iql_set_opt_state(m._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    if m.target_update:
        m.sync_target()


# ---- 1. a disarmed handle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update', [0, 100])
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_disarmed_is_untouched(scenario, agent, model_type, E, cap, fused, target_update, monkeypatch):
    """return_steps = 1 in the config, and a handle armed with 3, stepped once and set back to 1: gradient buffer, loss, clip norm and the
    parameters after Adam of a handle that never heard of the option, bit for bit over two steps; no launch of the pre-pass from any of
    them, and no launch of the target kernel either unless a target network asks for it."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update, return_steps=1)
    _, m2 = _model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update)
    assert (m0.return_steps, m1.return_steps, _get_steps(m0), _get_steps(m1)) == (1, 1, 1, 1)
    rng = np.random.RandomState(11)
    size, cum, _, dones = _fill([m0, m1, m2], None, scn, E, cap, rng)
    A, B = scn.n_agent, m0.n_step
    _set_steps(m1, 1)
    _set_steps(m2, 3)
    assert _get_steps(m2) == 3
    ga, _ = _grads_at(m2, torch.from_numpy(_given_draw(rng, dones, A, B, size, cap, cum)).cuda())       # one armed step, undone below
    _reset_like(m2, m0)
    _set_steps(m2, 1)
    assert _get_steps(m2) == 1
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = torch.from_numpy(_given_draw(rng, dones, A, B, size, cap, cum)).cuda()
            (g0, s0), (g1, s1), (g2, s2) = (_grads_at(m, idx) for m in (m0, m1, m2))
            assert np.abs(g0).max() > 0 and not np.array_equal(ga, g0)
            for g, s, m in ((g1, s1, m1), (g2, s2, m2)):
                np.testing.assert_array_equal(g, g0)
                np.testing.assert_array_equal(s, s0)
                np.testing.assert_array_equal(m.get_flat(), m0.get_flat())
        assert _launches('iql_nstep') == 0
        assert _launches('iql_target') == (6 if target_update and m0.fused else 0)
        _set_steps(m2, 3)                                            # (the counter does count)
        _grads_at(m2, idx)
        assert _launches('iql_nstep') == 1
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    for m in (m0, m1, m2):
        m.close()


# ---- 2. all-terminal rings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_all_terminal_rings_give_the_one_step_update_bit_for_bit(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """done = 1 on every transition: k = 1 and y = G = r on every row, whatever n -- the unarmed step on the same draw, bit for bit:
    gradient buffer, clip norm, parameters after Adam, and the loss on the fused path.  The grouped path's loss (logging only) is a float64
    atomic sum over wavefronts whose order the hardware picks -- two launches of the SAME kernel on the same rows can differ in its last
    bit -- so there it is compared to 1e-13, far inside anything the feature could move and far outside that."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = _model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = _model(scenario, agent, model_type, E, buffer_size=cap, return_steps=3)
    assert m0.fused == m1.fused == (fused == '1') and _get_steps(m1) == 3
    rng = np.random.RandomState(cap + E)
    size, cum, rews, dones = _fill([m0, m1], None, scn, E, cap, rng, p_done=1.0)
    assert dones[:, :size].all()
    for step in range(2):
        idx = _given_draw(rng, dones, scn.n_agent, m0.n_step, size, cap, cum)
        dev = torch.from_numpy(idx).cuda()
        (g0, s0), (g1, s1) = _grads_at(m0, dev), _grads_at(m1, dev)
        assert np.abs(g0).max() > 0
        np.testing.assert_array_equal(g1, g0)
        np.testing.assert_array_equal(s1[:, 1], s0[:, 1])
        if m0.fused:
            np.testing.assert_array_equal(s1[:, 0], s0[:, 0])
        else:
            np.testing.assert_allclose(s1[:, 0], s0[:, 0], rtol=1e-13, atol=0)
        np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        slot, ret, disc, k = _nstep_debug(m1)
        np.testing.assert_array_equal(slot, idx)
        assert (k == 1).all() and (disc == np.float32(m1.cfg['gamma'])).all()
        np.testing.assert_array_equal(ret.reshape(scn.n_agent, E, -1), np.take_along_axis(rews.transpose(2, 0, 1), idx.transpose(1, 0, 2), 2))
    m0.close(); m1.close()


# ---- 3. the pre-pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', CASES)
def test_prepass_against_the_rule(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """Bootstrap slot and horizon of every row exactly; G and gamma^k exactly float32 of the float64 values of nstep_window (module
    docstring: the same operations in the same order, no contraction on either side); n = 2, 3, 32."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(2 * cap + E)
    size, cum, rews, dones = _fill([m], None, scn, E, cap, rng)
    assert m.replay_size() == (size, cum)
    gamma = float(m.cfg['gamma'])
    for n in (2, 3, 32):
        idx = _given_draw(rng, dones, scn.n_agent, m.n_step, size, cap, cum)
        slot_o, G, disc_o, k_o, s_ = _windows(idx, rews, dones, size, cap, cum, n, gamma)
        _require_categories(_categories_of(slot_o, k_o, s_, dones, cum, cap, n), cum, cap, n)
        _set_steps(m, n)
        _check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(torch.from_numpy(idx).cuda().data_ptr())))
        slot, ret, disc, k = _nstep_debug(m)
        np.testing.assert_array_equal(slot, slot_o)
        np.testing.assert_array_equal(k, k_o)
        np.testing.assert_array_equal(disc, disc_o.astype(np.float32))
        np.testing.assert_array_equal(ret, G.astype(np.float32))
    m.close()


# ---- 4. targets and gradients ----------------------------------------------------------------------------------------------------
CONFIGS = {'plain': {}, 'target': dict(target_update=100), 'double': dict(target_update=100, double_q=1),
           'per': dict(target_update=100, double_q=1, prioritized_replay=1), 'dueling': dict(dueling=1),
           'all': dict(target_update=100, double_q=1, prioritized_replay=1, dueling=1)}
BETA, LR_FIRST, LR = 0.4, 1e-8, 1e-3


def _make(scenario, agent, model_type, E, cap, n, **cfg):
    from tests.iql_nstep_oracle import NStepOracleIQL
    if cfg.get('dueling'):
        from tests.test_iql_dueling_gpu import _duel_model
        scn, m = _duel_model(scenario, E, cap, return_steps=n, **{k: v for k, v in cfg.items() if k != 'dueling'})
    else:
        scn, m = _model(scenario, agent, model_type, E, buffer_size=cap, return_steps=n, **cfg)
    assert m.return_steps == n and _get_steps(m) == n
    o = NStepOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, return_steps=n, per=bool(m.prioritized_replay),
                       alpha=m.per_alpha, eps=m.per_eps, target_update=m.target_update, double_q=bool(m.double_q), batch_size=m.n_step,
                       buffer_size=cap, gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'], reward_clip=m.cfg['reward_clip'],
                       max_grad_norm=m.cfg['max_grad_norm'], replay_seed=m.replay_seed)
    return scn, m, o


def _decided(scn, E, rng, o, dueling):
    if dueling:
        from tests.test_iql_dueling_gpu import _rand_obs_decided as _decided_duel
        return _decided_duel(scn, E, rng, o)
    return _decided_plain(scn, E, rng, o)


def _arm_target(m, o, dueling):
    if dueling:
        from tests.test_iql_dueling_gpu import _arm_disagreeing_target
        _arm_disagreeing_target(m, o)
    else:
        m.set_target_flat(m.layout.pack(_disagreeing_target(m, o)))
        o.set_target_params(m.layout.unpack(m.get_target_flat()))
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0.01


def _compare_grads(m, o, g, og, idx, params_before, rows_before):
    """tests/test_iql_target_gpu.py's gradient comparison (the kinks are those of the online net on s, the SAMPLED slot's observation)."""
    tol = 2e-5
    for a in range(m.n_agent):
        q = o.qs[a]
        saved, q.p = q.p, params_before[a]
        cols, deep = _kinks(o, [rows_before[a][e][s][0] for e in range(m.E) for s in idx[e, a]], a)
        q.p = saved
        assert set(og[a]) == set(g[a])
        for k, ref in og[a].items():
            if deep and k not in ('q_w', 'q_b', 'v_w', 'v_b'):
                continue
            got, scale = g[a][k], max(np.abs(ref).max(), 1e-9)
            err = np.abs(got - ref)
            if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                sel = cols[:m.layout.n_fc0] if k.startswith('fcw') else cols[m.layout.n_fc0:]
                err = err[..., ~sel] if err.ndim == 2 else err[~sel]
            assert err.size == 0 or err.max() <= tol * scale, 'agent %d %s: %.2e' % (a, k, err.max() / scale)


def _step_vs_oracle(scn, m, o, idx, lr, cap, gap_floor):
    """One given-draw step on the device and in the oracle, everything compared -> the device's |delta| (None without prioritized replay)."""
    from tests.iql_ext_oracle import per_weights
    from tests.test_iql_per_gpu import _expected_after, _per_debug
    A, E, B, n, per = scn.n_agent, m.E, m.n_step, m.return_steps, bool(m.prioritized_replay)
    size, cum = m.replay_size()
    params_before = [{k: v.clone() for k, v in q.p.items()} for q in o.qs]
    rows_before = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
    if per:
        before, qmax_before = m.get_priorities()
        o.prio[:], o.qmax[:] = before, qmax_before            # the weights are functions of the device's own float32 priorities
    _check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(torch.from_numpy(idx).cuda().data_ptr())))
    m.update_step += 1
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    y, astar = _targets(m)
    slot, ret, disc, k = _nstep_debug(m)
    w, td = _per_debug(m) if per else (None, None)
    stats = np.zeros((A, 2))
    _check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(lr, beta=BETA, idx_given=idx)
    np.testing.assert_array_equal(o.last_idx, idx)
    _require_categories(o.categories(), cum, cap, n)
    np.testing.assert_array_equal(slot, o.last_slot)
    np.testing.assert_array_equal(k, o.last_k)
    np.testing.assert_array_equal(disc, o.last_disc.astype(np.float32))
    np.testing.assert_array_equal(ret, o.last_G.astype(np.float32))
    for a in range(A):
        q = o.qs[a]
        dy = np.abs(y[a] - q.last_y)
        print('agent %d: max|dy| %.2e, smallest online gap %.2e' % (a, dy.max(), _gap_of(q.last_q1_online)))
        assert _gap_of(q.last_q1_online) >= gap_floor, 'agent %d: a row with undecided online argmax at its bootstrap state' % a
        assert (dy <= 2e-5 + 2.0 ** -23 * np.abs(o.last_G[a])).all(), 'agent %d: y off by %.2e' % (a, dy.max())
        if m.double_q:
            np.testing.assert_array_equal(astar[a], q.last_astar)
            assert (q.last_astar != np.argmax(q.last_q1_target, 1)).any(), 'agent %d: the online argmax is the target argmax on every row' % a
        else:
            assert (astar[a] == -1).all()
    if per:
        wr = w.reshape(A, E, B)
        assert (wr.max(2) == 1).all() and (w > 0).all() and w.min() < 0.5
        for e in range(E):
            for a in range(A):
                np.testing.assert_allclose(wr[a, e], per_weights(before[e, a], size, idx[e, a], BETA), rtol=1e-6, atol=0)
        np.testing.assert_allclose(w, o.last_w, rtol=1e-6, atol=0)
        print('max |d|delta|| %.2e' % np.abs(td - o.last_td).max())
        np.testing.assert_allclose(td, o.last_td, rtol=0, atol=2e-5)          # |delta| against the n-step target
        after, qmax = m.get_priorities()
        want, wmax, hit = _expected_after(before, qmax_before, idx, td, size, m.per_alpha, m.per_eps)      # at slot s, not at j
        np.testing.assert_allclose(after[hit], want[hit], rtol=1e-6, atol=0)
        np.testing.assert_array_equal(after[~hit], before[~hit])
        np.testing.assert_allclose(qmax, wmax, rtol=1e-6, atol=0)
    _compare_grads(m, o, g, og, idx, params_before, rows_before)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)


def _positive_priorities(m, size, rng):
    """Random priorities over four decades on the filled slots, none of them 0: with a caller's draw a slot of priority 0 takes the ring's
    largest weight on the device, which the oracle's formula does not restate (no draw of the library's own can pick such a slot)."""
    prio, qmax = m.get_priorities()
    q = (10.0 ** rng.uniform(-2, 2, prio.shape)).astype(np.float32)
    q[:, :, size:] = 0
    m.set_priorities(q, np.maximum(qmax, q.max(2)))


# (the dueling head is IQL-DNN only)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused,config',
                         [c + (k,) for c in CASES for k, v in CONFIGS.items() if c[2] == 'dqn' or not v.get('dueling')])
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, config, monkeypatch):
    """n = 3 under every option.  Prioritized replay takes two steps: the priorities written back by the first (at the SAMPLED slots, from
    |delta| against the 3-step target) are the ones the second step's weights come from.  The first of the two moves the parameters by
    an Adam step of 1e-8, so the bootstrap states, decided by GAP when they entered the rings, are still decided by GAP / 2 (more than
    twice the Q-value tolerance) at the second."""
    from tests.test_iql_per_gpu import _set_beta
    cfg = CONFIGS[config]
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m, o = _make(scenario, agent, model_type, E, cap, 3, **cfg)
    assert m.fused == (fused == '1')
    rng = np.random.RandomState(cap + E + len(config))
    size, cum, rews, dones = _fill([m], o, scn, E, cap, rng, draw_next=lambda: _decided(scn, E, rng, o, cfg.get('dueling')))
    if m.target_update:
        _arm_target(m, o, cfg.get('dueling'))
    steps = [LR]
    if m.prioritized_replay:
        _positive_priorities(m, size, rng)
        _set_beta(m, BETA)
        steps = [LR_FIRST, LR]
    for i, lr in enumerate(steps):
        idx = _given_draw(rng, dones, scn.n_agent, m.n_step, size, cap, cum)
        _step_vs_oracle(scn, m, o, idx, lr, cap, GAP if i == 0 else GAP / 2)
    m.close()


# ---- 5. another horizon on a live handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[1], CASES[2], CASES[3]])
def test_switching_the_horizon_on_a_live_handle(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """3 -> 5 -> 1 between tsc_iql_compute_grads_at calls on the same rings and the same draw: each time the oracle's targets for that n
    (a target network is armed so that tsc_iql_debug_targets also answers at n = 1; no Adam step in between: lr = 0 in the oracle)."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m, o = _make(scenario, agent, model_type, E, cap, 3, target_update=100)
    rng = np.random.RandomState(cap + E)
    size, cum, rews, dones = _fill([m], o, scn, E, cap, rng)
    _arm_target(m, o, False)
    idx = _given_draw(rng, dones, scn.n_agent, m.n_step, size, cap, cum)
    dev = torch.from_numpy(idx).cuda()
    ys = {}
    for n in (3, 5, 1):
        _set_steps(m, n)
        assert _get_steps(m) == n
        with pytest.raises(RuntimeError, match='armed handle'):       # another horizon: the last step's targets are not this one's
            _targets(m)
        _check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(dev.data_ptr())))
        y, _ = _targets(m)
        o.return_steps = n
        o.minibatch_step(0.0, idx_given=idx)
        if n > 1:
            _require_categories(o.categories(), cum, cap, n)
            slot, ret, disc, k = _nstep_debug(m)
            np.testing.assert_array_equal(slot, o.last_slot)
            np.testing.assert_array_equal(k, o.last_k)
        else:
            assert (o.last_k == 1).all()
            with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):
                _nstep_debug(m)
        for a in range(scn.n_agent):
            dy = np.abs(y[a] - o.qs[a].last_y)
            assert (dy <= 2e-5 + 2.0 ** -23 * np.abs(o.last_G[a])).all(), 'n = %d agent %d: y off by %.2e' % (n, a, dy.max())
        ys[n] = y
    assert np.abs(ys[3] - ys[5]).max() > 1e-3 and np.abs(ys[3] - ys[1]).max() > 1e-3
    m.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    scn, m = _model('small_grid', 'iqld', 'dqn', 2, buffer_size=40)
    for bad in (0, 33, -1):
        with pytest.raises(RuntimeError, match='tsc_iql_set_return_steps'):
            _set_steps(m, bad)
    assert _get_steps(m) == 1
    with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):
        _nstep_debug(m)
    _set_steps(m, 32)
    assert _get_steps(m) == 32
    with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):        # armed, but no step yet
        _nstep_debug(m)
    with pytest.raises(RuntimeError, match='armed handle'):
        _targets(m)
    m.close()
    for bad in (0, 33, 2.5, '2.5'):
        with pytest.raises(ValueError, match='return_steps'):
            _model('small_grid', 'iqld', 'dqn', 2, return_steps=bad)
    # the E = 1 adaptor arms its handle from the config too
    from deeprl_signal_control_amd.iql import IQL
    one = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20, buffer_size=40, reward_norm=100.0, return_steps=4), seed=1)
    assert one.vec.return_steps == 4 and _get_steps(one.vec) == 4
    one.vec.close()
