"""GPU tests of the opt-in multi-step returns of the Q-learners ([MODEL_CONFIG] return_steps; include/tsc.h tsc_iql_set_return_steps;
csrc/tsc_iql.hip iql_nstep_kernel and, on the grouped-GEMM path, iql_gather_kernel's bootstrap slot / return and iql_td_kernel's per-row
discount; csrc/tsc_iql_fused.h iql_fused_target_kernel<.., QNStep>) against the float64 restatement of tests/iql_ext_oracle.py (return_steps).

Shapes: tests/iql_harness.py::CASES, for the reasons given there.  The rings are filled by its fill (done at probability 0.1) past their
capacity -- cap + 7 adds, so the newest slot w = 6 sits mid-ring -- except the IQL-LR ring of 1000 slots, which takes 45 adds: the
size < cap branch, where no window can wrap.  With force_terminal: the fourth-newest transition is made terminal in every instance that
would otherwise keep no terminal slot, so that EVERY ring has one to draw.

Draws are the caller's (tsc_iql_compute_grads_at).  Every (instance, agent) draws w, w - 1, cap - 1 when the ring has wrapped, one slot
whose own done flag is set, and distinct random slots besides.  Before anything is compared the oracle's windows must show, among every
agent's rows: a full horizon (k = n), a window ended by done, a window ended by the newest slot, and -- where the ring has wrapped -- a
window that crossed cap - 1 -> 0.  These are conditions on the test's own inputs, not tolerances.  A full horizon cannot exist for n = 32
on these rings (22 to 64 slots; in the unfilled ring an episode of 32 steps without an end is a 3 % event), so n = 32 is held to the
other three.

Tolerances are the project's: the pre-pass outputs are exact (slot, k; G and gamma^k are one float32 rounding of the float64 value the
oracle forms with the same operations in the same order -- the build forbids contraction, so no fused multiply-add enters the device's
loop); y within 2e-5 + 2^-23 |G| per row (the Q-value tolerance of tests/test_iql_gpu.py scaled by gamma^k <= 1, plus the one rounding of
G); a* exact on every row; loss and clip norm rtol 1e-4; gradients within 2e-5 max|g| per tensor with the ReLU-kink exception of kinks;
|delta| within 2e-5 and weights / written-back priorities rtol 1e-6 as in tests/test_iql_per_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import iql_harness as H
from tests.iql_harness import CASES, GAP
from tests.iql_ext_oracle import nstep_window

pytestmark = pytest.mark.gpu


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


# ---- 1. a disarmed handle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target_update', [0, 100])
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [CASES[0], CASES[2]])
def test_disarmed_is_untouched(scenario, agent, model_type, E, cap, fused, target_update, monkeypatch):
    """return_steps = 1 in the config, and a handle armed with 3, stepped once and set back to 1: gradient buffer, loss, clip norm and the
    parameters after Adam of a handle that never heard of the option, bit for bit over two steps; no launch of the pre-pass from any of
    them, and no launch of the target kernel either unless a target network asks for it."""
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update, return_steps=1)
    _, m2 = H.model(scenario, agent, model_type, E, buffer_size=cap, target_update=target_update)
    assert (m0.return_steps, m1.return_steps, H.get_steps(m0), H.get_steps(m1)) == (1, 1, 1, 1)
    rng = np.random.RandomState(11)
    size, cum, _, dones = H.fill([m0, m1, m2], None, scn, E, cap, rng, force_terminal=True)
    A, B = scn.n_agent, m0.n_step
    H.set_steps(m1, 1)
    H.set_steps(m2, 3)
    assert H.get_steps(m2) == 3
    ga, _ = H.grads_at(m2, torch.from_numpy(_given_draw(rng, dones, A, B, size, cap, cum)).cuda())       # one armed step, undone below
    H.reset_like(m2, m0)
    H.set_steps(m2, 1)
    assert H.get_steps(m2) == 1
    _lib.profile(enable=True)
    _lib.profile(reset=True)
    try:
        for step in range(2):
            idx = torch.from_numpy(_given_draw(rng, dones, A, B, size, cap, cum)).cuda()
            (g0, s0), (g1, s1), (g2, s2) = (H.grads_at(m, idx) for m in (m0, m1, m2))
            assert np.abs(g0).max() > 0 and not np.array_equal(ga, g0)
            for g, s, m in ((g1, s1, m1), (g2, s2, m2)):
                np.testing.assert_array_equal(g, g0)
                np.testing.assert_array_equal(s, s0)
                np.testing.assert_array_equal(m.get_flat(), m0.get_flat())
        assert H.launches('iql_nstep') == 0
        assert H.launches('iql_target') == (6 if target_update and m0.fused else 0)
        H.set_steps(m2, 3)                                            # (the counter does count)
        H.grads_at(m2, idx)
        assert H.launches('iql_nstep') == 1
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
    scn, m0 = H.model(scenario, agent, model_type, E, buffer_size=cap)
    _, m1 = H.model(scenario, agent, model_type, E, buffer_size=cap, return_steps=3)
    assert m0.fused == m1.fused == (fused == '1') and H.get_steps(m1) == 3
    rng = np.random.RandomState(cap + E)
    size, cum, rews, dones = H.fill([m0, m1], None, scn, E, cap, rng, p_done=1.0, force_terminal=True)
    assert dones[:, :size].all()
    for step in range(2):
        idx = _given_draw(rng, dones, scn.n_agent, m0.n_step, size, cap, cum)
        dev = torch.from_numpy(idx).cuda()
        (g0, s0), (g1, s1) = H.grads_at(m0, dev), H.grads_at(m1, dev)
        assert np.abs(g0).max() > 0
        np.testing.assert_array_equal(g1, g0)
        np.testing.assert_array_equal(s1[:, 1], s0[:, 1])
        if m0.fused:
            np.testing.assert_array_equal(s1[:, 0], s0[:, 0])
        else:
            np.testing.assert_allclose(s1[:, 0], s0[:, 0], rtol=1e-13, atol=0)
        np.testing.assert_array_equal(m1.get_flat(), m0.get_flat())
        slot, ret, disc, k = H.nstep_debug(m1)
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
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap)
    rng = np.random.RandomState(2 * cap + E)
    size, cum, rews, dones = H.fill([m], None, scn, E, cap, rng, force_terminal=True)
    assert m.replay_size() == (size, cum)
    gamma = float(m.cfg['gamma'])
    for n in (2, 3, 32):
        idx = _given_draw(rng, dones, scn.n_agent, m.n_step, size, cap, cum)
        slot_o, G, disc_o, k_o, s_ = _windows(idx, rews, dones, size, cap, cum, n, gamma)
        _require_categories(_categories_of(slot_o, k_o, s_, dones, cum, cap, n), cum, cap, n)
        H.set_steps(m, n)
        H.check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(torch.from_numpy(idx).cuda().data_ptr())))
        slot, ret, disc, k = H.nstep_debug(m)
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
    if cfg.get('dueling'):
        scn, m = H.duel_model(scenario, E, cap, return_steps=n, **{k: v for k, v in cfg.items() if k != 'dueling'})
    else:
        scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap, return_steps=n, **cfg)
    assert m.return_steps == n and H.get_steps(m) == n
    return scn, m, H.oracle_for(m)


def _step_vs_oracle(scn, m, o, idx, lr, cap, gap_floor):
    """One given-draw step on the device and in the oracle, everything compared."""
    A, n, per = scn.n_agent, m.return_steps, bool(m.prioritized_replay)
    size, cum = m.replay_size()
    params_before, rows_before = H.snapshot(o)
    if per:
        before, qmax_before = m.get_priorities()
        o.prio[:], o.qmax[:] = before, qmax_before            # the weights are functions of the device's own float32 priorities
    H.check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(torch.from_numpy(idx).cuda().data_ptr())))
    m.update_step += 1
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    y, astar = H.targets(m)
    slot, ret, disc, k = H.nstep_debug(m)
    w, td = H.per_debug(m) if per else (None, None)
    stats = np.zeros((A, 2))
    H.check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(lr, beta=BETA, idx_given=idx)
    np.testing.assert_array_equal(o.last_idx, idx)
    _require_categories(o.categories(), cum, cap, n)
    np.testing.assert_array_equal(slot, o.last_slot)
    np.testing.assert_array_equal(k, o.last_k)
    np.testing.assert_array_equal(disc, o.last_disc.astype(np.float32))
    np.testing.assert_array_equal(ret, o.last_G.astype(np.float32))
    # y: the Q-value tolerance scaled by gamma^k <= 1, plus the one rounding of G (module docstring)
    H.check_targets(m, o, y, astar, gap_floor, ytol=lambda a: 2e-5 + 2.0 ** -23 * np.abs(o.last_G[a]))
    if per:
        H.check_weights(w, td, o, before, size, idx, BETA)                     # |delta| against the n-step target
        H.check_write_back(m, before, qmax_before, idx, td, size)              # at slot s, not at j
    H.compare_grads(m, o, g, og, idx, params_before, rows_before)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)


# (the dueling head is IQL-DNN only)
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused,config',
                         [c + (k,) for c in CASES for k, v in CONFIGS.items() if c[2] == 'dqn' or not v.get('dueling')])
def test_targets_and_gradient_against_the_oracle(scenario, agent, model_type, E, cap, fused, config, monkeypatch):
    """n = 3 under every option.  Prioritized replay takes two steps: the priorities written back by the first (at the SAMPLED slots, from
    |delta| against the 3-step target) are the ones the second step's weights come from.  The first of the two moves the parameters by
    an Adam step of 1e-8, so the bootstrap states, decided by GAP when they entered the rings, are still decided by GAP / 2 (more than
    twice the Q-value tolerance) at the second."""
    cfg = CONFIGS[config]
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m, o = _make(scenario, agent, model_type, E, cap, 3, **cfg)
    assert m.fused == (fused == '1')
    rng = np.random.RandomState(cap + E + len(config))
    size, cum, rews, dones = H.fill([m], o, scn, E, cap, rng, draw_next=lambda: H.rand_obs_decided(scn, E, rng, o), force_terminal=True)
    if m.target_update:
        H.arm_disagreeing_target(m, o)
    steps = [LR]
    if m.prioritized_replay:
        H.positive_priorities(m, size, rng)
        H.set_beta(m, BETA)
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
    size, cum, rews, dones = H.fill([m], o, scn, E, cap, rng, force_terminal=True)
    H.arm_disagreeing_target(m, o)
    idx = _given_draw(rng, dones, scn.n_agent, m.n_step, size, cap, cum)
    dev = torch.from_numpy(idx).cuda()
    ys = {}
    for n in (3, 5, 1):
        H.set_steps(m, n)
        assert H.get_steps(m) == n
        with pytest.raises(RuntimeError, match='armed handle'):       # another horizon: the last step's targets are not this one's
            H.targets(m)
        H.check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(dev.data_ptr())))
        y, _ = H.targets(m)
        o.return_steps = n
        o.minibatch_step(0.0, idx_given=idx)
        if n > 1:
            _require_categories(o.categories(), cum, cap, n)
            slot, ret, disc, k = H.nstep_debug(m)
            np.testing.assert_array_equal(slot, o.last_slot)
            np.testing.assert_array_equal(k, o.last_k)
        else:
            assert (o.last_k == 1).all()
            with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):
                H.nstep_debug(m)
        for a in range(scn.n_agent):
            dy = np.abs(y[a] - o.qs[a].last_y)
            assert (dy <= 2e-5 + 2.0 ** -23 * np.abs(o.last_G[a])).all(), 'n = %d agent %d: y off by %.2e' % (n, a, dy.max())
        ys[n] = y
    assert np.abs(ys[3] - ys[5]).max() > 1e-3 and np.abs(ys[3] - ys[1]).max() > 1e-3
    m.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    scn, m = H.model('small_grid', 'iqld', 'dqn', 2, buffer_size=40)
    for bad in (0, 33, -1):
        with pytest.raises(RuntimeError, match='tsc_iql_set_return_steps'):
            H.set_steps(m, bad)
    assert H.get_steps(m) == 1
    with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):
        H.nstep_debug(m)
    H.set_steps(m, 32)
    assert H.get_steps(m) == 32
    with pytest.raises(RuntimeError, match='tsc_iql_debug_nstep'):        # armed, but no step yet
        H.nstep_debug(m)
    with pytest.raises(RuntimeError, match='armed handle'):
        H.targets(m)
    m.close()
    for bad in (0, 33, 2.5, '2.5'):
        with pytest.raises(ValueError, match='return_steps'):
            H.model('small_grid', 'iqld', 'dqn', 2, return_steps=bad)
    # the E = 1 adaptor arms its handle from the config too
    from deeprl_signal_control_amd.iql import IQL
    one = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20, buffer_size=40, reward_norm=100.0, return_steps=4), seed=1)
    assert one.vec.return_steps == 4 and H.get_steps(one.vec) == 4
    one.vec.close()
