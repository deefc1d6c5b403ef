"""The actuated and SOTL controllers on the device (actuated_kernel, csrc/tsc_env.hip) against the plain-loop rules of
tests/actuated_rules.py over the oracle's state: in closed loop -- the device's controller chooses, the handle and the oracles step
under its actions and stay bit-equal (tests/env_harness.py follow / oracle_steps) -- actions, the per-phase counts and the controller's
state of every instance at every step, exactly.  tests/test_actuated_host.py states, on the oracle alone, that these runs take every
branch of both rules.  Nothing here has a tolerance.

No test asks for the 48 KiB refusal of tsc_env_set_actuated: the kernel needs 4 x (n_walk + 1 + 2 n_mov + 3 A x PMAX + 256) bytes,
which passes 48 KiB only with, say, 4096 movements and more than 1,200 (agent, phase) pairs at once; the largest network of
tests/networks.py, grid_x4, needs 18,196 B."""
import ctypes as C

import numpy as np
import pytest
import torch

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import VecTrafficEnv
from deeprl_signal_control_amd.scenario import build_scenario
from tests import actuated_rules as R
from tests import env_harness as H
from tests import networks as nw

pytestmark = pytest.mark.gpu
_cache = {}
RULES = {'actuated': R.GAP, 'sotl': R.SOTL}


def scenario(name):
    if name == 'real_net':
        if name not in _cache:
            _cache[name] = build_scenario('real_net', 'greedy', episode_length_sec=600)
        return _cache[name], 2000
    return nw.NETWORKS[name].scenario(), nw.NETWORKS[name].seed


def device_call(env, rule, prm, **kw):
    return env.actuated_actions(**prm, **kw) if rule == 'actuated' else env.sotl_actions(**prm, **kw)


def assert_state(env, state, msg):
    got = env.controller_state()
    for k, want in zip(('cur', 'age', 'kappa'), state):
        np.testing.assert_array_equal(got[k], want, err_msg='%s %s' % (k, msg))


def closed_loop(name, E, steps, rule, prm, state_every=7):
    """The device controller drives `steps` control steps of a handle and its oracles; at every step its actions and counts, and every
    state_every steps and at the end its state, equal the loop rule over the oracles' snapshots.  name: a registry name (scenario),
    or (scenario, seed) itself.  -> (the handle, the rule's state, the branches taken, the last counts)."""
    from oracle.env_oracle import OracleEnv
    scn, seed = scenario(name) if isinstance(name, str) else name
    tb = R.tables(scn, rule, prm)
    env = VecTrafficEnv(scn, E, seed=seed)
    orc = [OracleEnv(scn, seed=seed + e) for e in range(E)]
    env.reset()
    obs = [o.reset() for o in orc]
    state = R.initial_state(scn, E, prm['min_green'])
    took, last = {}, {}

    def draw(t, obs):
        act, cnt = device_call(env, rule, prm, return_counts=True)
        act_h, cnt_h = act.cpu().numpy(), cnt.cpu().numpy()
        for e in range(E):
            want_cnt, tk = R.rule_step(rule, scn, tb, orc[e].ms.snapshot(), state, e, prm)
            R.count_branches(took, tk)
            np.testing.assert_array_equal(cnt_h[e], want_cnt, err_msg='counts t=%d e=%d' % (t, e))
            np.testing.assert_array_equal(act_h[e], state[0][e], err_msg='action t=%d e=%d' % (t, e))
        if t % state_every == 0 or t == steps - 1:
            assert_state(env, state, 't=%d' % t)
        last['counts'] = cnt_h
        return act, None
    H.follow(env, H.oracle_steps(scn, orc, obs, steps, draw), state_at=[steps - 1])
    return env, state, took, last['counts']


@pytest.mark.parametrize('rule', ['actuated', 'sotl'])
@pytest.mark.parametrize('name,E,steps', [('grid_x2', 2, 60), ('ctrl8', 2, 60), ('link62', 3, 60), ('real_net', 2, 120), ('grid_x4', 2, 30)])
def test_closed_loop(name, E, steps, rule):
    env, state, took, _ = closed_loop(name, E, steps, rule, RULES[rule])
    env.close()
    print(name, rule, took)
    assert took.get('gap_out' if rule == 'actuated' else 'change', 0) > 0


@pytest.mark.parametrize('rule', ['actuated', 'sotl'])
def test_closed_loop_300_agents(rule):
    """isolated_300: the per-agent loop past one workgroup's threads.  The junctions' second phase serves nothing, so the action stays
    0 and the age runs alike at every junction; what differs from agent to agent, and is compared for all 300 together with the state
    at every step, is the counts (under SOTL red(0 | 0) is 0: the calls)."""
    env, (cur, age, kappa), took, counts = closed_loop('isolated_300', 2, 20, rule, RULES[rule], state_every=1)
    env.close()
    assert not cur.any() and not kappa.any()
    for e in range(2):
        assert len(set(counts[e, 256:, 0, 0].tolist())) > 1, e
        assert rule == 'sotl' or len(set(counts[e, 256:, 0, 1].tolist())) > 1, e


def test_default_parameters():
    """actuated_actions() as it stands: min_green = 1, max_green = 10, gap 3.0 s."""
    prm = dict(min_green=1, max_green=10, gap_sec=3.0)
    scn, seed = scenario('grid_x2')
    env, state, took, _ = closed_loop('grid_x2', 2, 40, 'actuated', prm)
    try:
        assert 'min_green' not in took and took.get('extension', 0) > 0 and took.get('gap_out', 0) > 0
        assert state[0].any()
        env.reset()
        assert_state(env, R.initial_state(scn, 2, 1), 'after reset()')
    finally:
        env.close()


def test_state_resets():
    """reset() and re-arming with other parameters give the initial state; reset() of one handle leaves another's alone."""
    scn, seed = scenario('ctrl8')
    E = 2
    a, b = VecTrafficEnv(scn, E, seed=seed), VecTrafficEnv(scn, E, seed=seed)
    try:
        a.reset(); b.reset()
        prm = dict(R.SOTL, theta=8)
        for t in range(25):
            act = a.sotl_actions(**prm)
            assert torch.equal(act, b.sotl_actions(**prm)), t
            a.step(act); b.step(act)
        before = b.controller_state()
        assert before['cur'].any() and before['kappa'].any() and (before['age'] != prm['min_green']).any()
        np.testing.assert_array_equal(a.controller_state()['kappa'], before['kappa'])
        a.reset()                                                       # mid-episode
        assert_state(a, R.initial_state(scn, E, prm['min_green']), 'after reset()')
        for k, v in b.controller_state().items():
            np.testing.assert_array_equal(v, before[k], err_msg='the other handle, ' + k)
        b.sotl_actions(**dict(prm, min_green=3))                        # re-arms, then one call from the initial state
        tb = R.tables(scn, 'sotl', prm)
        want = R.initial_state(scn, E, 3)
        for e in range(E):
            R.rule_step('sotl', scn, tb, b.get_state(e), want, e, dict(prm, min_green=3))
        assert_state(b, want, 'one call after re-arming')                # (nothing was left of the old state)
        b.actuated_actions(**R.GAP)                                     # the other rule re-arms too
        got = b.controller_state()
        assert not got['kappa'].any() and got['age'].max() <= R.GAP['min_green'] + 1
    finally:
        a.close(); b.close()


def test_nothing_else_moves():
    scn, seed = scenario('grid_x2')
    E = 2
    rng = np.random.RandomState(4)
    armed, plain = VecTrafficEnv(scn, E, seed=seed), VecTrafficEnv(scn, E, seed=seed)
    try:
        assert torch.equal(armed.reset(), plain.reset())

        def before(t):
            device_call(armed, 'actuated' if t < 8 else 'sotl', RULES['actuated' if t < 8 else 'sotl'], return_counts=True)
        H.lockstep([armed, plain], 16, lambda t: (H.uniform_actions(scn, rng, E), None), state_of=range(E), before=before)
        for e in range(E):
            sa, sb = armed.get_state(e), plain.get_state(e)
            for k in sa:
                assert sa[k].tobytes() == sb[k].tobytes(), (e, k)
        for x, y in zip(armed.counters(), plain.counters()):
            np.testing.assert_array_equal(x, y)
    finally:
        armed.close(); plain.close()


@pytest.mark.parametrize('rule', ['actuated', 'sotl'])
def test_independent_of_max_pressure(rule):
    """Max-pressure (min_green = 3) and the rule armed on one handle: both action streams equal those of two handles that arm one
    each, all three stepping under the rule's actions."""
    scn, seed = scenario('grid_x2')
    E, prm = 2, RULES[rule]
    both, mp, ac = (VecTrafficEnv(scn, E, seed=seed) for _ in range(3))
    try:
        for env in (both, mp, ac):
            env.reset()
        changed = 0
        for t in range(30):
            p1, a1 = both.max_pressure_actions(min_green=3), device_call(both, rule, prm)
            p2, a2 = mp.max_pressure_actions(min_green=3), device_call(ac, rule, prm)
            assert torch.equal(p1, p2) and torch.equal(a1, a2), t
            changed += int((p1 != a1).any())
            for env in (both, mp, ac):
                env.step(a1)
        assert changed > 10                                             # the two controllers do not say the same
    finally:
        for env in (both, mp, ac):
            env.close()


def raw_arm(env, tb, rule=0, g=2, G=6, theta=20, mu=2, zone=None, mov=None, lrm=None, served=None):
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    mov, lrm, served = (np.ascontiguousarray(tb[k] if x is None else x, np.int32)
                        for k, x in (('mov', mov), ('lane_route_mov', lrm), ('served', served)))
    zone = np.ascontiguousarray(tb['zone'] if zone is None else zone, np.float32)
    _lib.check(env._L.tsc_env_set_actuated(env._h, rule, g, G, theta, mu, zone.ctypes.data_as(fp), len(mov), mov.ctypes.data_as(ip),
                                           lrm.ctypes.data_as(ip), served.shape[2], served.ctypes.data_as(ip)))


def test_errors():
    """Every refusal of tsc_env_set_actuated, on an unarmed handle (nothing gets armed) and on an armed one (tables and state stay)."""
    scn, seed = scenario('ctrl8')
    tb = R.tables(scn, 'actuated', R.GAP)
    env = VecTrafficEnv(scn, 1, seed=seed)
    out = torch.zeros(1, scn.n_agent, dtype=torch.int32, device='cuda')
    hold = np.zeros((1, scn.n_agent, 2), np.int32)

    def refusals():
        for kw, text in ((dict(rule=2), 'rule 2 is neither'), (dict(rule=-1), 'rule -1 is neither'), (dict(g=0), 'min_green 0 must be >= 1'),
                         (dict(g=3, G=2), 'max_green 2 must be >= min_green 3'), (dict(rule=1, theta=0), 'theta 0 must be >= 1'),
                         (dict(rule=1, mu=-1), 'mu -1 must be >= 0')):
            with pytest.raises(RuntimeError, match=text):
                raw_arm(env, tb, **kw)
        for bad in (0.0, -1.0, np.inf, np.nan):
            zone = tb['zone'].copy(); zone[scn.n_lane - 1] = bad
            with pytest.raises(RuntimeError, match='zone of lane %d' % (scn.n_lane - 1)):
                raw_arm(env, tb, zone=zone)
        bad = tb['mov'].copy(); bad[0, 0] = scn.n_agent
        with pytest.raises(RuntimeError, match='names agent'):
            raw_arm(env, tb, mov=bad)
        bad = tb['mov'].copy(); bad[0, 2] = scn.n_lane
        with pytest.raises(RuntimeError, match='names lanes'):
            raw_arm(env, tb, mov=bad)
        bad = tb['mov'].copy(); bad[0, 3] = 63
        with pytest.raises(RuntimeError, match='signal link 63'):
            raw_arm(env, tb, mov=bad)
        bad = tb['lane_route_mov'].copy(); bad[0, 0] = len(tb['mov'])
        with pytest.raises(RuntimeError, match='names movement'):
            raw_arm(env, tb, lrm=bad)
        bad = tb['served'].copy(); bad[0, 0, 0] = len(tb['mov'])
        with pytest.raises(RuntimeError, match='serves movement'):
            raw_arm(env, tb, served=bad)
        other = int(np.nonzero(tb['mov'][:, 0] != 0)[0][0])
        bad = tb['served'].copy(); bad[0, 0, 0] = other
        with pytest.raises(RuntimeError, match="another agent's"):
            raw_arm(env, tb, served=bad)
        with pytest.raises(ValueError, match='actuated_max_green'):
            env.actuated_actions(min_green=4, max_green=3)
        with pytest.raises(ValueError, match='actuated_gap_sec'):
            env.actuated_actions(gap_sec=0.0)
        with pytest.raises(ValueError, match='sotl_theta'):
            env.sotl_actions(theta=0)
        with pytest.raises(ValueError, match='sotl_omega'):
            env.sotl_actions(omega_m=float('nan'))
    try:
        env.reset()
        refusals()
        for call in (lambda: env._L.tsc_env_actuated_actions(env._h, C.c_void_p(out.data_ptr()), None),
                     lambda: env._L.tsc_env_actuated_state(env._h, hold.ctypes.data_as(C.POINTER(C.c_int32)), None)):
            with pytest.raises(RuntimeError, match='no controller tables \\(tsc_env_set_actuated\\)'):     # a refused call armed nothing
                _lib.check(call())
        # armed, some steps in: the refusals leave tables and state as they are, and the closed loop goes on equal to the rule
        state = R.initial_state(scn, 1, R.GAP['min_green'])
        moved = []

        def steps(n):
            for _ in range(n):
                moved.append(bool(state[0].any()))
                act, cnt = env.actuated_actions(**R.GAP, return_counts=True)
                want, _ = R.rule_step('actuated', scn, tb, env.get_state(0), state, 0, R.GAP)
                np.testing.assert_array_equal(cnt.cpu().numpy()[0], want)
                np.testing.assert_array_equal(act.cpu().numpy(), state[0])
                env.step(act)
        steps(12)
        assert any(moved)
        refusals()
        assert_state(env, state, 'after the refusals')
        steps(8)
        assert_state(env, state, 'at the end')
    finally:
        env.close()


def test_more_than_32_phases_are_refused():
    phases = ['G' if p % 2 == 0 else 'r' for p in range(33)]
    scn = nw.compile_network('phases33', 'ia2c', [(150.0, 13.89, 0), (100.0, 13.89, -1)], [[[(0, 0), (1, -1)]]], [phases], [[]],
                             [(0, 100, 600, 0)], episode_length_sec=100)
    with pytest.raises(ValueError, match='33 phases per agent'):
        scn.actuated_tables('actuated', gap_sec=3.0)
    tb = dict(scn.pressure_tables(), zone=np.full(scn.n_lane, 30.0, np.float32))
    env = VecTrafficEnv(scn, 1, seed=1)
    try:
        env.reset()
        with pytest.raises(RuntimeError, match='33 phases per agent'):
            raw_arm(env, tb)
        assert (env.max_pressure_actions().cpu().numpy() == 0).all()   # (the handle works: max-pressure has no such limit)
    finally:
        env.close()
