"""The max-pressure and fixed-time controllers on the device (pressure_kernel / fixed_time_kernel, csrc/tsc_env.hip) against plain
loops written here over VecTrafficEnv.get_state: actions and the full pressure array, exactly (the rule is integer arithmetic)."""
import ctypes as C

import numpy as np
import pytest
import torch

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import VecTrafficEnv
from deeprl_signal_control_amd.scenario import build_scenario
from tests import env_harness as H
from tests.env_rules import hold_state, hold_update, loop_pressure

pytestmark = pytest.mark.gpu
_scn = {}


def scenario(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _scn:
        scn = build_scenario(name, 'greedy', **kw)
        _scn[key] = (scn, scn.pressure_tables())
    return _scn[key]


@pytest.mark.parametrize('name,E,measure,kw', [
    ('large_grid', 4, 'count', {}), ('large_grid', 4, 'queue', {}), ('real_net', 3, 'count', {}), ('real_net', 3, 'queue', {}),
    ('small_grid', 2, 'count', {}), ('small_grid', 2, 'queue', {}), ('large_grid', 4, 'count', dict(car_following='krauss'))])
def test_state_parity(name, E, measure, kw):
    scn, tb = scenario(name, **kw)
    env = VecTrafficEnv(scn, E, seed=31)
    env.reset()
    rng = np.random.RandomState(5)
    differing, negative, compared = False, False, 0
    for t in range(40):
        act, prs = env.max_pressure_actions(measure=measure, return_pressure=True)
        if t % 5 == 0 and t > 0:                          # the state after every fifth step
            act_h, prs_h = act.cpu().numpy(), prs.cpu().numpy()
            for e in range(E):
                want_act, want_prs = loop_pressure(scn, tb, env.get_state(e), measure)
                np.testing.assert_array_equal(prs_h[e], want_prs, err_msg='t=%d e=%d' % (t, e))
                np.testing.assert_array_equal(act_h[e], want_act, err_msg='t=%d e=%d' % (t, e))
                differing |= len(set(act_h[e].tolist())) > 1
            negative |= bool((prs_h < 0).any())
            compared += 1
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)) if t < 10 else act)
    print('%s %s: %d compared steps, agents differing %s, negative pressure %s, %.0f live vehicles / instance'
          % (name, measure, compared, differing, negative, env.mean_live_vehicles()))
    env.close()
    assert compared == 7 and differing and negative       # not vacuous


def test_block_indexing():
    scn, tb = scenario('large_grid')
    E = 1024
    env = VecTrafficEnv(scn, E, seed=3)
    env.reset()
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    for t in range(12):
        env.step(torch.randint(0, 5, (E, 25), generator=g, device='cuda', dtype=torch.int32))
    for measure in ('count', 'queue'):
        act, prs = env.max_pressure_actions(measure=measure, return_pressure=True)
        act, prs = act.cpu().numpy(), prs.cpu().numpy()
        for e in (0, 513, 1023):
            want_act, want_prs = loop_pressure(scn, tb, env.get_state(e), measure)
            np.testing.assert_array_equal(prs[e], want_prs, err_msg='%s e=%d' % (measure, e))
            np.testing.assert_array_equal(act[e], want_act, err_msg='%s e=%d' % (measure, e))
        assert prs.any()
    env.close()


def test_hold():
    scn, tb = scenario('large_grid')
    E, A, g = 4, 25, 3
    env = VecTrafficEnv(scn, E, seed=17)
    env.reset()
    rng = np.random.RandomState(2)
    for t in range(8):                                     # some traffic first (the hold is not armed yet)
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
    state = hold_state(E, A, g)                            # arming frees the first decision, as reset() does
    cur, age, _ = state
    t, n_changes = 0, 0
    while t < 30 or not ((age < g) & (cur != 0)).any():
        assert t < 60, 'no agent inside a hold on a phase other than 0'
        act = env.max_pressure_actions(min_green=g)
        act_h = act.cpu().numpy()
        for e in range(E):
            p_star, _ = loop_pressure(scn, tb, env.get_state(e), 'count')
            n_changes += hold_update(state, e, p_star, t, g)
        np.testing.assert_array_equal(act_h, cur, err_msg='t=%d' % t)
        env.step(act)
        t += 1
    assert n_changes > 10
    # reset() frees the first decision: agents inside a hold on another phase take the empty network's argmax, phase 0
    env.reset()
    act = env.max_pressure_actions(min_green=g).cpu().numpy()
    assert (act == 0).all()
    env.step(torch.from_numpy(act).cuda())
    env.close()


@pytest.mark.parametrize('s', [1, 4])
def test_fixed_time(s):
    scn, _ = scenario('real_net')
    assert len(set(scn.agent_nphase.tolist())) > 1         # heterogeneous phase counts
    E = 2
    env = VecTrafficEnv(scn, E, seed=9)
    for episode in range(2):                               # ... after a reset too
        env.reset()
        for t in range(11):
            act = env.fixed_time_actions(s)
            want = np.tile((t // s) % np.asarray(scn.agent_nphase), (E, 1))
            np.testing.assert_array_equal(act.cpu().numpy(), want, err_msg='episode %d t=%d' % (episode, t))
            env.step(act)
    env.close()


def test_nothing_else_moves():
    scn, _ = scenario('large_grid')
    E = 3
    rng = np.random.RandomState(4)
    armed, plain = VecTrafficEnv(scn, E, seed=21), VecTrafficEnv(scn, E, seed=21)
    acts = [H.upload(armed, H.uniform_actions(scn, rng, E)) for _ in range(15)]
    oa, ob = armed.reset(), plain.reset()
    assert torch.equal(oa, ob)
    for t, act in enumerate(acts):
        armed.max_pressure_actions(min_green=3, return_pressure=True)
        armed.max_pressure_actions(measure='queue')
        armed.fixed_time_actions(2)
        ra, rb = armed.step(act), plain.step(act)
        for x, y in zip(ra, rb):
            assert x.dtype == y.dtype and torch.equal(x, y), t
        assert torch.equal(armed.greedy_actions(ra[0]), plain.greedy_actions(rb[0]))
    for e in range(E):
        sa, sb = armed.get_state(e), plain.get_state(e)
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), (e, k)
    for x, y in zip(armed.counters(), plain.counters()):
        np.testing.assert_array_equal(x, y)
    armed.close(); plain.close()


def test_errors():
    scn, tb = scenario('small_grid')
    env = VecTrafficEnv(scn, 1, seed=1)
    env.reset()
    out = torch.zeros(1, scn.n_agent, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='no controller tables \\(tsc_env_set_pressure\\)'):
        _lib.check(env._L.tsc_env_pressure_actions(env._h, C.c_void_p(out.data_ptr()), None))
    ip = C.POINTER(C.c_int32)
    mov, lrm, served = (np.ascontiguousarray(tb[k], np.int32) for k in ('mov', 'lane_route_mov', 'served'))

    def arm(measure, min_green, mov=mov, lrm=lrm, served=served):
        _lib.check(env._L.tsc_env_set_pressure(env._h, measure, min_green, len(mov), mov.ctypes.data_as(ip), lrm.ctypes.data_as(ip),
                                               served.shape[2], served.ctypes.data_as(ip)))
    with pytest.raises(RuntimeError, match='measure 7 is neither'):
        arm(7, 1)
    with pytest.raises(RuntimeError, match='min_green 0 must be >= 1'):
        arm(0, 0)
    bad = mov.copy(); bad[0, 2] = scn.n_lane
    with pytest.raises(RuntimeError, match='names lanes'):
        arm(0, 1, mov=bad)
    bad = mov.copy(); bad[0, 3] = 63
    with pytest.raises(RuntimeError, match='signal link 63'):
        arm(0, 1, mov=bad)
    bad = served.copy(); bad[0, 0, 0] = len(mov)
    with pytest.raises(RuntimeError, match='serves movement'):
        arm(0, 1, served=bad)
    with pytest.raises(RuntimeError, match='no controller tables'):          # a refused call armed nothing
        _lib.check(env._L.tsc_env_pressure_actions(env._h, C.c_void_p(out.data_ptr()), None))
    with pytest.raises(ValueError, match='count \\| queue'):
        env.max_pressure_actions(measure='density')
    with pytest.raises(ValueError, match='pressure_min_green'):
        env.max_pressure_actions(min_green=0)
    with pytest.raises(RuntimeError, match='steps_per_phase 0'):
        env.fixed_time_actions(0)
    assert (env.max_pressure_actions().cpu().numpy() == 0).all()              # and the handle still works
    env.close()
