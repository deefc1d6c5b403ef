"""The pressure reward on the device (pressure_reward_kernel behind step_kernel, csrc/tsc_env.hip; armed by objective = pressure or
VecTrafficEnv.set_reward_pressure) against the host restatement trainer.pressure_reward over VecTrafficEnv.get_state: reward,
global_reward and reward_sum, exactly -- the rule is integer arithmetic and the float64 operations of a plain loop.

Step counts and demand were chosen with the CPU oracle (oracle.env_oracle.OracleEnv, greedy control, seed 31, vehicles on the walked
lanes / min P / max P under count):
  large_grid, init_density 0.2: 713 / -111 / +2 after 8 control steps, 718 / -144 / +33 after 30 (queue: first P > 0 by step 12);
  large_grid, default demand:   72 after 60 steps -- never a second round of the flat walk, hence init_density;
  Monaco, flow_rate 325:        at most ~200 in a whole episode; flow_rate 1000: 219 after 200 steps, 373 after 240, 484 after 360;
  small_grid:                   51 / -32 / +12 after 8 steps, 170 / -147 / +28 after 40 (one round of the walk throughout).
Every case asserts these preconditions on what it actually compared."""
import ctypes as C

import numpy as np
import pytest
import torch

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import VecTrafficEnv
from deeprl_signal_control_amd.scenario import build_scenario
from deeprl_signal_control_amd.trainer import max_pressure_actions, pressure_reward
from tests import env_harness as H
from tests.env_rules import instance_sum

pytestmark = pytest.mark.gpu
_scn = {}
DENSE = dict(init_density=0.2)


def scenario(name, agent='ma2c', **kw):
    key = (name, agent, tuple(sorted(kw.items())))
    if key not in _scn:
        scn = build_scenario(name, agent, **kw)
        _scn[key] = (scn, scn.pressure_tables())
    return _scn[key]


def walked_live(tb, st):
    return int(st['n'][tb['walk']].sum())


# (scenario, agent, scenario keywords, measure, train_mode, control steps, compare every, recording)
CASES = [
    ('large_grid', 'ma2c', DENSE, 'count', True, 40, 8, False),
    ('large_grid', 'ma2c', DENSE, 'queue', False, 40, 8, False),
    ('large_grid', 'ia2c', DENSE, 'count', True, 40, 8, False),
    ('large_grid', 'greedy', DENSE, 'queue', True, 40, 8, False),
    ('real_net', 'ma2c', dict(flow_rate=1000), 'count', True, 360, 60, False),
    ('real_net', 'ma2c', dict(flow_rate=1000), 'queue', False, 360, 60, False),
    ('real_net', 'ia2c', dict(flow_rate=1000), 'queue', True, 360, 60, False),
    ('small_grid', 'ma2c', {}, 'count', True, 40, 8, False),
    ('small_grid', 'ma2c', {}, 'queue', False, 40, 8, False),
    ('large_grid', 'ma2c', dict(DENSE, car_following='krauss'), 'count', True, 40, 8, True),
]


@pytest.mark.parametrize('name,agent,kw,measure,train_mode,steps,every,record', CASES)
def test_state_parity(name, agent, kw, measure, train_mode, steps, every, record):
    scn, tb = scenario(name, agent, objective='pressure', pressure_measure=measure, **kw)
    E = 3                                                  # an instance stride error shows
    env = VecTrafficEnv(scn, E, seed=31)
    assert env.reward_pressure == measure                  # armed at construction by the objective
    if record:
        env.set_record(True)
    obs = env.reset()                                      # (in train mode: instance e runs seed 31 + e)
    env.train_mode = train_mode                            # what step() hands to tsc_env_step
    assert env.car_following()[0] == kw.get('car_following', 'idm')
    gs, compared, most_live, pmin, pmax = [], 0, 0, 0, 0
    for t in range(1, steps + 1):
        obs, reward, _, g = env.step(env.greedy_actions(obs))
        gs.append(g.cpu().numpy().copy())
        if t % every and t != steps:
            continue
        r_h = reward.cpu().numpy()
        for e in range(E):
            st = env.get_state(e)
            want_r, want_g, P = pressure_reward(scn, st, measure, train_mode=train_mode)
            np.testing.assert_array_equal(r_h[e], want_r, err_msg='t=%d e=%d' % (t, e))
            assert gs[-1][e] == want_g, (t, e)
            most_live, pmin, pmax = max(most_live, walked_live(tb, st)), min(pmin, int(P.min())), max(pmax, int(P.max()))
        compared += 1
    total = env.reward_sum()
    print('%s %s %s: %d compared steps, most vehicles on the walked lanes %d, P in [%d, %d], reward_sum %.0f'
          % (name, agent, measure, compared, most_live, pmin, pmax, total))
    if record:
        assert [row['reward'] for row in env.control_data[1]] == [float(g[1]) for g in gs]     # the control log holds the pressure g
    env.close()
    assert compared >= 5
    assert pmax > 0 and pmin < 0, (pmin, pmax)             # both signs: the absolute value matters
    assert most_live > (0 if name == 'small_grid' else 256), most_live      # a second round of the flat walk
    assert total == instance_sum(gs) and total < 0


@pytest.mark.parametrize('name,E,kw', [('large_grid', 1024, {}), ('real_net', 512, dict(flow_rate=1000))])
def test_full_device(name, E, kw):
    scn, tb = scenario(name, 'ma2c', objective='pressure', **kw)
    env = VecTrafficEnv(scn, E, seed=5)                    # the library's own workgroup choice for a full device
    obs = env.reset()
    gs = []
    for t in range(30):
        obs, reward, _, g = env.step(env.greedy_actions(obs))
        gs.append(g.clone())
    r_h, g_h = reward.cpu().numpy(), gs[-1].cpu().numpy()
    sample = sorted({0, E - 1} | {e0 + k for e0 in (8, E // 2) for k in range(7)})       # first, last, every e % 8
    assert len(sample) == 16 and {e % 8 for e in sample} == set(range(8))
    any_p = False
    for e in sample:
        want_r, want_g, P = pressure_reward(scn, env.get_state(e), 'count')
        np.testing.assert_array_equal(r_h[e], want_r, err_msg='e=%d' % e)
        assert g_h[e] == want_g, e
        any_p |= bool(P.any())
    assert any_p
    assert env.reward_sum() == instance_sum([g.cpu().numpy() for g in gs])
    env.close()


def test_leaves_everything_else_alone():
    scn, _ = scenario('large_grid', 'ma2c', **DENSE)       # objective hybrid: both handles start on the built-in reward
    E = 3
    rng = np.random.RandomState(4)
    armed, plain = VecTrafficEnv(scn, E, seed=21), VecTrafficEnv(scn, E, seed=21)
    acts = [H.upload(armed, H.uniform_actions(scn, rng, E)) for _ in range(20)]
    armed.set_reward_pressure('count')
    for env in (armed, plain):
        env.set_record(True)
    assert torch.equal(armed.reset(), plain.reset())
    differ, ga, gp = False, [], []
    for t, act in enumerate(acts[:15]):
        (oa, ra, da, gla), (ob, rb, db, glb) = armed.step(act), plain.step(act)
        assert torch.equal(oa, ob) and torch.equal(da, db), t
        differ |= not torch.equal(ra, rb)
        ga.append(gla.cpu().numpy().copy()); gp.append(glb.cpu().numpy().copy())
        for k in ('_rec_ints', '_rec_speed', '_rec_queue'):                      # tsc_env_read_record of this step
            assert getattr(armed, k).tobytes() == getattr(plain, k).tobytes(), (t, k)
        if t == 9:                                         # reset of the armed sum: it starts over on the pressure reward
            assert armed.reward_sum(reset=True) == instance_sum(ga) and plain.reward_sum() == instance_sum(gp)
    assert differ
    assert armed.reward_sum() == instance_sum(ga[10:]) and plain.reward_sum() == instance_sum(gp)
    for e in range(E):
        sa, sb = armed.get_state(e), plain.get_state(e)
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), (e, k)
    for x, y in zip(armed.counters(), plain.counters()):
        np.testing.assert_array_equal(x, y)
    # disarmed: the built-in reward again, bit for bit, and its sum starts over
    armed.set_reward_pressure(None)
    assert armed.reward_pressure is None
    gp = []
    for t, act in enumerate(acts[15:]):
        ra, rb = armed.step(act), plain.step(act)
        for x, y in zip(ra, rb):
            assert x.dtype == y.dtype and torch.equal(x, y), t
        gp.append(rb[3].cpu().numpy().copy())
    assert armed.reward_sum() == instance_sum(gp)
    armed.close(); plain.close()


def test_independent_of_the_controller():
    scn, _ = scenario('large_grid', 'ma2c', **DENSE)
    E = 3
    both, ctrl, rew = (VecTrafficEnv(scn, E, seed=9) for _ in range(3))
    both.set_reward_pressure('count')
    rew.set_reward_pressure('count')
    for env in (both, ctrl, rew):
        env.reset()
    changed = False
    for t in range(20):
        a_both = both.max_pressure_actions(measure='queue', min_green=3)
        a_ctrl = ctrl.max_pressure_actions(measure='queue', min_green=3)
        assert torch.equal(a_both, a_ctrl), t
        changed |= bool((a_both != 0).any())
        r_both, r_rew = both.step(a_both), rew.step(a_both.clone())
        ctrl.step(a_ctrl)
        for x, y in zip(r_both, r_rew):
            assert torch.equal(x, y), t
    assert changed and both.reward_sum() == rew.reward_sum() < 0
    for env in (both, ctrl, rew):
        env.close()


def test_rearm_replaces_tables():
    """Re-arming the controller and the reward on one handle, twice each: every step runs on the tables of the setting in force,
    and the pressure sum runs on across the reward's re-arming."""
    scn, tb = scenario('small_grid', 'ma2c')
    E = 2
    env = VecTrafficEnv(scn, E, seed=31)
    obs = env.reset()
    first, second = (('count', 1), 'queue'), (('queue', 2), 'count')
    gs = []
    for t in range(12):
        (c_measure, min_green), r_measure = second if 4 <= t < 8 else first
        if t % 4 == 0:
            env.set_reward_pressure(r_measure)
        _, prs = env.max_pressure_actions(measure=c_measure, min_green=min_green, return_pressure=True)    # (re-arms on a new setting)
        prs = prs.cpu().numpy()
        for e in range(E):
            _, want_p = max_pressure_actions(scn, env.get_state(e), c_measure, return_pressure=True)
            np.testing.assert_array_equal(prs[e], want_p, err_msg='t=%d e=%d' % (t, e))
        obs, reward, _, g = env.step(env.greedy_actions(obs))
        gs.append(g.cpu().numpy().copy())
        r_h = reward.cpu().numpy()
        for e in range(E):
            want_r, want_g, _ = pressure_reward(scn, env.get_state(e), r_measure)
            np.testing.assert_array_equal(r_h[e], want_r, err_msg='t=%d e=%d' % (t, e))
            np.testing.assert_array_equal(gs[-1][e], want_g, err_msg='t=%d e=%d' % (t, e))
    assert env.reward_sum() == instance_sum(gs)            # the accumulator survived both re-armings
    assert min(float(g.min()) for g in gs) < 0             # (an all-zero run would pass the rest)
    env.close()


def test_errors():
    scn, tb = scenario('small_grid', 'ma2c')
    armed, plain, never = (VecTrafficEnv(scn, 1, seed=1) for _ in range(3))
    armed.set_reward_pressure('queue')
    ip = C.POINTER(C.c_int32)
    mov, lrm = (np.ascontiguousarray(tb[k], np.int32) for k in ('mov', 'lane_route_mov'))

    def arm(env, measure, mov=mov, lrm=lrm):
        _lib.check(env._L.tsc_env_set_reward_pressure(env._h, measure, len(mov), None if mov is None else mov.ctypes.data_as(ip),
                                                      None if lrm is None else lrm.ctypes.data_as(ip)))
    for env in (armed, never):
        with pytest.raises(RuntimeError, match='tsc_env_set_reward_pressure: measure 7 is neither'):
            arm(env, 7)
        bad = mov.copy(); bad[0, 2] = scn.n_lane
        with pytest.raises(RuntimeError, match='tsc_env_set_reward_pressure: movement 0 names lanes'):
            arm(env, 0, mov=bad)
        bad = mov.copy(); bad[1, 0] = scn.n_agent
        with pytest.raises(RuntimeError, match='movement 1 names agent %d of %d' % (scn.n_agent, scn.n_agent)):
            arm(env, 0, mov=bad)
        bad = lrm.copy(); bad[int(mov[0, 1]), 0] = len(mov)
        with pytest.raises(RuntimeError, match='names movement %d of %d' % (len(mov), len(mov))):
            arm(env, 0, lrm=bad)
        with pytest.raises(RuntimeError, match='null tables with measure 0'):
            _lib.check(env._L.tsc_env_set_reward_pressure(env._h, 0, len(mov), None, None))
    with pytest.raises(ValueError, match='count \\| queue'):
        armed.set_reward_pressure('density')
    # the handles keep what they had: the queue-measure pressure reward, and the built-in reward
    obs = [env.reset() for env in (armed, plain, never)]
    negative = False
    for t in range(12):
        act = plain.greedy_actions(obs[1])
        out = [env.step(act) for env in (armed, plain, never)]
        want_r, want_g, _ = pressure_reward(scn, armed.get_state(0), 'queue')
        np.testing.assert_array_equal(out[0][1].cpu().numpy()[0], want_r, err_msg='t=%d' % t)
        assert float(out[0][3][0]) == want_g
        negative |= want_g < 0
        assert torch.equal(out[1][1], out[2][1]) and torch.equal(out[1][3], out[2][3])
        obs = [o[0] for o in out]
    assert negative and never.reward_sum() == plain.reward_sum()
    never.set_reward_pressure(None)                        # disarming what was never armed is a no-op
    assert never.reward_sum() == plain.reward_sum()
    for env in (armed, plain, never):
        env.close()
