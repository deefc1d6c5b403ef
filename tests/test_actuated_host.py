"""Host side of the actuated and SOTL controllers (no GPU): the host restatements trainer.actuated_actions / trainer.sotl_actions
against the plain-loop rules of tests/actuated_rules.py on hand-made states that take every branch, the edges of the rules (the zone's
boundary in float32, wrong-lane vehicles, the skip and its wrap-around, the first maximum of kappa, red against the current phase),
phase_mask against served, the config keys, the CLI refusals and the ABI list; then, on the oracle alone, how often the closed-loop
cases of tests/test_actuated_gpu.py take every branch.  Everything is integer arithmetic and one float32 compare: equality is exact."""
import os

import numpy as np
import pytest

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import CONTROLLERS, actuated_kw, controller_kw
from deeprl_signal_control_amd.scenario import LANE_CAP, build_scenario
from deeprl_signal_control_amd.trainer import actuated_actions, sotl_actions
from tests import actuated_rules as R
from tests import networks as nw
from tests.test_pressure_host import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = dict(min_green=2, max_green=4, gap_sec=3.0)
SOTL = dict(min_green=2, theta=5, mu=1, omega_m=25.0)
_cache = {}


def grid():
    """large_grid, its two table sets and the movements of agent 0 by the phases that serve them (five phases; movements served by
    phase 0 alone, by {2, 4}, by {2, 3}, by {1, 2, 3} and by {1, 4})."""
    if 'grid' not in _cache:
        scn = build_scenario('large_grid', 'greedy')
        tg, ts = R.tables(scn, 'actuated', GAP), R.tables(scn, 'sotl', SOTL)
        by_mask = {}
        for i in range(len(tg['mov'])):
            if tg['mov'][i, 0] == 0:
                by_mask.setdefault(int(tg['phase_mask'][i]), i)
        _cache['grid'] = (scn, tg, ts, by_mask)
    return _cache['grid']


def state(scn, tb, vehicles):
    """A vehicle state from (movement, distance to the lane's end) pairs; a movement given as (lane, route) is taken as it is."""
    NL = scn.n_lane
    st = dict(n=np.zeros(NL, np.int32), x=np.zeros((NL, LANE_CAP), np.float32), v=np.zeros((NL, LANE_CAP), np.float32),
              sf=np.zeros((NL, LANE_CAP), np.float32), w=np.zeros((NL, LANE_CAP), np.int32), r=np.zeros((NL, LANE_CAP), np.int32))
    for mv, dist in vehicles:
        if isinstance(mv, tuple):
            l, r = mv
        else:
            l = int(tb['mov'][mv, 1])
            r = int(np.nonzero(tb['lane_route_mov'][l] == mv)[0][0])
        k = st['n'][l]
        st['x'][l, k], st['r'][l, k] = np.float32(np.float64(scn.lane_len[l]) - np.float64(dist)), r
        st['n'][l] += 1
    return st


def both_gap(scn, tb, st, cur0, age0, prm=GAP):
    """One call of the gap rule at agent 0 in (cur0, age0), the others freshly reset: trainer == loop -> (cur, age, branch of agent 0)."""
    cur, age = np.zeros(scn.n_agent, np.int32), np.full(scn.n_agent, prm['min_green'], np.int32)
    cur[0], age[0] = cur0, age0
    act, c2, a2, cnt = actuated_actions(scn, st, cur, age, return_counts=True, **prm)
    want_cnt, took = R.gap_step(scn, tb, st, cur, age, **prm)            # (updates cur and age in place)
    np.testing.assert_array_equal(cnt, want_cnt)
    np.testing.assert_array_equal(act, cur); np.testing.assert_array_equal(c2, cur); np.testing.assert_array_equal(a2, age)
    return int(cur[0]), int(age[0]), took[0], cnt[0]


def both_sotl(scn, tb, st, cur0, age0, kappa0, prm=SOTL):
    cur, age = np.zeros(scn.n_agent, np.int32), np.full(scn.n_agent, prm['min_green'], np.int32)
    kappa = np.zeros((scn.n_agent, tb['n_served'].shape[1]), np.int32)
    cur[0], age[0], kappa[0, :len(kappa0)] = cur0, age0, kappa0
    act, c2, a2, k2, cnt = sotl_actions(scn, st, cur, age, kappa, return_counts=True, **prm)
    want_cnt, took = R.sotl_step(scn, tb, st, cur, age, kappa, **prm)
    np.testing.assert_array_equal(cnt, want_cnt)
    np.testing.assert_array_equal(act, cur); np.testing.assert_array_equal(c2, cur); np.testing.assert_array_equal(a2, age)
    np.testing.assert_array_equal(k2, kappa)
    return int(cur[0]), int(age[0]), took[0], kappa[0].tolist(), cnt[0]


def test_phase_mask_against_served():
    for scn in (grid()[0], build_scenario('real_net', 'greedy'), nw.NETWORKS['link62'].scenario()):
        tb = scn.actuated_tables('sotl', omega_m=25.0)
        assert tb['phase_mask'].dtype == np.uint32 and tb['zone'].dtype == np.float32
        for i, (a, l, _m, _k) in enumerate(tb['mov'].tolist()):
            want = 0
            for p in range(tb['served'].shape[1]):
                if i in tb['served'][a, p, :tb['n_served'][a, p]].tolist():
                    want |= 1 << p
            assert int(tb['phase_mask'][i]) == want and want > 0, i
        assert tb['walk_in'].tolist() == sorted(set(tb['mov'][:, 1].tolist())) and len(tb['walk_in']) < len(tb['walk'])
        assert (tb['zone'] == np.float32(25.0)).all()
        zg = scn.actuated_tables('actuated', gap_sec=3.0)['zone']
        np.testing.assert_array_equal(zg, np.float32(3.0) * np.asarray(scn.lane_vmax, np.float32))
    with pytest.raises(ValueError, match='actuated \\| sotl'):
        scn.actuated_tables('gap', gap_sec=3.0)
    for bad in (None, 0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='gap_sec'):
            scn.actuated_tables('actuated', gap_sec=bad)
        with pytest.raises(ValueError, match='omega_m'):
            scn.actuated_tables('sotl', omega_m=bad)


def test_gap_rule_every_branch():
    scn, tb, _, m = grid()
    m0, m24, m23, m123, m14 = m[0b1], m[0b10100], m[0b1100], m[0b1110], m[0b10010]
    far, near = 70.0, 10.0
    # min-green hold: whatever waits
    assert both_gap(scn, tb, state(scn, tb, [(m14, near)]), 0, 1)[:3] == (0, 2, ['min_green'])
    # extension: a vehicle within the gap on the current phase, age < max_green
    assert both_gap(scn, tb, state(scn, tb, [(m0, near), (m14, near)]), 0, 2)[:3] == (0, 3, ['extension'])
    assert both_gap(scn, tb, state(scn, tb, [(m0, near), (m14, near)]), 0, 3)[:3] == (0, 4, ['extension'])
    # forced change at max_green although the current phase still calls
    assert both_gap(scn, tb, state(scn, tb, [(m0, near), (m14, far)]), 0, 4)[:3] == (1, 1, ['forced'])
    # ... without demand elsewhere the phase stays, age saturated at max_green
    assert both_gap(scn, tb, state(scn, tb, [(m0, near)]), 0, 4)[:3] == (0, 4, ['no_demand'])
    # gap-out: the current phase's vehicles are all beyond the zone
    assert both_gap(scn, tb, state(scn, tb, [(m0, far), (m14, far)]), 0, 2)[:3] == (1, 1, ['gap_out'])
    # the skip goes over the empty phase 1 (m24 is served by 2 and 4: the first of them) ...
    assert both_gap(scn, tb, state(scn, tb, [(m24, far)]), 0, 2)[:3] == (2, 1, ['gap_out', 'skip'])
    # ... and wraps around: from phase 3 over the empty 4 to 0; from 4 to 0 is no skip
    assert both_gap(scn, tb, state(scn, tb, [(m0, far)]), 3, 2)[:3] == (0, 1, ['gap_out', 'skip'])
    assert both_gap(scn, tb, state(scn, tb, [(m0, far)]), 4, 2)[:3] == (0, 1, ['gap_out'])
    assert both_gap(scn, tb, state(scn, tb, [(m23, far)]), 4, 2)[:3] == (2, 1, ['gap_out', 'skip'])
    # demand on the current phase alone is none to change to
    assert both_gap(scn, tb, state(scn, tb, [(m0, far)]), 0, 2)[:3] == (0, 3, ['no_demand'])
    assert both_gap(scn, tb, state(scn, tb, []), 2, 3)[:3] == (2, 4, ['no_demand'])
    # the counts: call counts the near vehicles, dem all of them, per phase over what it serves
    cnt = both_gap(scn, tb, state(scn, tb, [(m123, near), (m123, far), (m14, far), (m0, near)]), 0, 1)[3]
    assert cnt[:, 0].tolist() == [1, 1, 1, 1, 0] and cnt[:, 1].tolist() == [1, 3, 2, 2, 1]


def test_sotl_every_branch():
    scn, _, tb, m = grid()
    m0, m24, m23, m123, m14 = m[0b1], m[0b10100], m[0b1100], m[0b1110], m[0b10010]
    far, near = 70.0, 10.0
    # min-green hold: kappa is integrated all the same, and kappa[cur] stays 0
    cur, age, took, kappa, cnt = both_sotl(scn, tb, state(scn, tb, [(m14, far)] * 6), 0, 1, [3, 0, 0, 0, 0])
    assert (cur, age, took, kappa) == (0, 2, ['min_green'], [0, 6, 0, 0, 6])
    # a platoon of 1 <= mu near the stop line is not cut, whatever kappa says
    cur, age, took, kappa, _ = both_sotl(scn, tb, state(scn, tb, [(m0, near), (m14, far)]), 0, 5, [0, 9, 0, 0, 0])
    assert (cur, age, took, kappa) == (0, 6, ['platoon'], [0, 10, 0, 0, 10 - 9])
    # two near vehicles > mu are cut: the threshold decides; the FIRST maximum of kappa (1 and 4 tie at 5) wins and is zeroed
    cur, age, took, kappa, _ = both_sotl(scn, tb, state(scn, tb, [(m0, near), (m0, near), (m14, far)]), 0, 5, [0, 4, 0, 0, 4])
    assert (cur, age, took, kappa) == (1, 1, ['change'], [0, 0, 0, 0, 5])
    # ... a later, larger one wins over an earlier one
    cur, age, took, kappa, _ = both_sotl(scn, tb, state(scn, tb, [(m14, far)]), 0, 2, [0, 4, 0, 0, 6])
    assert (cur, age, took, kappa) == (4, 1, ['change'], [0, 5, 0, 0, 0])
    # below the threshold
    cur, age, took, kappa, _ = both_sotl(scn, tb, state(scn, tb, [(m14, far)]), 0, 2, [0, 3, 0, 0, 2])
    assert (cur, age, took, kappa) == (0, 3, ['below'], [0, 4, 0, 0, 3])
    # red excludes the movements the current phase serves too: under phase 2, m23 and m123 add nothing to phases 1 and 3, m24
    # nothing to 4; m14 counts for 1 and 4, m0 for 0
    cur, age, took, kappa, cnt = both_sotl(scn, tb, state(scn, tb, [(m23, far), (m123, far), (m24, far), (m14, far), (m0, far), (m0, far)]),
                                           2, 1, [0, 0, 0, 0, 0])
    assert cnt[:, 1].tolist() == [2, 1, 0, 0, 1] and kappa == [2, 1, 0, 0, 1] and (cur, age, took) == (2, 2, ['min_green'])
    # age saturates at 2^30
    assert both_sotl(scn, tb, state(scn, tb, []), 0, 1 << 30, [0] * 5)[:3] == (0, 1 << 30, ['below'])
    # a phase that serves nothing is never taken: isolated junctions have two phases, the second one empty
    one = nw.isolated(2)
    assert one.agent_nphase.tolist() == [2, 2]
    t1 = R.tables(one, 'sotl', SOTL)
    st = state(one, t1, [(0, far)] * 8)
    cur, age, kappa = np.zeros(2, np.int32), np.full(2, 5, np.int32), np.zeros((2, 2), np.int32)
    act, c2, a2, k2 = sotl_actions(one, st, cur, age, kappa, **SOTL)
    assert act.tolist() == [0, 0] and a2.tolist() == [6, 6] and not k2.any()


def test_zone_boundary_in_float32():
    scn, tb, ts, m = grid()
    mv = m[0b10100]                                                        # served by phase 2: call(2) is what is read
    l = int(tb['mov'][mv, 1])
    L, zone, inf = np.float32(scn.lane_len[l]), tb['zone'][l], np.float32(np.inf)
    assert (L, zone, ts['zone'][l]) == (np.float32(75.0), np.float32(60.0), np.float32(25.0))
    call = lambda st: int(both_gap(scn, tb, st, 2, 2)[3][2, 0])
    assert call(state(scn, tb, [(mv, float(zone))])) == 1                  # L - x == zone calls
    beyond = np.nextafter(zone, inf)                                       # one ulp of the difference farther does not
    st = state(scn, tb, [(mv, float(beyond))])
    assert np.float32(L - st['x'][l, 0]) == beyond and call(st) == 0
    # one ulp of x farther is less than half an ulp of the difference: float32(L - x) rounds back onto the zone and calls, where
    # float64 arithmetic would not
    st = state(scn, tb, [(mv, float(zone))])
    st['x'][l, 0] = np.nextafter(st['x'][l, 0], -inf)
    assert np.float64(L) - np.float64(st['x'][l, 0]) > np.float64(zone) and np.float32(L - st['x'][l, 0]) == zone
    assert call(st) == 1
    # SOTL's zone is omega metres on every lane (x near 50 m has half the resolution of the difference: two ulps farther)
    near = lambda st: int(both_sotl(scn, ts, st, 0, 1, [0] * 5)[4][2, 0])
    assert near(state(scn, ts, [(mv, 25.0)])) == 1
    beyond = np.nextafter(np.nextafter(np.float32(25.0), inf), inf)
    st = state(scn, ts, [(mv, float(beyond))])
    assert np.float32(L - st['x'][l, 0]) == beyond and near(st) == 0


def test_wrong_lane_vehicle_calls_nothing():
    scn, tb, ts, m = grid()
    lanes = sorted({int(tb['mov'][i, 1]) for i in range(len(tb['mov'])) if tb['mov'][i, 0] == 0})      # agent 0's incoming lanes
    wrong = [(l, r) for l in lanes for r in range(scn.n_route) if tb['lane_route_mov'][l, r] < 0]
    assert wrong, 'every route of the lanes %r takes a movement' % lanes
    st = state(scn, tb, [(wrong[0], 5.0)] * 3)
    cur, age, took, cnt = both_gap(scn, tb, st, 0, 2)
    assert not cnt.any() and took == ['no_demand']
    cur, age, took, kappa, cnt = both_sotl(scn, ts, st, 1, 2, [0] * 5)
    assert not cnt.any() and not any(kappa) and took == ['below']


def test_host_restatements_refuse_device_tensors():
    import torch
    scn, tb, _, _ = grid()
    st = {k: torch.from_numpy(v) for k, v in state(scn, tb, []).items()}
    z = np.zeros(scn.n_agent, np.int32)
    with pytest.raises(TypeError, match='host restatement'):
        actuated_actions(scn, st, z, z)
    with pytest.raises(TypeError, match='host restatement'):
        sotl_actions(scn, st, z, z, np.zeros((scn.n_agent, 5), np.int32))


def test_config_keys():
    defaults = dict(actuated_min_green=1, actuated_max_green=10, actuated_gap_sec=3.0, sotl_min_green=2, sotl_theta=20, sotl_mu=2,
                    sotl_omega=25.0)
    assert actuated_kw({}) == defaults
    assert actuated_kw(dict(actuated_min_green=' 2 ', actuated_max_green='6', actuated_gap_sec='2.5', sotl_min_green='3', sotl_theta='40',
                            sotl_mu='0', sotl_omega='30')) == \
        dict(actuated_min_green=2, actuated_max_green=6, actuated_gap_sec=2.5, sotl_min_green=3, sotl_theta=40, sotl_mu=0, sotl_omega=30.0)
    for key in ('actuated_min_green', 'actuated_max_green', 'sotl_min_green', 'sotl_theta'):
        for bad in ('0', '-2', '1.5', 'x'):
            with pytest.raises(ValueError, match=key):
                actuated_kw({key: bad})
    for bad in ('-1', '1.5', 'x'):
        with pytest.raises(ValueError, match='sotl_mu'):
            actuated_kw(dict(sotl_mu=bad))
    for key in ('actuated_gap_sec', 'sotl_omega'):
        for bad in ('0', '-2.5', 'inf', 'nan', 'x'):
            with pytest.raises(ValueError, match=key):
                actuated_kw({key: bad})
    with pytest.raises(ValueError, match='actuated_max_green = 3: must be >= actuated_min_green = 4'):
        actuated_kw(dict(actuated_min_green='4', actuated_max_green='3'))
    # the keys the other controllers read are theirs alone
    assert controller_kw(dict(actuated_min_green='0')) == dict(pressure_measure='count', pressure_min_green=1, fixed_time_steps=6)
    assert CONTROLLERS == ('greedy', 'maxpressure', 'fixedtime', 'actuated', 'sotl')


def test_cli_refusals_before_any_device_work(tmp_path):
    from deeprl_signal_control_amd import main
    write_config(tmp_path, 'actuated', 'actuated_min_green = 4\nactuated_max_green = 3')
    with pytest.raises(ValueError, match='actuated_max_green'):
        main.evaluate_agent(str(tmp_path / 'actuated'), str(tmp_path) + '/', [10000])
    write_config(tmp_path, 'sotl', 'sotl_theta = 0')
    with pytest.raises(ValueError, match='sotl_theta'):
        main.evaluate_agent(str(tmp_path / 'sotl'), str(tmp_path) + '/', [10000])
    for agent in ('actuated', 'sotl'):
        cfg = write_config(tmp_path / 'train', agent)
        args = main.parse_args(['--base-dir', str(tmp_path / 'out' / agent), 'train', '--config-dir', cfg])
        with pytest.raises(ValueError, match='no learner'):
            main.train(args)


def test_abi_names():
    header = open(os.path.join(ROOT, 'include', 'tsc.h')).read()
    for name in ('tsc_env_set_actuated', 'tsc_env_actuated_actions', 'tsc_env_actuated_state'):
        assert name in _lib.SYMBOLS and ('int %s(' % name) in header
    assert '120: tsc_env_set_actuated' in header and 'TSC_ACTUATED_GAP = 0, TSC_ACTUATED_SOTL = 1' in header


# ---- non-vacuity of the closed-loop GPU cases, on the oracle alone ----------------------------------------------------------------
def closed_loop_scenario(name):
    if name == 'real_net':
        if name not in _cache:
            _cache[name] = build_scenario('real_net', 'greedy', episode_length_sec=600)
        return _cache[name]
    return nw.NETWORKS[name].scenario()


@pytest.mark.parametrize('name,seeds,steps,least,absent', [
    ('grid_x2', (410, 411), 60, 10, ()), ('real_net', (2000,), 120, 10, ()), ('ctrl8', (480,), 60, 3, ('skip',))])
def test_closed_loop_takes_every_branch(name, seeds, steps, least, absent):
    """The GPU cases' runs (tests/actuated_rules.py GAP and SOTL) on OracleEnv, driven by the loop rule.  Measured: grid_x2 gap rule
    forced 99 (46 + 53) the rarest, SOTL min_green 449; real_net forced 38, SOTL min_green and change 24 each; ctrl8 (three phases
    in a corridor) never skips, its rarest branch is no_demand, 3 times."""
    scn = closed_loop_scenario(name)
    for rule, prm, names in (('actuated', R.GAP, R.GAP_BRANCHES), ('sotl', R.SOTL, R.SOTL_BRANCHES)):
        took = R.closed_loop(scn, rule, prm, seeds, steps)
        print(name, rule, took)
        for k in names:
            if k in absent:
                assert took.get(k, 0) == 0, (rule, k, took)
            else:
                assert took.get(k, 0) >= least, (rule, k, took)
