"""Host side of the max-pressure / fixed-time controllers (no GPU): Scenario.pressure_tables against a plain-loop derivation,
the host restatement trainer.max_pressure_actions on hand-made states, the hold, the config keys and the ABI list.  Everything
is integer arithmetic: equality is exact."""
import configparser
import os

import numpy as np
import pytest

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import controller_kw
from deeprl_signal_control_amd.scenario import LANE_CAP, build_scenario
from deeprl_signal_control_amd.trainer import greedy_actions, max_pressure_actions, pressure_hold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ('large_grid', 'real_net', 'small_grid')
_cache = {}


def scenario(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        scn = build_scenario(name, 'greedy', **kw)
        _cache[key] = (scn, scn.pressure_tables())
    return _cache[key]


def loop_tables(scn):
    """The movements and served lists by plain loops over mv_next, mv_link and green_tab (the issue's definition)."""
    seen = set()
    for l in range(scn.n_lane):
        a = int(scn.lane_node[l])
        for r in range(scn.n_route):
            m, k = int(scn.mv_next[l, r]), int(scn.mv_link[l, r])
            if a >= 0 and m >= 0 and k >= 0:
                seen.add((a, l, m, k))
    mov = sorted(seen)
    served = {}
    for a in range(scn.n_agent):
        for p in range(int(scn.agent_nphase[a])):
            served[a, p] = [i for i, (a2, _l, _m, k) in enumerate(mov) if a2 == a and chr(scn.green_tab[a, p, k]) in 'Gg']
    return mov, served


@pytest.mark.parametrize('name', SCENARIOS)
def test_movement_tables(name):
    scn, tb = scenario(name)
    mov, served = loop_tables(scn)
    assert [tuple(int(x) for x in row) for row in tb['mov']] == mov          # ordered by agent, l, m, k
    assert len(mov) > 0 and (tb['mov'][:, 1:3] >= 0).all()                   # no movement has a negative lane
    for l in range(scn.n_lane):
        for r in range(scn.n_route):
            i = int(tb['lane_route_mov'][l, r])
            m, k = int(scn.mv_next[l, r]), int(scn.mv_link[l, r])
            if scn.lane_node[l] >= 0 and m >= 0 and k >= 0:
                assert mov[i] == (int(scn.lane_node[l]), l, m, k)
            else:
                assert i == -1
    # every signal link that any route uses appears in some movement
    used = {(int(scn.lane_node[l]), int(scn.mv_link[l, r])) for l in range(scn.n_lane) for r in range(scn.n_route)
            if scn.lane_node[l] >= 0 and scn.mv_link[l, r] >= 0 and scn.mv_next[l, r] >= 0}
    assert used == {(a, k) for a, _l, _m, k in mov}
    # each served list matches the phase strings; padded phases serve nothing
    PMAX = tb['served'].shape[1]
    for a in range(scn.n_agent):
        for p in range(PMAX):
            got = [int(i) for i in tb['served'][a, p, :tb['n_served'][a, p]]]
            assert (tb['served'][a, p, tb['n_served'][a, p]:] == -1).all()
            if p < scn.agent_nphase[a]:
                assert got == served[a, p]
                assert got == [i for i in got if scn.phases[a][p][mov[i][3]] in 'Gg']
            else:
                assert got == []
    assert sorted(tb['walk'].tolist()) == sorted({l for _a, l, _m, _k in mov} | {m for _a, _l, m, _k in mov})


def agent_structure(scn, tb, a):
    """An agent's movements without lane numbers: (position of l among the agent's incoming lanes, signal link, phases serving it)."""
    lanes = [int(x) for x in scn.agent_lanes[a, :scn.agent_nlane[a]]]
    out = []
    for i, (a2, l, _m, k) in enumerate(tb['mov'].tolist()):
        if a2 == a:
            out.append((lanes.index(l), k, tuple(p for p in range(int(scn.agent_nphase[a])) if i in tb['served'][a, p])))
    return sorted(out)


def test_large_grid_same_structure_at_all_agents():
    """Movements come from routes.  With every turning movement routed (init_density > 0: the sinks are drawn per episode, 20
    routes over all 132 streams) all 25 intersections have the same twelve movements and the same served lists.  The default demand
    has twelve routes that leave some turns unused: each intersection then has exactly that template restricted to the links its
    routes use."""
    scn, tb = scenario('large_grid', init_density=0.2)
    template = agent_structure(scn, tb, 0)
    assert len(template) == 12 and sorted(k for _j, k, _s in template) == list(range(12))
    for a in range(25):
        assert agent_structure(scn, tb, a) == template
        assert tb['n_served'][a].tolist() == tb['n_served'][0].tolist()
    scn, tb = scenario('large_grid')
    for a in range(25):
        mine = agent_structure(scn, tb, a)
        links = {k for _j, k, _s in mine}
        assert mine == [t for t in template if t[1] in links]


def empty_state(scn):
    NL = scn.n_lane
    return dict(n=np.zeros(NL, np.int32), x=np.zeros((NL, LANE_CAP), np.float32), v=np.zeros((NL, LANE_CAP), np.float32),
                r=np.zeros((NL, LANE_CAP), np.int32))


def put(st, lane, route, count, v=0.0):
    for _ in range(count):
        i = int(st['n'][lane])
        st['r'][lane, i], st['v'][lane, i] = route, v
        st['n'][lane] = i + 1


def route_of(tb, i):
    l = int(tb['mov'][i, 1])
    return int(np.flatnonzero(tb['lane_route_mov'][l] == i)[0])


def test_tie_goes_to_the_lower_phase():
    scn, tb = scenario('large_grid')
    act, prs = max_pressure_actions(scn, empty_state(scn), return_pressure=True)
    assert (prs == 0).all() and (act == 0).all()
    # a movement that phases 1.. serve but phase 0 does not: the first of its phases wins
    a = 12
    i = next(i for i in np.flatnonzero(tb['mov'][:, 0] == a) if i not in tb['served'][a, 0])
    phases = [p for p in range(5) if i in tb['served'][a, p]]
    st = empty_state(scn)
    put(st, int(tb['mov'][i, 1]), route_of(tb, i), 3)
    act, prs = max_pressure_actions(scn, st, return_pressure=True)
    assert len(phases) >= 2 and all(prs[a, p] == 3 for p in phases) and act[a] == phases[0]


def wave_of(scn, st):
    """The greedy controllers' input for this state: vehicles on every incoming lane (all of them inside the detector here)."""
    w = np.zeros((scn.n_agent, scn.agent_lanes.shape[1]))
    for a in range(scn.n_agent):
        for j in range(int(scn.agent_nlane[a])):
            w[a, j] = st['n'][scn.agent_lanes[a, j]]
    return w


def test_full_downstream_lane_flips_the_choice_away_from_greedy():
    scn, tb = scenario('large_grid')
    a, found = 12, False
    for i in np.flatnonzero(tb['mov'][:, 0] == a):
        l, m = int(tb['mov'][i, 1]), int(tb['mov'][i, 2])
        st = empty_state(scn)
        put(st, l, route_of(tb, i), 5)
        g = greedy_actions(scn, wave_of(scn, st))
        mp = max_pressure_actions(scn, st)
        if i in tb['served'][a, g[a]] and mp[a] == g[a] and g[a] != 0:
            found = True
            break
    assert found, 'no movement of agent 12 on which greedy and max-pressure agree first'
    put(st, m, 0, 20)                                     # the downstream lane fills up (m is no incoming lane of agent a)
    g2 = greedy_actions(scn, wave_of(scn, st))
    mp2, prs = max_pressure_actions(scn, st, return_pressure=True)
    assert g2[a] == g[a]                                  # greedy is blind to the spill-back
    assert prs[a, g[a]] == 5 - 20 and mp2[a] != g2[a]


def test_queue_ignores_moving_vehicles():
    scn, tb = scenario('real_net')
    i = 0
    a, l = int(tb['mov'][i, 0]), int(tb['mov'][i, 1])
    st = empty_state(scn)
    put(st, l, route_of(tb, i), 4, v=5.0)
    put(st, l, route_of(tb, i), 2, v=0.05)
    put(st, l, route_of(tb, i), 1, v=0.1)                 # float32(0.1) is not < 0.1f: moving
    _, count = max_pressure_actions(scn, st, 'count', return_pressure=True)
    _, queue = max_pressure_actions(scn, st, 'queue', return_pressure=True)
    p = next(p for p in range(int(scn.agent_nphase[a])) if i in tb['served'][a, p])
    assert count[a, p] == 7 and queue[a, p] == 2
    st['v'][:] = 5.0
    _, queue = max_pressure_actions(scn, st, 'queue', return_pressure=True)
    assert (queue == 0).all()


def test_wrong_lane_vehicle_counts_downstream_only():
    scn, tb = scenario('large_grid')
    # a lane that is the downstream lane of some movement, and a route it does not serve (mv_next < -1: the vehicle must change lanes)
    for i in range(len(tb['mov'])):
        m = int(tb['mov'][i, 2])
        wrong = [r for r in range(scn.n_route) if scn.mv_next[m, r] < -1 and scn.lane_sib[m] >= 0 and scn.mv_next[scn.lane_sib[m], r] >= 0]
        if wrong and scn.lane_node[m] >= 0:
            break
    else:
        pytest.fail('no wrong-lane case in large_grid')
    st = empty_state(scn)
    put(st, m, wrong[0], 1)
    assert tb['lane_route_mov'][m, wrong[0]] == -1
    _, prs = max_pressure_actions(scn, st, return_pressure=True)
    assert (prs[int(scn.lane_node[m])] == 0).all()        # nothing upstream at its own intersection
    up_agent = int(tb['mov'][i, 0])
    for p in range(5):
        feeding = sum(1 for j in tb['served'][up_agent, p, :tb['n_served'][up_agent, p]] if tb['mov'][j, 2] == m)
        assert prs[up_agent, p] == -feeding               # ... but it fills the lane for the intersection upstream
    assert (prs[up_agent] < 0).any()


def test_host_restatement_refuses_device_tensors():
    import torch
    scn, _ = scenario('small_grid')
    st = {k: torch.from_numpy(v) for k, v in empty_state(scn).items()}
    with pytest.raises(TypeError, match='host restatement'):
        max_pressure_actions(scn, st)
    with pytest.raises(ValueError, match='count \\| queue'):
        max_pressure_actions(scn, empty_state(scn), measure='density')


def run_hold(seq, g):
    cur, age, out = -1, g, []                             # reset(): age = g, the first decision is free
    for p in seq:
        act, cur, age = pressure_hold(cur, age, p, g)
        out.append(act)
    return out


def test_hold_logic():
    seq = [2, 0, 0, 1, 1, 1, 3, 3, 0, 0]
    assert run_hold(seq, 1) == seq                        # stateless
    #        t: 0  1  2  3  4  5  6  7  8  9    2 held for steps 0-2; step 3 takes 1, held 3-5; step 6 takes 3, held 6-8; step 9 takes 0
    assert run_hold(seq, 3) == [2, 2, 2, 1, 1, 1, 3, 3, 3, 0]
    # an unchanged argmax does not restart the count: a change right after is taken at once
    assert run_hold([1, 1, 1, 1, 2, 2], 3) == [1, 1, 1, 1, 2, 2]
    out = run_hold([0, 1, 2, 3, 4, 0, 1, 2, 3], 3)
    assert out == [0, 0, 0, 3, 3, 3, 1, 1, 1]
    changes = [t for t in range(1, len(out)) if out[t] != out[t - 1]]
    assert all(b - a >= 3 for a, b in zip(changes, changes[1:]))


def test_config_keys():
    assert controller_kw({}) == dict(pressure_measure='count', pressure_min_green=1, fixed_time_steps=6)
    assert controller_kw(dict(pressure_measure=' queue ', pressure_min_green='3', fixed_time_steps='4')) == \
        dict(pressure_measure='queue', pressure_min_green=3, fixed_time_steps=4)
    with pytest.raises(ValueError, match='count \\| queue'):
        controller_kw(dict(pressure_measure='density'))
    for key in ('pressure_min_green', 'fixed_time_steps'):
        for bad in ('0', '-2', '1.5', 'x'):
            with pytest.raises(ValueError, match=key):
                controller_kw({key: bad})


INI = """
[MODEL_CONFIG]
policy = greedy

[TRAIN_CONFIG]
total_step = 120
test_interval = 60
log_interval = 60

[ENV_CONFIG]
clip_wave = 2.0
clip_wait = 2.0
control_interval_sec = 5
agent = %(agent)s
coop_gamma = 0.9
episode_length_sec = 300
norm_wave = 5.0
norm_wait = 100.0
coef_wait = 0.2
peak_flow1 = 1100
peak_flow2 = 925
init_density = 0
objective = hybrid
scenario = large_grid
seed = 12
test_seeds = 10000,20000
yellow_interval_sec = 2
%(extra)s
"""


def write_config(tmp_path, agent, extra=''):
    d = tmp_path / agent / 'data'
    d.mkdir(parents=True)
    (d / 'config.ini').write_text(INI % dict(agent=agent, extra=extra))
    return str(d / 'config.ini')


def test_cli_refusals_before_any_device_work(tmp_path):
    from deeprl_signal_control_amd import main
    write_config(tmp_path, 'maxpressure', 'pressure_measure = density')
    with pytest.raises(ValueError, match='count \\| queue'):
        main.evaluate_agent(str(tmp_path / 'maxpressure'), str(tmp_path) + '/', [10000])
    write_config(tmp_path, 'fixedtime', 'fixed_time_steps = 0')
    with pytest.raises(ValueError, match='fixed_time_steps'):
        main.evaluate_agent(str(tmp_path / 'fixedtime'), str(tmp_path) + '/', [10000])
    for agent in ('maxpressure', 'fixedtime'):
        cfg = write_config(tmp_path / 'train', agent)
        args = main.parse_args(['--base-dir', str(tmp_path / 'out' / agent), 'train', '--config-dir', cfg])
        with pytest.raises(ValueError, match='no learner'):
            main.train(args)


def test_abi_names():
    new = ('tsc_env_set_pressure', 'tsc_env_pressure_actions', 'tsc_env_fixed_time_actions')
    header = open(os.path.join(ROOT, 'include', 'tsc.h')).read()
    for name in new:
        assert name in _lib.SYMBOLS and ('int %s(' % name) in header
    assert '112: tsc_env_set_pressure' in header
