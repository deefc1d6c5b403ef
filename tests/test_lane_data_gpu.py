"""Per-lane traffic statistics on the device (tsc_env_lane_data, SUMO's laneData) against the CPU oracle: the raw sums of every slot,
interval and instance equal, bit for bit, what the oracle's vehicles after every simulated second give under the semantics of
INTEGRATION.md ("Lane data"), for the IDM and the Krauss walk, at both workgroup sizes of the recording walk and at E = 1024; the
sums agree with the traffic table, the counters and a trajectory trace of the same run; they change nothing else the env computes."""
import ctypes as C
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net, build_small_grid
from tests import env_harness as H
from tests.env_rules import F, INTS, check_lane_data

pytestmark = pytest.mark.gpu

SCENARIOS = {'large_grid': lambda **kw: build_large_grid('greedy', **kw), 'real_net': lambda **kw: build_real_net('greedy', **kw),
             'small_grid': lambda **kw: build_small_grid('greedy', **kw)}


def _run(scn, E, steps, instances, policy, period=60, seed=21, rng_seed=0):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    env = VecTrafficEnv(scn, E, seed=seed)
    env.set_record(True)
    env.set_lane_data(period)
    orc = {e: H.snapshot_oracle(scn, seed + e) for e in instances}
    env.reset()
    obs = {e: o.reset() for e, o in orc.items()}
    rng = np.random.RandomState(rng_seed)
    H.follow(env, H.oracle_steps(scn, orc, obs, steps, lambda t, obs: (H.policy_actions(env, rng, policy), None)))
    sums = check_lane_data(scn, env, orc, period)
    ints, _ = env.read_lane_data()                                  # (the instances the oracle did not run have sums too)
    assert (ints[:, :, F['sampledSeconds']].sum(axis=(1, 2)) > 0).all()
    env.close()
    return sums


@pytest.mark.parametrize('name,policy', [('large_grid', 'random'), ('large_grid', 'greedy'), ('real_net', 'random'),
                                         ('real_net', 'greedy'), ('small_grid', 'random'), ('small_grid', 'greedy')])
def test_lane_data_matches_oracle(name, policy):
    scn = SCENARIOS[name]()
    sums = _run(scn, 8, 60, list(range(8)), policy)
    assert min(s['departed'] for s in sums.values()) > 50
    if name == 'large_grid':
        assert sum(s['laneChangedFrom'] for s in sums.values()) > 0           # rule 10 is exercised
    if name == 'real_net':
        assert sum(s['entered'] for s in sums.values()) > 0


@pytest.mark.parametrize('threads', ['256', '1024'])
def test_lane_data_matches_oracle_krauss(threads, monkeypatch):
    monkeypatch.setenv('TSC_ENV_THREADS', threads)
    scn = build_large_grid('greedy', car_following='krauss', krauss_sigma=0.5)
    with H.oracle_krauss(0.5):
        sums = _run(scn, 8, 60, list(range(8)), 'random')
    assert min(s['departed'] for s in sums.values()) > 50


def test_lane_data_benchmark_shape():
    """E = 1024 with the library's own workgroup choice; instances at both ends and in the middle."""
    sums = _run(build_large_grid('greedy'), 1024, 60, [0, 513, 1023], 'greedy')
    assert min(s['departed'] for s in sums.values()) > 50


def test_lane_data_consistency():
    """Per instance and interval: sampled vehicle-seconds, departures and arrivals against the traffic table; teleports against
    the counters; per SUMO lane the balance of vehicles (from a trajectory trace of the same run) against the event counts;
    reset() starts the sums over."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    E, period = 4, 60
    env = VecTrafficEnv(scn, E, seed=9)
    env.set_record(True)
    env.set_trace(range(E))
    env.set_lane_data(period)
    env.reset()
    rng = np.random.RandomState(1)
    steps = 120
    for _ in range(steps):
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
    T = steps * scn.control_interval_sec
    n_int = T // period
    cols = env.collect_lane_data()
    tr = env.collect_trajectories()
    names = scn.lane_data_slots()['names']
    n_sumo = len(names)
    teleported = env.counters()[1]
    for e in range(E):
        c = {k: np.asarray(cols[e][k]).reshape(-1, n_sumo) for k in INTS}
        traffic = pd.DataFrame(env.traffic_data[e])
        assert list(traffic['time_sec']) == list(range(1, T + 1))
        k_of = (traffic['time_sec'].to_numpy() - 1) // period
        for key, col in (('sampledSeconds', 'number_total_car'), ('departed', 'number_departed_car'),
                         ('arrived', 'number_arrived_car')):
            want = np.bincount(k_of, weights=traffic[col].to_numpy(), minlength=n_int).astype(np.int64)
            np.testing.assert_array_equal(c[key][:n_int].sum(axis=1), want, err_msg='%s, instance %d' % (key, e))
            assert c[key][n_int:].sum() == 0
        assert c['teleported'].sum() == teleported[e]
        d = tr[e]
        lane_idx = {nm: j for j, nm in enumerate(names)}
        lane_of = np.array([lane_idx[nm] for nm in d['lane']])

        def count(sec):                                             # vehicles per SUMO lane at the end of second sec - 1
            return np.bincount(lane_of[d['time_sec'] == sec], minlength=n_sumo)

        for k in range(n_int):
            start = count(k * period) if k else np.zeros(n_sumo, np.int64)
            bal = (c['departed'][k] + c['entered'][k] + c['laneChangedTo'][k] - c['arrived'][k] - c['left'][k]
                   - c['laneChangedFrom'][k] - c['teleported'][k])
            np.testing.assert_array_equal(count((k + 1) * period) - start, bal, err_msg='interval %d, instance %d' % (k, e))
            # sampled vehicle-seconds per SUMO lane = the trace's rows on it over the interval's seconds
            secs = (d['time_sec'] > k * period) & (d['time_sec'] <= (k + 1) * period)
            np.testing.assert_array_equal(c['sampledSeconds'][k], np.bincount(lane_of[secs], minlength=n_sumo))
    env.reset()
    for _ in range(2):
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
    cols = env.collect_lane_data()
    for e in range(E):
        s = np.asarray(cols[e]['sampledSeconds']).reshape(-1, n_sumo)
        assert s[0].sum() == sum(r['number_total_car'] for r in env.traffic_data[e][-10:])
        assert s[1:].sum() == 0
    env.close()


@pytest.mark.parametrize('with_trace', [False, True])
def test_lane_data_only_observes(with_trace):
    scn = build_real_net('greedy')
    E = 8
    measured, plain = H.recording_pair(scn, E)
    if with_trace:
        measured.set_trace([1, 6])
    measured.set_lane_data(300)
    for env in (measured, plain):
        env.reset()
    rng = np.random.RandomState(3)
    H.lockstep_uniform([measured, plain], scn, rng, E, 80, tables=True)
    assert all(np.asarray(c['sampledSeconds']).sum() > 0 for c in measured.collect_lane_data().values())
    if with_trace:
        assert all(len(v['time_sec']) > 0 for v in measured.collect_trajectories().values())
    measured.set_lane_data(0)                                        # detached: the recording kernels without lane data
    assert measured.collect_lane_data() == {}
    with pytest.raises(RuntimeError, match='no lane data'):
        measured.read_lane_data()
    one_i, one_d = np.zeros(1, np.int32), np.zeros(1, np.float64)
    with pytest.raises(RuntimeError, match='no lane data'):
        _lib.check(measured._L.tsc_env_read_lane_data(measured._h, one_i.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      one_d.ctypes.data_as(C.POINTER(C.c_double))))
    H.lockstep_uniform([measured, plain], scn, rng, E, 20, tables=True)
    for env in (measured, plain):
        env.close()


def test_lane_data_arguments():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    env = VecTrafficEnv(scn, 2, seed=5)
    try:
        with pytest.raises(ValueError, match='set_record'):
            env.set_lane_data(60)
        env.set_record(True)
        with pytest.raises(ValueError, match='multiple'):
            env.set_lane_data(7)
        tabs = scn.lane_data_slots()
        ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        with pytest.raises(RuntimeError, match='multiple'):         # the C ABI's own check
            _lib.check(env._L.tsc_env_lane_data(env._h, 7, len(tabs['start']), tabs['slot0'].ctypes.data_as(ip),
                                                tabs['start'].ctypes.data_as(fp), tabs['sumo'].ctypes.data_as(ip)))
    finally:
        env.close()


def test_lane_data_refused_rearm_keeps_handle():
    """A re-arming call the library refuses changes nothing: the handle goes on as one that never saw it."""
    scn = build_large_grid('greedy')
    E = 2
    bad, good = H.recording_pair(scn, E)
    for env in (bad, good):
        env.set_lane_data(60)
        env.reset()
    rng = np.random.RandomState(2)
    H.lockstep_uniform([bad, good], scn, rng, E, 2)                          # the lane data is live when the bad call comes
    tabs = scn.lane_data_slots()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    with pytest.raises(RuntimeError, match='bad slot tables'):
        _lib.check(bad._L.tsc_env_lane_data(bad._h, 120, scn.n_lane - 1, tabs['slot0'].ctypes.data_as(ip),
                                            tabs['start'].ctypes.data_as(fp), tabs['sumo'].ctypes.data_as(ip)))
    for env in (bad, good):
        env.reset()
    H.lockstep_uniform([bad, good], scn, rng, E, 4)
    (ints_b, speed_b), (ints_g, speed_g) = bad.read_lane_data(), good.read_lane_data()
    np.testing.assert_array_equal(ints_b, ints_g)
    np.testing.assert_array_equal(speed_b, speed_g)
    assert ints_g.sum() > 0 and speed_g.sum() > 0
    for env in (bad, good):
        env.close()


def test_evaluate_lane_data(tmp_path):
    """evaluate --lane-data 300 with 4 seeds over the reference's 3600-s episode: 4 x 12 x n_sumo_lanes rows; per seed the sampled
    vehicle-seconds equal the traffic table's vehicles."""
    from deeprl_signal_control_amd import main as cli
    from tests.test_cli_gpu import INI
    assert 'episode_length_sec = 300\n' in INI
    cfg = tmp_path / 'config_greedy.ini'
    cfg.write_text((INI % {'agent': 'greedy'}).replace('episode_length_sec = 300\n', 'episode_length_sec = 3600\n'))
    base = str(tmp_path / 'exp')
    os.makedirs(base + '/greedy/data')
    shutil.copy(str(cfg), base + '/greedy/data/')
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'greedy', '--evaluation-seeds', '10000,20000,30000,40000',
                    '--lane-data', '300'])
    assert out['greedy'][0].shape == (4,)
    eva = base + '/eva_data/'
    ld = pd.read_csv(eva + 'large_grid_greedy_lanedata.csv', index_col=0)
    assert list(ld.columns) == ['episode', 'begin', 'end', 'id', 'sampledSeconds', 'density', 'occupancy', 'waitingTime', 'speed',
                                'traveltime', 'departed', 'arrived', 'entered', 'left', 'laneChangedFrom', 'laneChangedTo',
                                'teleported']
    n_sumo = len(build_large_grid('greedy').lane_data_slots()['names'])
    assert len(ld) == 4 * 12 * n_sumo
    assert sorted(set(ld['episode'])) == [1, 2, 3, 4]
    traffic = pd.read_csv(eva + 'large_grid_greedy_traffic.csv', index_col=0)
    for ep in range(1, 5):
        assert ld[ld['episode'] == ep]['sampledSeconds'].sum() == traffic[traffic['episode'] == ep]['number_total_car'].sum()
    assert ld['sampledSeconds'].sum() > 0
