"""Per-vehicle trajectories on the device (tsc_env_trace, the traced recording kernels) against the CPU oracle: every second's rows,
lane by lane in queue order, equal the oracle's vehicles bit for bit, for the IDM and the Krauss walk, at both workgroup sizes the
recording walk runs with; the trace changes nothing else the env computes; its rows agree with the traffic table and the trip log."""
import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net, build_small_grid
from tests import env_harness as H
from tests.env_rules import check_trace

pytestmark = pytest.mark.gpu


def _run(scn, E, steps, traced, policy, seed=21, rng_seed=0):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    env = VecTrafficEnv(scn, E, seed=seed)
    env.set_record(True)
    env.set_trace(traced)
    orc = {e: H.snapshot_oracle(scn, seed + e) for e in traced}
    env.reset()
    obs = {e: o.reset() for e, o in orc.items()}
    rng = np.random.RandomState(rng_seed)
    H.follow(env, H.oracle_steps(scn, orc, obs, steps, lambda t, obs: (H.policy_actions(env, rng, policy), None)))
    tr = env.collect_trajectories()
    assert sorted(tr) == sorted(traced)
    ids = [check_trace(scn, tr[e], orc[e].snaps) for e in traced]
    env.close()
    return ids


@pytest.mark.parametrize('name,policy', [('large_grid', 'random'), ('large_grid', 'greedy'), ('real_net', 'random'),
                                         ('real_net', 'greedy'), ('small_grid', 'random'), ('small_grid', 'greedy')])
def test_trace_matches_oracle(name, policy):
    scn = {'large_grid': lambda: build_large_grid('greedy'), 'real_net': lambda: build_real_net('greedy'),
           'small_grid': lambda: build_small_grid('greedy')}[name]()
    ids = _run(scn, 8, 60, [2, 5], policy)
    assert min(ids) > 50                                          # vehicles enough to mean something


@pytest.mark.parametrize('threads', ['256', '1024'])
def test_trace_matches_oracle_krauss(threads, monkeypatch):
    monkeypatch.setenv('TSC_ENV_THREADS', threads)
    scn = build_large_grid('greedy', car_following='krauss', krauss_sigma=0.5)
    with H.oracle_krauss(0.5):
        ids = _run(scn, 8, 60, [0, 7], 'random')
    assert min(ids) > 50


def test_trace_benchmark_shape():
    """E = 1024 with the library's own workgroup choice; instances at both ends and in the middle."""
    ids = _run(build_large_grid('greedy'), 1024, 24, [0, 513, 1023], 'greedy')
    assert min(ids) > 50


def test_trace_only_observes():
    scn = build_large_grid('greedy')
    E = 8
    traced, plain = H.recording_pair(scn, E)
    traced.set_trace([1, 4])
    for env in (traced, plain):
        env.reset()
    H.lockstep_uniform([traced, plain], scn, np.random.RandomState(3), E, 80, tables=True)
    assert all(len(v['time_sec']) > 0 for v in traced.collect_trajectories().values())
    for env in (traced, plain):
        env.close()


def test_trace_consistency():
    """Rows per second == the traffic table's number_total_car; a finished trip's id is in the rows from the second after its
    depart second (the trip log's depart is the second it was inserted in, whose end the traffic table labels depart + 1) up to
    the second before its arrival, and nowhere else; reset() starts the counts over."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    E = 4
    env = VecTrafficEnv(scn, E, seed=9)
    env.set_record(True)
    env.set_trace([0, 3])
    env.reset()
    rng = np.random.RandomState(1)
    for _ in range(120):
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
    env.collect_tripinfo()
    tr = env.collect_trajectories()
    n_trips = 0
    for e in (0, 3):
        d = tr[e]
        per_sec = np.bincount(d['time_sec'], minlength=601)[1:601]
        tot = np.array([r['number_total_car'] for r in env.traffic_data[e]])
        assert [r['time_sec'] for r in env.traffic_data[e]] == list(range(1, 601))
        np.testing.assert_array_equal(per_sec, tot)
        for row in env.trip_data[e]:
            secs = d['time_sec'][d['id'] == row['id']]
            dep, arr = int(float(row['depart_sec'])), int(float(row['arrival_sec']))
            np.testing.assert_array_equal(secs, np.arange(dep + 1, arr), err_msg=row['id'])
            n_trips += 1
    assert n_trips > 100
    env.reset()
    for _ in range(2):
        env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
    tr = env.collect_trajectories()
    assert tr[0]['time_sec'].max() == 10 and len(tr[0]['time_sec']) == sum(r['number_total_car'] for r in env.traffic_data[0][-10:])
    env.close()


def test_trace_overflow_and_detach():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    E = 4
    with pytest.raises(ValueError, match='set_record'):
        bare = VecTrafficEnv(scn, E, seed=5)
        try:
            bare.set_trace([0])
        finally:
            bare.close()
    traced, plain = H.recording_pair(scn, E)
    with pytest.raises(RuntimeError):                              # the C ABI's own checks
        traced.set_trace([0, 0])
    with pytest.raises(RuntimeError):
        traced.set_trace([E])
    traced.set_trace([0, 2], row_cap=100)
    for env in (traced, plain):
        env.reset()
    rng = np.random.RandomState(4)
    H.lockstep_uniform([traced, plain], scn, rng, E, 20)
    with pytest.raises(RuntimeError, match='row_cap'):
        traced.collect_trajectories()
    traced.set_trace([])                                           # detached: the untraced recording kernels from here on
    assert traced.collect_trajectories() == {}
    H.lockstep_uniform([traced, plain], scn, rng, E, 20, tables=True)
    for env in (traced, plain):
        env.close()


def test_trace_refused_rearm_keeps_handle():
    """A re-arming call the library refuses changes nothing: the handle goes on as one that never saw it."""
    scn = build_large_grid('greedy')
    E = 4
    bad, good = H.recording_pair(scn, E)
    for env in (bad, good):
        env.set_trace([0, 2])
        env.reset()
    rng = np.random.RandomState(2)
    H.lockstep_uniform([bad, good], scn, rng, E, 2)                        # the trace is running when the bad call comes
    with pytest.raises(RuntimeError, match='instance 1 listed twice'):
        bad.set_trace([1, 1])
    for env in (bad, good):
        env.reset()
    H.lockstep_uniform([bad, good], scn, rng, E, 4)
    tr_b, tr_g = bad.collect_trajectories(), good.collect_trajectories()
    assert sorted(tr_b) == sorted(tr_g) == [0, 2]
    for e in tr_g:
        assert len(tr_g[e]['time_sec']) > 0 and sorted(tr_b[e]) == sorted(tr_g[e])
        for k in tr_g[e]:
            np.testing.assert_array_equal(tr_b[e][k], tr_g[e][k], err_msg='%d %s' % (e, k))
    for env in (bad, good):
        env.close()
