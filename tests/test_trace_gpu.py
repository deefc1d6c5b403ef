"""Per-vehicle trajectories on the device (tsc_env_trace, the traced recording kernels) against the CPU oracle: every second's rows,
lane by lane in queue order, equal the oracle's vehicles bit for bit, for the IDM and the Krauss walk, at both workgroup sizes the
recording walk runs with; the trace changes nothing else the env computes; its rows agree with the traffic table and the trip log."""
import numpy as np
import pytest
import torch

from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net, build_small_grid

pytestmark = pytest.mark.gpu


def _snapshot_oracle(scn, seed):
    """OracleEnv whose _simulate also keeps, after every simulated second, every lane's vehicles (route, x, v, global id)."""
    from oracle.env_oracle import OracleEnv

    class SnapOracle(OracleEnv):
        def _simulate(self, num_step):
            for _ in range(num_step):
                self.ms.step(1)
                self.cur_sec += 1
                if self.is_record:
                    self._measure_traffic_step()
                lv = [self.ms.lane_vehicles(l) for l in range(self.scn.n_lane)]
                self.snaps.append({k: np.concatenate([d[k] for d in lv]) for k in ('r', 'x', 'v', 'id')}
                                  | {'n': np.array([d['n'] for d in lv])})

    o = SnapOracle(scn, seed=seed)
    o.snaps = []
    return o


def _actions(env, scn, rng, policy, E):
    if policy == 'greedy':
        return env.greedy_actions()
    act = np.zeros((E, scn.n_agent), np.int32)
    for a, n in enumerate(scn.n_a_ls):
        act[:, a] = rng.randint(0, n, E)
    return torch.from_numpy(act).cuda()


def _check_against_oracle(scn, tr, snaps, by_entry_lane=False):
    """Rows of every second (time_sec = second + 1) == the oracle's vehicles in (lane, slot) order; oracle id <-> (route, serial)
    one bijection over the whole run.  by_entry_lane: serials count per insertion stream, so where several streams share a route
    (the synthetic networks of tests/networks.py) the key is (route, serial, the lane the vehicle was first seen on -- its
    stream's entry lane)."""
    assert len(snaps) > 0
    ends = np.cumsum([0] + [int((tr['time_sec'] == j + 1).sum()) for j in range(len(snaps))])
    assert ends[-1] == len(tr['time_sec']), 'rows after the last simulated second'
    id_of, key_of, entry = {}, {}, {}
    for j, sn in enumerate(snaps):
        sl = slice(ends[j], ends[j + 1])
        np.testing.assert_array_equal(tr['sim_lane'][sl], np.repeat(np.arange(scn.n_lane), sn['n']), err_msg='second %d' % j)
        np.testing.assert_array_equal(tr['route'][sl], sn['r'], err_msg='second %d' % j)
        np.testing.assert_array_equal(tr['x'][sl].view(np.uint32), sn['x'].view(np.uint32), err_msg='second %d' % j)
        np.testing.assert_array_equal(tr['speed'][sl].astype(np.float32).view(np.uint32), sn['v'].view(np.uint32), err_msg='second %d' % j)
        for oid, l, r, s in zip(sn['id'].tolist(), tr['sim_lane'][sl].tolist(), tr['route'][sl].tolist(), tr['serial'][sl].tolist()):
            key = (r, s, entry.setdefault(oid, l)) if by_entry_lane else (r, s)
            assert id_of.setdefault(key, oid) == oid and key_of.setdefault(oid, key) == key, (j, oid, r, s)
    return len(id_of)


def _run(scn, E, steps, traced, policy, seed=21, rng_seed=0):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    env = VecTrafficEnv(scn, E, seed=seed)
    env.set_record(True)
    env.set_trace(traced)
    orc = {e: _snapshot_oracle(scn, seed + e) for e in traced}
    env.reset()
    for o in orc.values():
        o.reset()
    rng = np.random.RandomState(rng_seed)
    for t in range(steps):
        act = _actions(env, scn, rng, policy, E)
        env.step(act)
        a = act.cpu().numpy()
        for e, o in orc.items():
            o.step(list(a[e]))
    tr = env.collect_trajectories()
    assert sorted(tr) == sorted(traced)
    ids = [_check_against_oracle(scn, tr[e], orc[e].snaps) for e in traced]
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
    from oracle.microsim import lib
    monkeypatch.setenv('TSC_ENV_THREADS', threads)
    scn = build_large_grid('greedy', car_following='krauss', krauss_sigma=0.5)
    L = lib()
    L.ms_set_krauss(1, 0.5)
    try:
        ids = _run(scn, 8, 60, [0, 7], 'random')
    finally:
        L.ms_set_krauss(0, 0.5)
    assert min(ids) > 50


def test_trace_benchmark_shape():
    """E = 1024 with the library's own workgroup choice; instances at both ends and in the middle."""
    ids = _run(build_large_grid('greedy'), 1024, 24, [0, 513, 1023], 'greedy')
    assert min(ids) > 50


def _pair(scn, E, seed=5):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    envs = []
    for _ in range(2):
        env = VecTrafficEnv(scn, E, seed=seed)
        env.set_record(True)
        envs.append(env)
    return envs


def _step_both(envs, scn, rng, E, steps):
    """Same actions into both envs; everything they return must agree."""
    for _ in range(steps):
        act = np.zeros((E, scn.n_agent), np.int32)
        for a, n in enumerate(scn.n_a_ls):
            act[:, a] = rng.randint(0, n, E)
        outs = [[x.cpu().numpy().copy() for x in env.step(torch.from_numpy(act).cuda())] for env in envs]
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x, y)


def _tables_equal(a, b):
    a.collect_tripinfo(); b.collect_tripinfo()
    for k in ('traffic_data', 'control_data', 'trip_data', 'truncated_trip_data'):
        assert getattr(a, k) == getattr(b, k), k


def test_trace_only_observes():
    scn = build_large_grid('greedy')
    E = 8
    traced, plain = _pair(scn, E)
    traced.set_trace([1, 4])
    for env in (traced, plain):
        env.reset()
    _step_both([traced, plain], scn, np.random.RandomState(3), E, 80)
    _tables_equal(traced, plain)
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
        env.step(_actions(env, scn, rng, 'random', E))
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
        env.step(_actions(env, scn, rng, 'random', E))
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
    traced, plain = _pair(scn, E)
    with pytest.raises(RuntimeError):                              # the C ABI's own checks
        traced.set_trace([0, 0])
    with pytest.raises(RuntimeError):
        traced.set_trace([E])
    traced.set_trace([0, 2], row_cap=100)
    for env in (traced, plain):
        env.reset()
    rng = np.random.RandomState(4)
    _step_both([traced, plain], scn, rng, E, 20)
    with pytest.raises(RuntimeError, match='row_cap'):
        traced.collect_trajectories()
    traced.set_trace([])                                           # detached: the untraced recording kernels from here on
    assert traced.collect_trajectories() == {}
    _step_both([traced, plain], scn, rng, E, 20)
    _tables_equal(traced, plain)
    for env in (traced, plain):
        env.close()


def test_trace_refused_rearm_keeps_handle():
    """A re-arming call the library refuses changes nothing: the handle goes on as one that never saw it."""
    scn = build_large_grid('greedy')
    E = 4
    bad, good = _pair(scn, E)
    for env in (bad, good):
        env.set_trace([0, 2])
        env.reset()
    rng = np.random.RandomState(2)
    _step_both([bad, good], scn, rng, E, 2)                        # the trace is running when the bad call comes
    with pytest.raises(RuntimeError, match='instance 1 listed twice'):
        bad.set_trace([1, 1])
    for env in (bad, good):
        env.reset()
    _step_both([bad, good], scn, rng, E, 4)
    tr_b, tr_g = bad.collect_trajectories(), good.collect_trajectories()
    assert sorted(tr_b) == sorted(tr_g) == [0, 2]
    for e in tr_g:
        assert len(tr_g[e]['time_sec']) > 0 and sorted(tr_b[e]) == sorted(tr_g[e])
        for k in tr_g[e]:
            np.testing.assert_array_equal(tr_b[e][k], tr_g[e][k], err_msg='%d %s' % (e, k))
    for env in (bad, good):
        env.close()
