"""Per-instance traffic demand on the device (tsc_env_set_demand, demand_kernel, the per-instance emission tables step_kernel reads)
against the CPU oracle: instance e of a handle runs its own veh/h column, its oracle is OracleEnv(replace(scn, flows=flows_e)), and
observations, rewards and the vehicle state are equal bit for bit -- on every scenario, every workgroup size, the Krauss walk and
the recording / trace / lane-data walks; the nominal column is the handle's old behaviour; errors change nothing."""
import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import DemandSampler, build_large_grid, build_real_net, build_small_grid
from tests import env_harness as H
from tests.env_harness import assert_same as _same, demand_parity, episode_outputs as _episode, with_rates
from tests.env_rules import check_trace, expected_vehicles

pytestmark = pytest.mark.gpu

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)


def _columns(scn, E, jitter=0.2, scales=SCALES):
    """int32 [E, n_flow]: instance e runs scale scales[e % len] with every flow element jittered by u in [1 - j, 1 + j]."""
    smp = DemandSampler(scn, scales)
    rows = []
    for e in range(E):
        u = np.random.RandomState(1000 + e).uniform(1.0 - jitter, 1.0 + jitter, len(scn.flows))
        rows.append((smp.column(scales[e % len(scales)]).astype(np.float64) * u).astype(np.int32))
    return np.stack(rows)


# ---- 1. parity with the oracle, large_grid MA2C ---------------------------------------------------------------------------
@pytest.mark.parametrize('E,steps,threads', [(24, 150, '256'), (24, 150, '512'), (24, 150, '1024'), (24, 150, ''), (8, 720, '')])
def test_large_grid_vs_oracle(E, steps, threads, monkeypatch):
    if threads:
        monkeypatch.setenv('TSC_ENV_THREADS', threads)
    scn = build_large_grid('ma2c')
    vph = _columns(scn, E)
    env, _ = demand_parity(scn, E, steps, 100, vph, rng_seed=E)
    assert env.mean_live_vehicles() > 50
    env.close()


# ---- 2. Monaco, small_grid, Krauss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('threads', ['256', ''])
def test_monaco_vs_oracle(threads, monkeypatch):
    if threads:
        monkeypatch.setenv('TSC_ENV_THREADS', threads)
    scn = build_real_net('ma2c')
    env, _ = demand_parity(scn, 12, 400, 300, _columns(scn, 12), rng_seed=4, p_change=0.25)
    env.close()


def test_small_grid_vs_oracle():
    scn = build_small_grid('ma2c')
    env, _ = demand_parity(scn, 6, 400, 500, _columns(scn, 6), rng_seed=5, p_change=0.25)
    env.close()


def test_krauss_vs_oracle():
    scn = build_large_grid('ma2c', car_following='krauss', krauss_sigma=0.5)
    with H.oracle_krauss(0.5):
        env, _ = demand_parity(scn, 12, 120, 100, _columns(scn, 12), rng_seed=6)
    assert env.car_following() == ('krauss', 0.5)
    env.close()


# ---- 3. the benchmarked instance counts ---------------------------------------------------------------------------------
def test_benchmark_shape_large_grid():
    """E = 1024, the library's own workgroup choice; first, last and two instances per e % 8 residue against their oracles."""
    scn = build_large_grid('ma2c')
    E = 1024
    watch = sorted([0, E - 1] + [r + 8 * k for r in range(8) for k in (5 + r, 100 + 3 * r)])
    assert len(set(watch)) == 18 and all(sum(e % 8 == r for e in watch[1:-1]) == 2 for r in range(8))
    env, _ = demand_parity(scn, E, 120, 100, _columns(scn, E), watch=watch, rng_seed=7, p_random=1.0)
    env.close()


def test_benchmark_shape_monaco():
    scn = build_real_net('ma2c')
    E = 512
    watch = [0, 73, 138, 203, 268, 333, 398, E - 1]
    env, _ = demand_parity(scn, E, 120, 300, _columns(scn, E), watch=watch, rng_seed=8, p_change=0.25)
    env.close()


# ---- 4. demand really differs --------------------------------------------------------------------------------------------
def test_vehicle_counts_follow_each_instances_column():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    E = 12
    vph = _columns(scn, E)
    env = VecTrafficEnv(scn, E, seed=40)
    env.set_demand(vph)
    env.reset()
    for t in range(int(env.T)):
        env.step(env.greedy_actions())
    totals = []
    for e in range(E):
        st = env.get_state(e)
        totals.append(int(st['serial'].sum() + st['pending'].sum()))
        assert totals[e] == expected_vehicles(scn, vph[e], scn.episode_length_sec), e
    by_scale = {s: [totals[e] for e in range(E) if SCALES[e % 6] == s] for s in SCALES}
    for lo, hi in zip(SCALES[:-1], SCALES[1:]):                   # jitter 0.2 cannot bridge the gaps between these scales' sums
        assert max(by_scale[lo]) < min(by_scale[hi]), (lo, hi, by_scale)
    env.close()


# ---- 5. nominal is nominal -----------------------------------------------------------------------------------------------
def test_nominal_is_nominal():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('ma2c')
    E, steps = 6, 80
    nominal = np.tile(scn.flows[:, 2].astype(np.int32), (E, 1))
    plain = VecTrafficEnv(scn, E, seed=60, seed_stride=0)          # (stride 0: every episode of a handle runs the same seeds)
    np.testing.assert_array_equal(plain.demand(), nominal)
    ref = _episode(plain, steps, 3)
    np.testing.assert_array_equal(plain.demand(), nominal)
    env = VecTrafficEnv(scn, E, seed=60, seed_stride=0)
    # the scenario's own column, through the per-instance tables
    env.set_demand(nominal)
    np.testing.assert_array_equal(env.demand(), nominal)
    _same(_episode(env, steps, 3), ref)
    # a custom demand differs, and is reported from its reset on
    vph = _columns(scn, E)
    env.set_demand(vph)
    np.testing.assert_array_equal(env.demand(), nominal)           # not before the reset
    custom = _episode(env, steps, 3)
    np.testing.assert_array_equal(env.demand(), vph)
    assert any(not np.array_equal(x, y) for x, y in zip(custom, ref))
    # None restores the scenario's column at the next reset
    env.set_demand(None)
    np.testing.assert_array_equal(env.demand(), vph)
    _same(_episode(env, steps, 3), ref)
    np.testing.assert_array_equal(env.demand(), nominal)
    # a set_demand in the middle of an episode: the running episode is untouched, the next one has it
    def mid(t):
        if t == 30:
            env.set_demand(vph)
            np.testing.assert_array_equal(env.demand(), nominal)
    _same(_episode(env, steps, 3, mid), ref)
    _same(_episode(env, steps, 3), custom)
    np.testing.assert_array_equal(env.demand(), vph)
    # ... and back in the middle of a custom episode
    def mid2(t):
        if t == 30:
            env.set_demand(None)
    _same(_episode(env, steps, 3, mid2), custom)
    _same(_episode(env, steps, 3), ref)
    plain.close(); env.close()


# ---- 6. the recording path -----------------------------------------------------------------------------------------------
def test_recording_trace_and_lane_data_under_demand():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('greedy')
    E, steps, traced, seed0 = 6, 120, [1, 5], 70
    vph = _columns(scn, E)
    env = VecTrafficEnv(scn, E, seed=seed0)
    env.set_demand(vph)
    env.set_record(True)
    env.set_trace(traced)
    env.set_lane_data(300)
    orc = []
    for e in range(E):
        o = H.snapshot_oracle(with_rates(scn, vph[e]), seed0 + e)
        o.is_record = True
        orc.append(o)
    env.reset()
    obs = [o.reset() for o in orc]
    rng = np.random.RandomState(9)
    H.follow(env, H.oracle_steps(scn, orc, obs, steps, lambda t, obs: (rng.randint(0, 5, (E, scn.n_agent)).astype(np.int32), None)))
    ints, _ = env.read_lane_data()
    from deeprl_signal_control_amd.env import LANEDATA_INTS
    dep = []
    for e in range(E):
        want = orc[e].ms.totals()['departed']
        got_rec = sum(int(r['number_departed_car']) for r in env.traffic_data[e])
        assert got_rec == want == sum(int(r['number_departed_car']) for r in orc[e].traffic_data), e
        for a_, b_ in zip(env.traffic_data[e], orc[e].traffic_data):
            assert a_['number_departed_car'] == b_['number_departed_car'] and a_['number_total_car'] == b_['number_total_car'], (e, a_['time_sec'])
        assert int(ints[e, :, LANEDATA_INTS.index('departed'), :].sum()) == want, e
        dep.append(want + orc[e].ms.totals()['pending'])
        assert want > 100, e
    # scale 2.0 against 0.5 with jitter 0.2: every element's rate is at least 2.0 * 0.8 / (0.5 * 1.2) = 2.67 times the other's, so
    # the vehicles emitted (departed + still waiting for room) more than double, roundings included
    assert dep[5] > 2 * dep[0]
    tr = env.collect_trajectories()
    for e in traced:
        assert check_trace(scn, tr[e], orc[e].snaps) > 50
    env.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_errors_change_nothing():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('ma2c')
    E, steps = 4, 40
    nominal = np.tile(scn.flows[:, 2].astype(np.int32), (E, 1))
    plain = VecTrafficEnv(scn, E, seed=80, seed_stride=0)
    ref = _episode(plain, steps, 2)
    env = VecTrafficEnv(scn, E, seed=80, seed_stride=0)

    def refused(vph, exc, words):
        with pytest.raises(exc) as ei:
            env.set_demand(vph)
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))
    refused(nominal[:3], ValueError, ['shape'])
    refused(nominal[:, :-1], ValueError, ['shape'])
    refused(nominal.astype(np.float64), ValueError, ['integer'])
    bad = nominal.copy(); bad[2, 7] = -1
    refused(bad, RuntimeError, ['instance 2', 'flow 7', 'negative'])
    bad = nominal.copy(); bad[3, 11] = 256 * 3600                 # 256 vehicles in every second of the element
    refused(bad, RuntimeError, ['instance 3', 'flow 11', '255'])
    np.testing.assert_array_equal(env.demand(), nominal)
    _same(_episode(env, steps, 2), ref)                            # the failed calls left the nominal demand
    np.testing.assert_array_equal(env.demand(), nominal)
    # ... and a custom demand stays in force through a failed call
    vph = _columns(scn, E)
    env.set_demand(vph)
    custom = _episode(env, steps, 2)
    bad = vph.copy(); bad[0, 0] = -5
    refused(bad, RuntimeError, ['instance 0', 'flow 0'])
    _same(_episode(env, steps, 2), custom)
    np.testing.assert_array_equal(env.demand(), vph)
    # 255 vehicles in a second is allowed (the limit of tsc_env_create)
    ok = nominal.copy(); ok[1, 0] = 255 * 3600
    env.set_demand(ok)
    env.reset()
    np.testing.assert_array_equal(env.demand(), ok)
    plain.close(); env.close()


def test_sampler_handle_draws_per_episode_and_tests_run_nominal():
    """VecTrafficEnv(..., demand=sampler): train-mode resets install every instance's draw from its episode seed; test mode runs
    the scenario's own demand."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('ma2c')
    smp = DemandSampler(scn, (0.6, 0.8, 1.0, 1.2), 0.15)
    E = 8
    env = VecTrafficEnv(scn, E, seed=12, demand=smp)
    nominal = np.tile(scn.flows[:, 2].astype(np.int32), (E, 1))
    for ep in range(2):
        env.reset()
        want = [smp.draw(12 + ep * E + e) for e in range(E)]
        np.testing.assert_array_equal(env.demand(), np.stack([w[1] for w in want]))
        np.testing.assert_array_equal(env.demand_scale, [w[0] for w in want])
    env.train_mode = False
    env.reset(test_ind=1)
    np.testing.assert_array_equal(env.demand(), nominal)
    env.train_mode = True
    env.reset()
    assert not np.array_equal(env.demand(), nominal)
    env.close()
