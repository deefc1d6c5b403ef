"""The kernels around the step -- pressure_kernel, pressure_reward_kernel, greedy_kernel, fixed_time_kernel, demand_kernel and the trace
and lane-data branches of the recording walk (csrc/tsc_env.hip) -- on the synthetic networks of tests/networks.py, against the host
references the built-in scenarios' tests already use (tests/env_rules.py, tests/env_harness.py): loop_pressure, trainer.pressure_reward,
the greedy rule as Scenario.greedy_controller_tables states it, lane_data_reference / check_trace over the oracle's vehicles after
every second, demand_parity and expected_vehicles.  The runs are the rows of networks.AUX; tests/test_networks_aux_host.py states, on the oracle alone, what
each of them reaches (pressure_walk with two and three lanes per thread and a second round of the flat walk, more than 256 agents,
ties, clipped entries, every lane-data field, the partial last interval, partly covered 4-second words).

Nothing here has a tolerance: integers, or the bit patterns of float32 / float64.

No test asks for the 48 KiB refusals of tsc_env_set_pressure / tsc_env_set_reward_pressure: they cannot be reached.  The kernels need
4 x (2 n_walk + 1 + n_mov + 256 + A x PMAX) bytes, and under the other limits -- 1024 lanes, 4096 movements, 4096 (agent, phase)
pairs -- that is at most 4 x (2048 + 1 + 4096 + 256 + 4096) = 41,988 B."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import env_harness as H
from tests import networks as nw
from tests.env_harness import assert_same as _same, demand_parity as _parity, episode_outputs as _episode
from tests.env_rules import (check_lane_data, check_trace, expected_vehicles as _expected_vehicles, greedy_rule, hold_state, hold_update,
                             instance_sum, loop_pressure)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _library_chooses_the_plan(monkeypatch):
    for k in ('TSC_ENV_THREADS', 'TSC_ENV_KF', 'TSC_ENV_HELP', 'TSC_ENV_SPEC'):
        monkeypatch.delenv(k, raising=False)


def _device(case, **kw):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    net = case.net()
    return VecTrafficEnv(case.scenario(), case.E, seed=net.seed, test_seeds=H.eval_seeds(net, case.E), **kw)


def _follow(case, dev):
    """The device beside the oracles of an AUX case: steps `dev` through run_oracle's actions and yields (t, the device's step
    result (t = -1: the reset observation), the oracle's results, the oracles) after every control step."""
    for t, acts, pols, res, orc in nw.aux_run(case):
        if t < 0:
            yield t, dev.reset(), res, orc
            continue
        if pols is not None:
            dev.update_fingerprint(H.upload(dev, pols))
        yield t, dev.step(H.upload(dev, acts)), res, orc


# ---- max-pressure controller ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.AUX['pressure'], ids=repr)
def test_pressure_vs_loop(case):
    """Actions and the full pressure array of both measures against the rule, vehicle by vehicle over the oracle's state, every
    few control steps and at the entry's peak."""
    scn, tb = case.scenario(), case.scenario().pressure_tables()
    dev = _device(case)
    try:
        compared = 0
        for t, out, res, orc in _follow(case, dev):
            if t < 0 or not case.compared(t):
                continue
            for measure in ('count', 'queue'):
                act, prs = dev.max_pressure_actions(measure=measure, return_pressure=True)
                act, prs = act.cpu().numpy(), prs.cpu().numpy()
                for e in range(case.E):
                    want_act, want_prs = loop_pressure(scn, tb, orc[e].ms.snapshot(), measure)
                    np.testing.assert_array_equal(prs[e], want_prs, err_msg='%s t=%d e=%d' % (measure, t, e))
                    np.testing.assert_array_equal(act[e], want_act, err_msg='%s t=%d e=%d' % (measure, t, e))
            compared += 1
        assert compared >= 4
    finally:
        dev.close()


def test_pressure_hold_with_more_than_256_agents():
    """min_green = 3 on isolated_300: the hold state [E][A][2] of 300 agents, with the bookkeeping of tests/test_pressure_gpu.py's
    test_hold, and the free decision after reset()."""
    case = nw.AUX['hold']
    scn, tb, g = case.scenario(), case.scenario().pressure_tables(), case.min_green
    E, A = case.E, scn.n_agent
    dev = _device(case)
    try:
        for _ in _follow(case, dev):                            # some traffic first (the hold is not armed yet)
            pass
        state = hold_state(E, A, g)
        cur, age, _ = state
        t, n_changes = 0, 0
        while t < case.least or not ((age < g) & (cur != 0)).any():
            assert t < case.most, 'no agent inside a hold on a phase other than 0'
            act = dev.max_pressure_actions(min_green=g)
            act_h = act.cpu().numpy()
            for e in range(E):
                p_star, _ = loop_pressure(scn, tb, dev.get_state(e), 'count')
                n_changes += hold_update(state, e, p_star, t, g)
            np.testing.assert_array_equal(act_h, cur, err_msg='t=%d' % t)
            dev.step(act)
            t += 1
        assert n_changes > 10 and (cur[:, 256:] != 0).any()
        dev.reset()                                             # frees the first decision: the empty network's argmax, phase 0
        act = dev.max_pressure_actions(min_green=g).cpu().numpy()
        assert (act == 0).all()
        dev.step(torch.from_numpy(act).cuda())
    finally:
        dev.close()


def test_pressure_4096_movements_and_one_more():
    """The movement limit through hand-made tables: merge4_yield's own movements plus copies of its first row up to n_mov = 4096,
    which the phases that serve the row serve too.  No (lane, route) names a copy, so its `up` is 0 and it adds -down(its
    downstream lane): accepted, and equal to the loop over the same tables.  4097 movements are refused, and the handle goes on
    answering with the 4096."""
    from deeprl_signal_control_amd import _lib
    case = nw.Aux('merge4_yield', 'merge4_yield', 2, 30)
    scn, tb = case.scenario(), case.scenario().pressure_tables()
    n_real = len(tb['mov'])
    a0 = int(tb['mov'][0, 0])
    ip = C.POINTER(C.c_int32)

    def tables(n_mov):
        mov = np.concatenate([tb['mov'], np.tile(tb['mov'][:1], (n_mov - n_real, 1))]).astype(np.int32)
        copies = np.arange(n_real, n_mov, dtype=np.int32)
        A, PMAX, SRV = tb['served'].shape
        served = np.full((A, PMAX, SRV + len(copies)), -1, np.int32)
        n_served = tb['n_served'].copy()
        served[:, :, :SRV] = tb['served']
        for p in range(int(scn.agent_nphase[a0])):
            if 0 in tb['served'][a0, p, :n_served[a0, p]].tolist():
                served[a0, p, n_served[a0, p]:n_served[a0, p] + len(copies)] = copies
                n_served[a0, p] += len(copies)
        return dict(mov=mov, lane_route_mov=np.ascontiguousarray(tb['lane_route_mov'], np.int32), served=served, n_served=n_served)

    dev = _device(case)
    try:
        for _ in _follow(case, dev):
            pass

        def arm(t_):
            return dev._L.tsc_env_set_pressure(dev._h, 0, 1, len(t_['mov']), t_['mov'].ctypes.data_as(ip), t_['lane_route_mov'].ctypes.data_as(ip),
                                               t_['served'].shape[2], t_['served'].ctypes.data_as(ip))

        def answer():
            act = torch.empty(case.E, scn.n_agent, dtype=torch.int32, device='cuda')
            prs = torch.empty(case.E, scn.n_agent, scn.green_tab.shape[1], dtype=torch.int32, device='cuda')
            _lib.check(dev._L.tsc_env_pressure_actions(dev._h, C.c_void_p(act.data_ptr()), C.c_void_p(prs.data_ptr())))
            return act.cpu().numpy(), prs.cpu().numpy()

        full = tables(4096)
        assert full['n_served'].max() >= 4092
        _lib.check(arm(full))
        want = [loop_pressure(scn, full, dev.get_state(e), 'count') for e in range(case.E)]
        plain = [loop_pressure(scn, tb, dev.get_state(e), 'count') for e in range(case.E)]
        assert any(not np.array_equal(w[1], p[1]) for w, p in zip(want, plain))          # the copies count
        for again in range(2):
            act, prs = answer()
            for e in range(case.E):
                np.testing.assert_array_equal(prs[e], want[e][1], err_msg='e=%d' % e)
                np.testing.assert_array_equal(act[e], want[e][0], err_msg='e=%d' % e)
            if again == 0:
                with pytest.raises(RuntimeError, match='4097 movements, .* at most 4096 each'):
                    _lib.check(arm(tables(4097)))
    finally:
        dev.close()


# ---- pressure reward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.AUX['reward'], ids=repr)
def test_pressure_reward_vs_host(case):
    """reward, global_reward and reward_sum against trainer.pressure_reward over the oracle's state: 130 MA2C agents with ring
    neighbours, 300 agents, test mode, and the control log of a recording handle."""
    from deeprl_signal_control_amd.trainer import pressure_reward
    scn = case.scenario()
    dev = _device(case)
    try:
        dev.set_reward_pressure(case.measure)
        if case.record:
            dev.set_record(True)
        gs, compared = [], 0
        for t, out, res, orc in _follow(case, dev):
            if t < 0:
                dev.train_mode = case.train_mode                # (what step() hands to tsc_env_step; the seeds are the train-mode ones)
                continue
            _, reward, _, g = out
            gs.append(g.cpu().numpy().copy())
            if not case.compared(t):
                continue
            r_h = reward.cpu().numpy()
            for e in range(case.E):
                want_r, want_g, _ = pressure_reward(scn, orc[e].ms.snapshot(), case.measure, train_mode=case.train_mode)
                np.testing.assert_array_equal(r_h[e], want_r, err_msg='t=%d e=%d' % (t, e))
                assert gs[-1][e] == want_g, (t, e)
            compared += 1
        total = dev.reward_sum()
        assert compared >= 4 and total == instance_sum(gs) and total < 0
        if case.record:
            for e in range(case.E):
                assert [row['reward'] for row in dev.control_data[e]] == [float(g[e]) for g in gs]     # the control log holds the pressure g
    finally:
        dev.close()


# ---- greedy controller ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.AUX['greedy'], ids=repr)
def test_greedy_vs_rule_on_the_oracles_observations(case):
    """greedy_actions on the device's float32 observations == the rule on the oracle's float64 observations, after the reset and
    every control step of the entry's run."""
    scn = case.scenario()
    n_cand, term, action = scn.greedy_controller_tables()
    dev = _device(case)
    try:
        for t, out, res, orc in _follow(case, dev):
            obs = out if t < 0 else out[0]
            obs64 = res if t < 0 else [r[0] for r in res]
            got = dev.greedy_actions(obs).cpu().numpy()
            want = np.array([[greedy_rule((term[a], action[a], n_cand[a]), obs64[e][a])[0] for a in range(scn.n_agent)]
                             for e in range(case.E)], np.int32)
            np.testing.assert_array_equal(got, want, err_msg='t=%d' % t)
    finally:
        dev.close()


@pytest.mark.parametrize('norm,clip', nw.GREEDY_NORMS)
def test_greedy_recovers_the_float64_rule_from_every_count_tuple(norm, clip):
    """Agent 0 of merge4 under networks.GREEDY_PHASES, every tuple of 0 .. 8 vehicles on its four lanes as float32 observation rows
    min(c / norm, clip): the action is the float64 rule's over the counts -- also where the float32 entries, added up as they are,
    would pick another one (3 / 5 against 1 / 5 + 2 / 5), and on clipped entries."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn, counts, ob32, want, naive64, naive32 = nw.greedy_exhaustive(norm, clip)
    assert (want != naive64).any() and (ob32 == np.float32(clip)).any()
    E = 729
    dev = VecTrafficEnv(scn, E, seed=1)
    try:
        got = np.zeros(len(counts), np.int32)
        for i in range(0, len(counts), E):
            obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
            obs[:, 0, :4] = ob32[i:i + E]
            got[i:i + E] = dev.greedy_actions(torch.from_numpy(obs).cuda()).cpu().numpy()[:, 0]
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, 'counts %s: %d, the rule says %d (%d tuples differ)' % (counts[bad[0]].tolist(), got[bad[0]], want[bad[0]], len(bad))
    finally:
        dev.close()


# ---- fixed time -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.AUX['fixed'], ids=lambda c: '%s-%d' % (c.key, c.s))
def test_fixed_time(case):
    """(t // s) % n_phase with t = tsec / control interval: more than one block of (instance, agent) threads on isolated_300, an
    8 s control interval on ctrl8; again after a reset."""
    scn = case.scenario()
    dev = _device(case)
    try:
        assert case.E * scn.n_agent > 256 or scn.control_interval_sec == 8
        for episode in range(2):
            dev.reset()
            for t in range(case.steps):
                act = dev.fixed_time_actions(case.s)
                want = np.tile((t // case.s) % np.asarray(scn.agent_nphase), (case.E, 1))
                np.testing.assert_array_equal(act.cpu().numpy(), want, err_msg='episode %d t=%d' % (episode, t))
                dev.step(act)
    finally:
        dev.close()


# ---- trace and lane data --------------------------------------------------------------------------------------------------
def _walk(case, lane_data=True):
    """One handle with the trace (and the lane data) armed beside the snapshot oracles of the watched instances, over the case's
    control steps: -> (vehicles per traced instance, the lane data's sums per instance)."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = case.scenario()
    dev = VecTrafficEnv(scn, case.E, seed=case.seed)
    try:
        dev.set_record(True)
        dev.set_trace(case.watch)
        if lane_data:
            dev.set_lane_data(case.period)
        with H.walk_context(case):
            orc = H.WalkOracles(case)
            dev.reset()
            rng = np.random.RandomState(case.rng_seed)
            for _ in range(nw.walk_steps(case)):
                acts = H.uniform_actions(scn, rng, case.E)
                dev.step(torch.from_numpy(acts).cuda())
                orc.step(acts)
        views = orc.views()
        tr = dev.collect_trajectories()
        assert sorted(tr) == sorted(case.watch)
        ids = {e: check_trace(scn, tr[e], views[e].snaps, by_entry_lane=True) for e in case.watch}
        sums = check_lane_data(scn, dev, views, case.period) if lane_data else None
        return ids, sums
    finally:
        dev.close()


@pytest.mark.parametrize('case', nw.AUX['walk'], ids=repr)
def test_trace_and_lane_data_vs_oracle(case):
    """Both on one handle, to the end of the episode (grid_x2: 60 steps): every second's trajectory rows and every slot's sums of
    every interval, the partial last one included, equal the oracle's vehicles."""
    ids, sums = _walk(case)
    assert min(ids.values()) > 50
    assert min(s['departed'] for s in sums.values()) > 50 and min(s['arrived'] for s in sums.values()) > 0
    if case.key == 'burst':
        assert min(s['teleported'] for s in sums.values()) > 0
    if case.key == 'merge4_pieces':
        assert min(s['entered'] for s in sums.values()) > 0
    if case.key == 'grid_x2':
        assert min(s['laneChangedFrom'] for s in sums.values()) > 0


def test_trace_with_254_streams():
    """The traced recording walk at 512 threads with 254 insertion streams (its LDS need, by smem_layout: 101,504 B + 22,560 B of
    recording arrays, fits)."""
    ids, _ = _walk(nw.AUX['trace254'], lane_data=False)
    assert min(ids.values()) > 254


def test_recording_is_refused_on_grid_x4_and_the_handle_goes_on():
    """grid_x4 is the largest tile that fits without recording, and recording does not fit.  By smem_layout (every array rounded up
    to 16 B; NLA = 384, NLP = 768, NU = 332, NR = 48, A = 100, KMAX = 12, NS = 48, 28 slots per lane, 4 crossings):
      r 816 + mv 63,744 + six lane summaries 9,216 + five outbox arrays 30,720 + nout 1,536 + three detector arrays 9,216 + link
      states 2,400 + len / vmax / node / sib 6,144 + pend / ser / emit 768 + zip 15,936 + up4 1,536 + pre 1,536 + wtot 64 + mark
      10,384 + bound 352 + nc / seed 3,072 + wtail 128 + hz 16 = 157,584 B;
      recording adds or0 / or1 12,288 + rq 1,536 + rsp 3,072 + rint 32 = 16,928 B: 174,512 B > 163,840 B.
    set_record(True) is refused with that figure, and the handle steps on, without recording, bit-equal to the oracle."""
    case = nw.Aux('grid_x4', 'grid_x4', 2, 20)
    scn = case.scenario()
    dev = _device(case)
    try:
        with pytest.raises(RuntimeError, match='tsc_env_record: LDS need 174512 B > 160 KiB'):
            dev.set_record(True)
        assert not getattr(dev, 'is_record', False)
        for t, out, res, orc in _follow(case, dev):
            if t < 0:
                got = dev.step_plan()
                assert got['row'] + (got['threads'],) == tuple(nw.NETWORKS['grid_x4'].plan) and got['lds_bytes'] == 157584, got
                continue
            H.assert_step_equal(scn, t, [x.cpu().numpy() for x in out], res)
        H.assert_state_equal(dev, orc, range(case.E), t)
    finally:
        dev.close()


# ---- per-instance demand --------------------------------------------------------------------------------------------------
def test_demand_windows_vs_oracle_and_per_second_counts():
    """windows() with a column per instance (networks.windows_columns: the scenario's own, exactly 255 vehicles in a second, redrawn
    rates, bounds that add up to 256 with no second above 255 -- all accepted): parity with OracleEnv(replace(flows)), then, in a
    second episode, after every simulated second the vehicles emitted so far (inserted + pending) are the integer rule's."""
    case = nw.AUX['demand']
    scn = case.scenario()
    vph = nw.windows_columns(scn)
    env, _ = _parity(scn, case.E, case.steps, case.seed, vph, rng_seed=11)
    try:
        env.reset()
        np.testing.assert_array_equal(env.demand(), vph)
        rng = np.random.RandomState(12)
        for t in range(case.steps):
            env.step(torch.from_numpy(H.uniform_actions(scn, rng, case.E)).cuda())
            for e in range(case.E):
                st = env.get_state(e)
                assert int(st['t'][0]) == t + 1
                assert int(st['serial'].sum() + st['pending'].sum()) == _expected_vehicles(scn, vph[e], t + 1), (t, e)
        assert _expected_vehicles(scn, vph[1], 84) - _expected_vehicles(scn, vph[1], 82) == 2 * 255
    finally:
        env.close()


def test_demand_256_in_a_second_is_refused_and_changes_nothing():
    from deeprl_signal_control_amd.env import VecTrafficEnv
    case = nw.AUX['demand']
    scn = case.scenario()
    vph = nw.windows_columns(scn)
    col, flow, second = nw.windows_refused_column(scn)
    E, steps = case.E, 100
    plain = VecTrafficEnv(scn, E, seed=case.seed + 50, seed_stride=0)
    env = VecTrafficEnv(scn, E, seed=case.seed + 50, seed_stride=0)
    try:
        plain.set_demand(vph)
        env.set_demand(vph)
        ref = _episode(plain, steps, 2)
        bad = vph.copy()
        bad[2] = col
        with pytest.raises(RuntimeError) as ei:
            env.set_demand(bad)
        for w in ('instance 2', 'flow %d' % flow, 'second %d' % second, '255'):
            assert w in str(ei.value), (w, str(ei.value))
        _same(_episode(env, steps, 2), ref)                     # the handle keeps the demand it had
        np.testing.assert_array_equal(env.demand(), vph)
    finally:
        plain.close(); env.close()


def test_demand_with_254_streams():
    """set_demand on isolated_254, E = 3: demand_kernel on a 254 x 3 grid; observations and rewards at every step and the vehicle
    state at the end equal the oracles of the three columns."""
    case = nw.AUX['demand254']
    scn = case.scenario()
    env, _ = _parity(scn, case.E, case.steps, case.seed, nw.demand254_columns(scn, case.E), rng_seed=13)
    env.close()
