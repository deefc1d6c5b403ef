"""Host reference rules of the kernels around the simulator step -- TEST INFRASTRUCTURE ONLY, plain numpy and Python (no GPU, no
library at import): the max-pressure rule and its hold bookkeeping, reward_sum's order, the greedy controller's rule, the integer
emission rule of the demand tables, the lane data and the trajectory rows from the oracle's vehicles after every second, the trip rows
of a handle and the record tables against a reference's.  One copy of each, written from the semantics alone; the GPU tests compare
the device with them and the host tests (tests/test_*_host.py) state on the oracle alone what those comparisons rest on.  The walks
and the comparisons of a step are in tests/env_harness.py."""
import numpy as np

INTS = ('sampledSeconds', 'waitingTime', 'departed', 'arrived', 'entered', 'left', 'laneChangedFrom', 'laneChangedTo', 'teleported')
F = {k: i for i, k in enumerate(INTS)}


# ---- controllers ------------------------------------------------------------------------------------------------------------------
def loop_pressure(scn, tb, st, measure):
    """The max-pressure rule, vehicle by vehicle over a state (get_state / ms.snapshot): -> (argmax action [A], pressure [A, PMAX])."""
    up, down = [0] * len(tb['mov']), [0] * scn.n_lane
    for l in range(scn.n_lane):
        for i in range(int(st['n'][l])):
            q = 1 if measure == 'count' else int(st['v'][l, i] < np.float32(0.1))
            down[l] += q
            mv = int(tb['lane_route_mov'][l, st['r'][l, i]])
            if mv >= 0:
                up[mv] += q
    A, PMAX = tb['n_served'].shape
    prs = np.zeros((A, PMAX), np.int32)
    act = np.zeros(A, np.int32)
    for a in range(A):
        for p in range(int(scn.agent_nphase[a])):
            prs[a, p] = sum(up[i] - down[int(tb['mov'][i, 2])] for i in tb['served'][a, p, :tb['n_served'][a, p]])
        best = 0
        for p in range(1, int(scn.agent_nphase[a])):
            if prs[a, p] > prs[a, best]:
                best = p
        act[a] = best
    return act, prs


def hold_state(E, A, g):
    """The hold's bookkeeping of a freshly armed (or reset) handle: (cur, age, last_change); the first decision is free."""
    return np.full((E, A), -1), np.full((E, A), g), np.full((E, A), -10)


def hold_update(state, e, p_star, t, g):
    """One control step of instance e's hold bookkeeping, from this step's argmax p_star [A]: -> phase changes counted (the first
    choice after arming is none)."""
    cur, age, last_change = state
    n_changes = 0
    for a in range(len(p_star)):
        if age[e, a] < g:
            age[e, a] += 1
        elif p_star[a] != cur[e, a]:
            if cur[e, a] >= 0:
                assert t - last_change[e, a] >= g, (t, e, a)
                n_changes += 1
            cur[e, a], age[e, a], last_change[e, a] = p_star[a], 1, t
        else:
            age[e, a] += 1
    return n_changes


def instance_sum(per_step_g):
    """reward_sum as the library documents it: per instance in step order, then the instances in order."""
    acc = np.zeros(per_step_g[0].shape, np.float64)
    for g in per_step_g:
        acc = acc + g
    tot = 0.0
    for v in acc:
        tot += float(v)
    return tot


def greedy_rule(tables, ob):
    """The greedy controller's rule as Scenario.greedy_controller_tables states it, for one agent: tables = (its term rows [GC, GT],
    its action row [GC], its candidate count), ob its float64 observation.  Per candidate the terms are added in table order, in
    float64, from 0.0; the first maximum wins.  -> (action, flows)."""
    term, action, n_cand = tables
    flows = []
    for c in range(int(n_cand)):
        flow = 0.0
        for j in term[c]:
            if j < 0:
                break
            flow = flow + float(ob[j])
        flows.append(flow)
    best = 0
    for c in range(1, len(flows)):
        if flows[c] > flows[best]:
            best = c
    return int(action[best]), flows


# ---- demand -----------------------------------------------------------------------------------------------------------------------
def expected_vehicles(scn, vph, seconds):
    """Vehicles the integer rule emits in seconds [0, seconds): element f has emitted ceil(tau vph / 3600) after tau seconds."""
    b, en = scn.flows[:, 0].astype(np.int64), scn.flows[:, 1].astype(np.int64)
    tau = np.clip(np.minimum(en, seconds) - b, 0, None)
    return int(((tau * vph.astype(np.int64) + 3599) // 3600).sum())


# ---- lane data --------------------------------------------------------------------------------------------------------------------
def lane_data_reference(scn, snaps, period):
    """The lane data of one instance from the oracle's vehicles after every second (snaps[t]: the end of second t), written from
    the semantics alone: raw per-slot sums ints [n_interval, 9, n_slot] and speed [n_interval, n_slot].  A vehicle's slot is the
    lane's last piece whose start (float64, cumulated over the pieces before it) is <= x; events compare a vehicle id's slot at
    the end of t - 1 with its slot at the end of t."""
    tabs = scn.lane_data_slots()
    slot0, sumo = tabs['slot0'], tabs['sumo']
    n_slot, T = int(slot0[-1]), int(scn.episode_length_sec)
    n_int = -(-T // period)
    starts = []
    for ps in scn.lane_pieces:
        off, st = 0.0, []
        for _, _, ln in ps:
            st.append(off)
            off += ln
        starts.append(st)
    sib = None if scn.lane_sib is None else np.asarray(scn.lane_sib)
    mv_next = np.asarray(scn.mv_next).reshape(scn.n_lane, -1)
    ints = np.zeros((n_int, len(INTS), n_slot), np.int64)
    speed = np.zeros((n_int, n_slot), np.float64)
    halt = np.float32(0.1)
    prev = {}
    for t, sn in enumerate(snaps):
        assert t < T
        k = t // period
        lanes = np.repeat(np.arange(scn.n_lane), sn['n'])
        cur, per_sec = {}, np.zeros(n_slot, np.float64)
        slots = []
        for oid, l, x, v, r in zip(sn['id'].tolist(), lanes.tolist(), sn['x'], sn['v'], sn['r'].tolist()):
            st, j = starts[l], 0
            while j + 1 < len(st) and float(x) >= st[j + 1]:
                j += 1
            s = int(slot0[l]) + j
            slots.append(s)
            cur[oid] = (l, s, r)
            ints[k, F['sampledSeconds'], s] += 1
            if v < halt:
                ints[k, F['waitingTime'], s] += 1
            per_sec[s] += float(v)
        if len(lanes):                 # the slot's SUMO lane is the one Scenario.sumo_lane_pos (pinned by the FCD tests) names
            names = np.array(tabs['names'], dtype=object)[sumo[np.array(slots)]]
            np.testing.assert_array_equal(names, scn.sumo_lane_pos(lanes, sn['x'].astype(np.float64))[0])
        speed[k] = speed[k] + per_sec
        for oid, (l, s, r) in cur.items():
            if oid not in prev:
                ints[k, F['departed'], s] += 1
                continue
            lo, so, _ = prev[oid]
            if sib is not None and sib[lo] == l:
                ints[k, F['laneChangedFrom'], so] += 1
                ints[k, F['laneChangedTo'], s] += 1
            elif sumo[so] != sumo[s]:
                ints[k, F['left'], so] += 1
                ints[k, F['entered'], s] += 1
        for oid, (lo, so, r) in prev.items():
            if oid not in cur:
                ints[k, F['arrived' if mv_next[lo, r] == -1 else 'teleported'], so] += 1
        prev = cur
    return ints, speed


def lane_data_merge(scn, ints, speed):
    """Per SUMO lane (by name): integer sums and the speed sums added in slot order from 0.0, [n_interval, n_sumo_lane]."""
    tabs = scn.lane_data_slots()
    names = tabs['names']
    out_i = np.zeros((ints.shape[0], len(INTS), len(names)), np.int64)
    out_s = np.zeros((ints.shape[0], len(names)), np.float64)
    for s, j in enumerate(tabs['sumo'].tolist()):
        out_i[:, :, j] += ints[:, :, s]
        out_s[:, j] = out_s[:, j] + speed[:, s]
    return out_i, out_s


def check_lane_data(scn, env, orc, period):
    """read_lane_data and collect_lane_data of a handle against lane_data_reference / lane_data_merge over the snapshots of the
    oracles {instance: snaps, ms.totals()} -> {instance: {field: its sum}}."""
    ints, speed = env.read_lane_data()
    cols = env.collect_lane_data()
    n_sumo = len(scn.lane_data_slots()['names'])
    for e, o in orc.items():
        ri, rs = lane_data_reference(scn, o.snaps, period)
        assert ri.sum() > 0
        np.testing.assert_array_equal(ints[e], ri, err_msg='instance %d' % e)
        np.testing.assert_array_equal(speed[e].view(np.uint64), rs.view(np.uint64), err_msg='instance %d' % e)
        mi, ms = lane_data_merge(scn, ri, rs)
        for f, k in enumerate(INTS):
            np.testing.assert_array_equal(cols[e][k].reshape(-1, n_sumo), mi[:, f, :], err_msg='%s, instance %d' % (k, e))
        np.testing.assert_array_equal(cols[e]['speed_sum'].reshape(-1, n_sumo).view(np.uint64), ms.view(np.uint64))
        # the oracle's own counters: the test's classification of the disappearances is the simulator's
        tot = o.ms.totals()
        assert ri[:, F['arrived']].sum() == tot['arrived'], (e, tot)
        assert ri[:, F['teleported']].sum() == tot['teleported'], (e, tot)
    return {e: {k: int(ints[e, :, f].sum()) for f, k in enumerate(INTS)} for e in orc}


# ---- trajectories, trips, record tables -------------------------------------------------------------------------------------------
def check_trace(scn, tr, snaps, by_entry_lane=False):
    """Rows of every second (time_sec = second + 1) == the oracle's vehicles in (lane, slot) order; oracle id <-> (route, serial)
    one bijection over the whole run.  by_entry_lane: serials count per insertion stream, so where several streams share a route
    (the synthetic networks of tests/networks.py) the key is (route, serial, the lane the vehicle was first seen on -- its
    stream's entry lane).  -> the vehicles seen."""
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


def device_trips(env, e):
    """The trip rows of instance e of a recording handle (tsc_env_read_trips), int32 [n, 6]."""
    import ctypes as C
    from deeprl_signal_control_amd import _lib
    cap = 16384
    buf = np.zeros((cap, 6), np.int32)
    cnt = C.c_int32()
    _lib.check(env._L.tsc_env_read_trips(env._h, e, buf.ctypes.data_as(C.c_void_p), cap, C.byref(cnt)))
    return buf[:min(cnt.value, cap)]


def assert_trips_equal(got, ref, msg=''):
    """Trip rows (route, serial, depart, arrival, waiting seconds, waiting count) as sets: both sorted by all six columns."""
    key = lambda a: a[np.lexsort(a.T[::-1])]
    np.testing.assert_array_equal(key(got), key(ref), err_msg=msg)


def check_record_tables(g, traffic, control, trips, least_trips=101):
    """The per-second rows, the control rows and the trip table of a recording env against the arrays g['traffic_*'],
    g['control_*'], g['trip_*'] of a reference: integers and strings exactly, float means to 1e-12 (np.mean's pairwise sum against
    the per-lane partial sums).  least_trips: the fewest finished trips the run must show (the comparison is not vacuous)."""
    for k in ('episode', 'time_sec', 'number_total_car', 'number_departed_car', 'number_arrived_car'):
        np.testing.assert_array_equal(np.array([r[k] for r in traffic]), g['traffic_' + k], err_msg=k)
    for k in ('avg_wait_sec', 'avg_speed_mps', 'std_queue', 'avg_queue'):
        np.testing.assert_allclose(np.array([r[k] for r in traffic], np.float64), g['traffic_' + k], rtol=1e-12, atol=1e-12, err_msg=k)
    for k in ('episode', 'time_sec', 'step', 'reward'):
        np.testing.assert_array_equal(np.array([r[k] for r in control]), g['control_' + k], err_msg=k)
    assert [r['action'] for r in control] == list(g['control_action'])
    want = sorted(zip(*(g['trip_' + k] for k in ('arrival_sec', 'id', 'depart_sec', 'duration_sec', 'wait_step', 'wait_sec'))),
                  key=lambda t: (float(t[0]), t[1]))
    got = sorted(((r['arrival_sec'], r['id'], r['depart_sec'], r['duration_sec'], r['wait_step'], r['wait_sec']) for r in trips),
                 key=lambda t: (float(t[0]), t[1]))
    assert len(got) == len(want) >= least_trips and got == [tuple(str(x) for x in t) for t in want]
    assert all(r['episode'] == 1 for r in trips)
