"""The generated networks with two-lane streets of tests/networks.py (random_street_network, RANDOM_STREET_SEEDS,
RANDOM_STREET_VARIANT_SEEDS) on the host (no GPU, no library): every network is run through the CPU oracle alone, over the very (E,
steps, actions, seeds) tests/test_streets_gpu.py compares, and what makes the sample worth running is stated as floors -- networks of
the 48 in which a clause of MICROSIM_SPEC.md rule 10 is reached.  The floors are conditions on the inputs: a changed generator or
seed list that stops meeting them fails here, not silently on the GPU.  One oracle walk per network (survey), shared by every test.

An event is found in Python from the state BEFORE a second (the rule reads old state only) and, where it is about what a vehicle did,
from where the oracle's vehicle ids are after it: a vehicle that stood on lane l and stands on lane_sib[l] has changed.

How sharp the 48 runs are was measured once with patched copies of oracle/microsim.c (not kept): each mutant runs as the stand-in
handle of tests/test_env_harness_host.py under the true oracle's actions, through env_harness.follow (every step, the vehicle state at
the peak and at the end, the counters).  Networks of the 48 that report a difference:
    room test n + 2 MAX_CROSS <= CAP -> n + MAX_CROSS <= CAP                    17
    gap test without the closing-speed term dv                                  30
    third leader removed                                                        42
    junction arrivals gathered before lane changers                             23
    ncross < MAX_CROSS dropped for changes                                      14
    teleport condition (tl >= 0 || sb >= 0) -> tl >= 0                          24
    clamp behind the sibling's old tail dropped for changers                     5
    mv_next[sib][r] >= -1 -> >= 0                                               34
(the unchanged oracle as the stand-in: 0).  The clamp is the rarest: it binds for a changer behind a vehicle that has just left
the lane, with the sibling's tail a few metres ahead -- which is why the lane on which the most routes end is always a street.

One event the sweep cannot reach, by rule 10 itself: changes in BOTH directions on one street in one second (see
test_no_street_carries_changes_in_both_directions_in_one_second); the floor for both directions counts runs.
"""
import ctypes as C

import numpy as np

from tests import env_harness as H
from tests import networks as nw

LEN, S0, ACC, DEC, THEAD, ICAB = (np.float32(x) for x in (5.0, 2.0, 5.0, 10.0, 1.0, 0.070710678))
CAP, MAX_CROSS = 28, 4
_survey = {}


def follow(v, v0, lead, g=0.0, vl=0.0, s0gap=0.0):
    """MICROSIM_SPEC.md rule 3 (the IDM step against one leader) in float32, operation for operation as oracle/microsim.c."""
    f = np.float32
    v, v0, g, vl, s0gap = f(v), f(v0), f(g), f(vl), f(s0gap)
    ratio = f(v / v0)
    r2 = f(ratio * ratio)
    acc = f(ACC * f(f(1.0) - f(r2 * r2)))
    vsafe = f(np.inf)
    if lead:
        sstar = f(f(S0 + f(v * THEAD)) + f(f(v * f(v - vl)) * ICAB))
        sstar = max(sstar, S0)
        s = max(g, f(0.5))
        q = f(sstar / s)
        acc = f(acc - f(ACC * f(q * q)))
        gs = max(f(g - s0gap), f(0.0))
        vsafe = f(np.sqrt(f(f(f(DEC * DEC) + f(vl * vl)) + f(f(f(2.0) * DEC) * gs))) - DEC)
    acc = max(acc, f(-DEC))
    vn = f(v + acc)
    vn = min(vn, vsafe)
    if vn > v0 and v <= v0:
        vn = v0
    return max(vn, f(0.0))


class _Lanes:
    """Every lane's vehicles of an oracle through its own C getter, with buffers allocated once."""

    def __init__(self, ms, NL):
        self.ms, self.NL, cap = ms, NL, ms.cap
        self.x, self.v, self.sf = (np.zeros(cap, np.float32) for _ in range(3))
        self.w, self.r, self.i = (np.zeros(cap, np.int32) for _ in range(3))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self.args = (self.x.ctypes.data_as(fp), self.v.ctypes.data_as(fp), self.w.ctypes.data_as(ip), self.r.ctypes.data_as(ip),
                     self.i.ctypes.data_as(ip), self.sf.ctypes.data_as(fp))

    def read(self):
        """Per lane a list of (id, x, v, w, route, sf), head first."""
        out = []
        for l in range(self.NL):
            n = self.ms.L.ms_lane_vehicles(self.ms.h, l, *self.args)
            out.append(list(zip(self.i[:n].tolist(), self.x[:n].copy(), self.v[:n].copy(), self.w[:n].tolist(), self.r[:n].tolist(),
                                self.sf[:n].copy())))
        return out


EVENTS = ('room_only', 'gap_only', 'closing', 'third', 'teleport', 'both_sources', 'both_ways', 'both_ways_second', 'two_leave', 'short',
          'fast', 'unsignalised', 'entry_wrong', 'ends', 'two_feeders', 'vmax_differ')


def survey(seed):
    """The oracle's run of random_street_network(seed) -> dict of what the scenario is and of the events of rule 10 its run
    reaches (the floor table of test_coverage_floors).  Built once per seed."""
    if seed in _survey:
        return _survey[seed]
    net = nw.random_street_network(seed)
    scn = net.scenario()
    NL, E = scn.n_lane, net.E
    length, vmax, node, sib = (np.asarray(x) for x in (scn.lane_len, scn.lane_vmax, scn.lane_node, scn.lane_sib))
    nxt = np.asarray(scn.mv_next)
    junction = [[int(u) for u in scn.lane_up[l] if u >= 0 and u != sib[l]] for l in range(NL)]
    entry = {int(l) for l in scn.stream_entry_lane}
    teleport = int(scn.teleport_sec)
    ev = {k: False for k in EVENTS}
    changes, lanes, old, born, sources = [0] * E, {}, {}, [dict() for _ in range(E)], [dict() for _ in range(E)]
    ever = [set() for _ in range(E)]                                # the lanes a changer has left so far

    def wrong(l, r):
        return sib[l] >= 0 and nxt[l, r] < -1 and nxt[sib[l], r] >= -1

    def before(e, st):
        """The refusals and the third leader of the lanes' heads, from the old state alone (i = 0: nothing has left the lane)."""
        for l in range(NL):
            if not st[l] or not wrong(l, st[l][0][4]):
                continue
            _, x, v, w, r, sf = st[l][0]
            sb = int(sib[l])
            room = len(st[sb]) + 2 * MAX_CROSS <= CAP
            gap = True
            if st[sb]:
                _, tx, tv = st[sb][-1][:3]
                dv = max(np.float32(v - tv), np.float32(0.0))
                gap = np.float32(np.float32(tx - LEN) - x) >= np.float32(S0 + dv)
            ev['room_only'] |= gap and not room
            ev['gap_only'] |= room and not gap
            if not (room and gap) and st[sb] and w < teleport:
                g3 = np.float32(np.float32(st[sb][-1][1] - LEN) - x)
                if g3 >= 0:
                    v0 = np.float32(np.float32(vmax[l]) * sf)
                    vn = min(follow(v, v0, False), follow(v, v0, True, np.float32(np.float32(length[l]) - x)))
                    ev['third'] |= follow(v, v0, True, g3, st[sb][-1][2], S0) < vn

    def after(e, st, new):
        where = {vid: l for l in range(NL) for vid, *_ in new[l]}
        left, got = {}, {}
        for l in range(NL):
            for i, (vid, x, v, w, r, sf) in enumerate(st[l]):
                l2 = where.get(vid)
                if l2 is None:
                    ev['teleport'] |= i == 0 and wrong(l, r) and w >= teleport
                elif l2 != l:
                    got.setdefault(l2, set()).add(l)
                    if l in junction[l2]:
                        sources[e].setdefault(l2, set()).add(l)
                    if l2 == sib[l]:
                        changes[e] += 1
                        left[l] = left.get(l, 0) + 1
                        tail = st[l2][-1] if st[l2] else None
                        ev['closing'] |= tail is not None and v - tail[2] > 0
                        ev['short'] |= length[l] < 50.0
                        ev['fast'] |= vmax[l] > length[l]
                        ev['unsignalised'] |= node[l] < 0
                        ev['entry_wrong'] |= l in entry and born[e].get(vid) == l
                        ev['ends'] |= nxt[l2, r] == -1
                        ev['vmax_differ'] |= vmax[l] != vmax[l2]
        for l2, src in got.items():
            ev['both_sources'] |= sib[l2] in src and len(src) >= 2
        ev['both_ways_second'] |= any(int(sib[l]) in left for l in left)
        ever[e] |= set(left)
        ev['both_ways'] |= any(int(sib[l]) in ever[e] for l in left)
        ev['two_leave'] |= any(n >= 2 for n in left.values())
        for l in range(NL):
            for vid, *_ in new[l]:
                born[e].setdefault(vid, l)

    def on_second(e, ms):
        if e not in lanes:
            lanes[e] = _Lanes(ms, NL)
            old[e] = [[] for _ in range(NL)]
        new = lanes[e].read()
        after(e, old[e], new)
        before(e, new)                              # (the state before the next second)
        old[e] = new

    done, orc = [None] * E, None
    for t, acts, pols, res, orc in H.run_oracle(scn, net, on_second=on_second):
        if t < 0:
            continue
        for e, r in enumerate(res):
            if r[2] and done[e] is None:
                done[e] = t
    tot = [o.ms.totals() for o in orc]
    counted = [o.ms.lanechange_counts()['changes'] for o in orc]
    assert counted == changes, (seed, counted, changes)             # the oracle's own counter: the walk sees every change
    ev['two_feeders'] = any(len(junction[l]) >= 2 and sib[l] >= 0 and len(s) >= 2 for src in sources for l, s in src.items())
    nu = scn.live_lane_prefix()
    out = dict(ev, seed=seed, net=net, scn=scn, done=done, changes=min(changes), arrived=min(x['arrived'] for x in tot),
               teleported=sum(x['teleported'] for x in tot), interval=int(scn.control_interval_sec),
               merge='zipper' if scn.mv_zip.any() else 'yield' if (scn.mv_yield >= 0).any() else None,
               unused_twin=any(sib[l] >= nu for l in range(nu)))
    _survey[seed] = out
    return out


def test_random_street_network_is_a_pure_function_of_the_seed():
    """Built twice, the tables are equal; and the draws do not touch numpy's global generator."""
    import dataclasses
    for seed in nw.RANDOM_STREET_SEEDS:
        np.random.seed(seed)
        before = np.random.get_state()[1].copy()
        a, b = (nw.compile_network(**nw._random_street_tables(seed)[0]) for _ in range(2))
        assert (np.random.get_state()[1] == before).all()
        assert nw._random_street_tables(seed)[1] == nw._random_tables(seed)[1]
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype
                np.testing.assert_array_equal(x, y, err_msg='%s of seed %d' % (f.name, seed))
            else:
                assert x == y, (f.name, seed)


def test_seed_lists():
    assert len(nw.RANDOM_STREET_SEEDS) == len(set(nw.RANDOM_STREET_SEEDS)) == 48
    assert len(nw.RANDOM_STREET_VARIANT_SEEDS) == len(set(nw.RANDOM_STREET_VARIANT_SEEDS)) == 16
    assert set(nw.RANDOM_STREET_VARIANT_SEEDS) <= set(nw.RANDOM_STREET_SEEDS)


def test_every_network_is_inside_the_declared_limits_and_speaks_the_products_encoding():
    for seed in nw.RANDOM_STREET_SEEDS:
        net = nw.random_street_network(seed)
        scn = net.scenario().check_limits()
        base = nw.random_network(seed).scenario()
        sib, up, nxt = np.asarray(scn.lane_sib), np.asarray(scn.lane_up), np.asarray(scn.mv_next)
        assert base.n_lane < scn.n_lane <= nw.STREET_MAX_LANES and scn.n_route == base.n_route and scn.n_agent == base.n_agent, seed
        assert all(1 <= k <= nw.STREET_MAX_LINKS for k in scn.agent_nlink) and np.bincount(scn.stream_entry_lane).max() <= 8, seed
        assert 12.0 <= scn.lane_len.min() and scn.lane_len.max() <= np.float32(209.9) and 5.0 <= scn.lane_vmax.min() and scn.lane_vmax.max() <= 25.0
        assert (net.E, net.steps, net.peak, net.p_random, net.seed) == tuple(getattr(nw.random_network(seed), k) for k in
                                                                             ('E', 'steps', 'peak', 'p_random', 'seed')), seed
        streets = np.flatnonzero(sib >= 0)
        assert len(streets) >= 2 and len(streets) == 2 * (scn.n_lane - base.n_lane), seed
        for l in streets:
            s = int(sib[l])
            assert sib[s] == l and scn.lane_len[s] == scn.lane_len[l] and scn.lane_node[s] == scn.lane_node[l], (seed, l)
            assert up[l, 0] == s and s not in up[l, 1:] and not (nxt[l] == s).any(), (seed, l)
            assert not ((nxt[l] >= -1) & (nxt[s] >= -1)).any(), (seed, l)       # a route is served by one lane of a street
            junction = [int(u) for u in up[l, 1:] if u >= 0]
            assert junction == sorted({int(f) for f in np.nonzero((nxt == l).any(axis=1))[0]}), (seed, l)
            ranks = sorted({int(z) & 0xFF for f in junction for z in scn.mv_zip[f][nxt[f] == l] if z})
            assert all(z >> 8 == len(junction) for f in junction for z in scn.mv_zip[f][nxt[f] == l] if z), (seed, l)
            assert ranks in ([], list(range(len(junction)))), (seed, l, ranks)
            assert all(y in junction for f in junction for y in scn.mv_yield[f][nxt[f] == l] if y >= 0), (seed, l)
        for s, l in enumerate(scn.stream_entry_lane):                   # every vehicle is served where it stands or beside it
            for r in {int(x) for x in scn.stream_choice[s, :, :, 0].ravel() if x >= 0}:
                assert nxt[l, r] >= -1 or (sib[l] >= 0 and nxt[sib[l], r] >= -1), (seed, s)
        for a in range(scn.n_agent):                # every used link is open in some phase of its agent and serves one lane
            for k in {int(x) for x in scn.mv_link[scn.lane_node == a].ravel() if x >= 0}:
                assert any(p[k] in 'Gg' for p in scn.phases[a]), (seed, a, k)
                assert len({int(l) for l in np.flatnonzero(scn.lane_node == a) if (scn.mv_link[l] == k).any()}) == 1, (seed, a, k)


def test_every_episode_ends_inside_its_run_and_every_instance_changes_lanes():
    for seed in nw.RANDOM_STREET_SEEDS:
        s = survey(seed)
        assert all(d is not None and d < s['net'].steps for d in s['done']), (seed, s['done'])
        assert s['changes'] > 0 and s['arrived'] > 0, (seed, s['changes'], s['arrived'])


FLOORS = [
    ('a lane change in every instance', lambda s: s['changes'] > 0, 48),
    ('a change refused only by the room test', lambda s: s['room_only'], 3),
    ('a change refused only by the gap test', lambda s: s['gap_only'], 12),
    ('a change accepted with a positive closing-speed term', lambda s: s['closing'], 12),
    ('the third leader gives a wrong-lane head its speed', lambda s: s['third'], 12),
    ('a wrong-lane head removed by the teleport surrogate', lambda s: s['teleport'], 4),
    ('a changer and a junction arrival into one lane in one second', lambda s: s['both_sources'], 8),
    ('changes in both directions on one street in one run', lambda s: s['both_ways'], 4),
    ('two or more changers leave one lane in one second', lambda s: s['two_leave'], 6),
    ('a change on a street shorter than 50 m', lambda s: s['short'], 8),
    ('a change on a street whose speed limit exceeds its length', lambda s: s['fast'], 6),
    ('a change on an unsignalised street', lambda s: s['unsignalised'], 8),
    ('a change on an entry lane by a vehicle inserted on the wrong lane', lambda s: s['entry_wrong'], 12),
    ('a changer whose route ends on the sibling', lambda s: s['ends'], 8),
    ('a street lane receives from two of its >= 2 junction feeders', lambda s: s['two_feeders'], 8),
    ('zipper', lambda s: s['merge'] == 'zipper', 12),
    ('yield', lambda s: s['merge'] == 'yield', 12),
    ('different speed limits on the lanes of a street that carries changes', lambda s: s['vmax_differ'], 12),
    ('a second lane that no route uses', lambda s: s['unused_twin'], 4),
] + [('control interval %d' % i, lambda s, i=i: s['interval'] == i, 1) for i in range(1, 9)]


def floor_counts(seeds):
    return {name: sum(bool(f(survey(s))) for s in seeds) for name, f, _ in FLOORS}


def test_coverage_floors():
    """Networks of the 48 in which each event occurs in the oracle's run, against its floor."""
    got = floor_counts(nw.RANDOM_STREET_SEEDS)
    for name, _, least in FLOORS:
        print('%-72s %3d (>= %d)' % (name, got[name], least))
    short = {name: (got[name], least) for name, _, least in FLOORS if got[name] < least}
    assert not short, short


def test_no_street_carries_changes_in_both_directions_in_one_second():
    """Rule 10 (b) excludes it: a changer stands at least 7 m behind the sibling's old tail and is itself no further back than its
    own lane's old tail, so of two lanes at most one can send to the other in a second -- the floor that asks for both directions
    counts runs (above), and a simulator that lets both happen at once differs from the oracle in every such second."""
    assert not [s for s in nw.RANDOM_STREET_SEEDS if survey(s)['both_ways_second']]


def test_variant_subset():
    ss = [survey(s) for s in nw.RANDOM_STREET_VARIANT_SEEDS]
    assert sum(s['teleport'] or s['room_only'] for s in ss) >= 4
    assert {s['merge'] for s in ss} >= {'zipper', 'yield'}
    assert all(s['arrived'] > 0 and s['changes'] > 0 for s in ss)       # in every instance: the recorded variant's trip table is not empty




def test_controller_tables_leave_wrong_lane_vehicles_out():
    """lane_route_mov (pressure, actuated and SOTL tables) is -1 for every wrong-lane (lane, route) pair of the variant networks, and
    such pairs occur on signalised lanes in most of them."""
    with_pairs = 0
    for seed in nw.RANDOM_STREET_VARIANT_SEEDS:
        scn = nw.random_street_network(seed).scenario()
        pairs = nw.wrong_lane_pairs(scn)
        mov = scn.actuated_tables('sotl', omega_m=25.0)['lane_route_mov']
        assert all(mov[l, r] == -1 for l, r in pairs), seed
        with_pairs += bool(pairs)
    assert with_pairs >= 8


def test_walk_cases():
    """The six trace and lane-data walks: variant networks, a street and its sibling in 2 to 4 pieces each at cuts that are no float32
    values, two under Krauss, no two streams on one (entry lane, route); on the oracle alone the lane data's laneChangedFrom and
    laneChangedTo add up to the oracle's own count of lane changes, which is not zero."""
    from tests.env_rules import F, lane_data_reference
    cases = nw.street_walks()
    assert len(cases) == 6 and sum(c.scenario().car_following == 'krauss' for c in cases) == 2
    assert all(float(np.float32(c)) != c for c in nw.STREET_CUTS)
    for case in cases:
        scn = case.scenario()
        seed = int(case.key.split('_')[1])
        assert seed in nw.RANDOM_STREET_VARIANT_SEEDS and case.period % scn.control_interval_sec == 0 and scn.episode_length_sec % case.period
        cut = [l for l in range(scn.n_lane) if len(scn.lane_pieces[l]) > 1]
        assert len(cut) == 2 and scn.lane_sib[cut[0]] == cut[1] and all(2 <= len(scn.lane_pieces[l]) <= 4 for l in cut), case
        assert [p[2] for p in scn.lane_pieces[cut[0]]][:1] != [p[2] for p in scn.lane_pieces[cut[1]]][:1], case
        keys = [(int(l), int(scn.stream_choice[s, 0, 0, 0])) for s, l in enumerate(scn.stream_entry_lane)]
        assert len(set(keys)) == len(keys) and (scn.stream_mode == 0).all(), case
        want = nw.walk_lane_changes(case)
        with H.walk_context(case):
            orc = H.WalkOracles(case)
            rng = np.random.RandomState(case.rng_seed)
            for _ in range(nw.walk_steps(case)):
                orc.step(H.uniform_actions(scn, rng, case.E))
        for e, v in orc.views().items():
            ints = lane_data_reference(scn, v.snaps, case.period)[0]
            got = (int(ints[:, F['laneChangedFrom']].sum()), int(ints[:, F['laneChangedTo']].sum()))
            print('%s, instance %d: %d lane changes, %d arrived, %d teleported' % (case, e, want[e], v.ms.totals()['arrived'],
                                                                                   v.ms.totals()['teleported']))
            assert got == (want[e], want[e]) and want[e] > 0, (case, e, got, want[e])
