"""Insertion streams on the host (no GPU, no library): the stream networks of tests/networks.py (forks, ratios_in_time, sinks_ragged,
windows_on_lane) and the generated networks with redrawn stream tables (random_stream_network over RANDOM_STREAM_SEEDS) run through
the CPU oracle alone, over the very (E, steps, actions, seeds) tests/test_streams_gpu.py compares.  What each run is for is stated as
an assertion about the oracle's insertions -- which stream inserted which vehicle in which second on which route (insertion_log) --
so that a network, generator or seed list that stops reaching an edge of the insertion code fails here, not silently on the GPU.

Every mode-1 insertion of every run is also looked up again in Python (networks.table_route on the table of the second of insertion,
with the draw of networks.route_draw16): the oracle's C lookup against a second statement of the rule."""
import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import LANE_CAP, draw_stream_routes
from oracle.env_oracle import episode_stream_routes
from tests import env_harness as H
from tests import networks as nw

LEN, S0 = np.float32(5.0), np.float32(2.0)                # MICROSIM_SPEC.md rule 6: vehicle length and standstill gap


def insertion_log(scn, net):
    """The oracle's run of `net` on `scn` -> dict(rows, blocked, pending, totals, routes, live).
    rows: (instance, second, stream, serial, route, x) of every insertion; blocked: (instance, second, stream, vehicles on the entry
    lane, x of its tail or None) of every stream that had a vehicle waiting and did not insert -- the lane as the stream found it,
    after the insertions of the lower-numbered streams of that second; pending: per instance the streams' pending counts at the end;
    routes: per instance episode_stream_routes of its seed; live: mean vehicles per instance and control step.
    The streams that inserted in a second are those whose serial grew; their vehicles are the last of the entry lane, in stream
    order (oracle/microsim.c appends them in that order)."""
    E = net.E
    entry = np.asarray(scn.stream_entry_lane)
    rows, blocked, last = [], [], {}

    def on_second(e, ms):
        t = ms.time - 1
        pend, ser = ms.stream_state()
        grew = ser - last.get(e, np.zeros_like(ser))
        assert ((grew == 0) | (grew == 1)).all()
        last[e] = ser
        for l in sorted({int(entry[s]) for s in np.flatnonzero((grew > 0) | (pend > 0))}):
            mine = [int(s) for s in np.flatnonzero(entry == l)]
            d = ms.lane_vehicles(l)
            new = [s for s in mine if grew[s]]
            first = d['n'] - len(new)                           # the lane before this second's insertions: vehicles [0, first)
            for j, s in enumerate(new):
                assert d['v'][first + j] == 0.0
                rows.append((e, t, s, int(ser[s]) - 1, int(d['r'][first + j]), np.float32(d['x'][first + j])))
            for s in mine:
                if pend[s] > 0 and not grew[s]:
                    n = first + sum(1 for q in new if q < s)
                    blocked.append((e, t, s, n, np.float32(d['x'][n - 1]) if n else None))
    live, orc = [], None
    for t, acts, pols, res, orc in H.run_oracle(scn, net, on_second=on_second):
        if t >= 0:
            live.append(np.mean([o.ms.totals()['live'] for o in orc]))
            last_res = res
    assert all(r[2] for r in last_res)                          # the episode ended inside the run
    return dict(rows=rows, blocked=blocked, pending=[o.ms.stream_state()[0] for o in orc], totals=[o.ms.totals() for o in orc],
                routes=[episode_stream_routes(scn, net.seed + e) for e in range(E)], live=float(np.mean(live)))


def interval_of(scn, t):
    return min(t // int(scn.choice_interval_sec), scn.stream_choice.shape[1] - 1)


def check_lookups(scn, net, log):
    """Every insertion's route by the rule, stated again: mode 0 the stream's route, mode 2 the instance's route of this episode,
    mode 1 table_route on the table of the second of insertion.  -> the mode-1 rows with their draws (e, t, s, k, route, u16)."""
    drawn = []
    for e, t, s, k, r, _ in log['rows']:
        md = int(scn.stream_mode[s])
        if md == 1:
            u16 = nw.route_draw16(net.seed + e, s, k)
            assert r == nw.table_route(scn.stream_choice[s, interval_of(scn, t)], u16), (e, t, s, k, r, u16)
            drawn.append((e, t, s, k, r, u16))
        else:
            assert r == (int(log['routes'][e][s]) if md == 2 else int(scn.stream_choice[s, 0, 0, 0])), (e, t, s, k, r)
    return drawn


def whole_lane_allows(scn, s, n, tail):
    """Would stream s insert with the whole lane as its window, on a lane of n vehicles whose last stands at `tail`?"""
    L = np.float32(scn.lane_len[scn.stream_entry_lane[s]])
    xt = tail if n else (L + LEN) + S0
    return n < LANE_CAP and not ((xt - LEN) - S0 < LEN)


def windowed(scn, s):
    return scn.stream_origin[s] != 0.0 or scn.stream_limit[s] < scn.lane_len[scn.stream_entry_lane[s]]


def emission_second(scn, s, k):
    """The second in which vehicle k of stream s is emitted (the integer rule of the flow elements, added up in flow order)."""
    horizon = int(scn.episode_length_sec) + 64
    per_sec = np.zeros(horizon, np.int64)
    for b, en, vph, st in np.asarray(scn.flows, np.int64).tolist():
        if st == s:
            tau = np.arange(max(b, 0), min(en, horizon)) - b
            per_sec[max(b, 0):min(en, horizon)] += ((tau + 1) * vph + 3599) // 3600 - (tau * vph + 3599) // 3600
    return int(np.searchsorted(np.cumsum(per_sec), k + 1))


_logs = {}


def _log(name):
    if name not in _logs:
        net = nw.SINKS_EVEN if name == 'sinks_even' else nw.NETWORKS[name]
        scn = net.scenario()
        log = insertion_log(scn, net)
        log['drawn'] = check_lookups(scn, net, log)
        print('%s: %d insertions, %d refusals, mean live vehicles %.1f, arrived %s, pending at the end %s'
              % (name, len(log['rows']), len(log['blocked']), log['live'], [x['arrived'] for x in log['totals']],
                 [int(p.sum()) for p in log['pending']]))
        _logs[name] = (net, scn, log)
    return _logs[name]


# ---- compile_network ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make', [lambda: nw.NETWORKS['ctrl8'].scenario(), lambda: nw.random_network(3).scenario()], ids=['ctrl8', 'random_3'])
def test_tuple_streams_compile_to_the_tables_they_always_did(make):
    """(entry lane, route) streams: one interval, one choice (route, 65536), mode 0, the whole lane, no choice interval -- and the
    same scenario compiled from the dict form of the same streams is equal table by table."""
    import dataclasses
    scn = make()
    NS = scn.n_stream
    assert scn.stream_choice.shape == (NS, 1, 1, 2) and scn.stream_choice.dtype == np.int32 and (scn.stream_choice[:, 0, 0, 1] == 65536).all()
    assert (scn.stream_mode == 0).all() and (scn.stream_origin == 0.0).all() and scn.choice_interval_sec == 1 << 30
    np.testing.assert_array_equal(scn.stream_limit, scn.lane_len[scn.stream_entry_lane])
    if scn.name.startswith('random'):
        args = nw._random_tables(3)[0]
        assert all(isinstance(s, tuple) for s in args['streams'])
        np.testing.assert_array_equal(scn.stream_choice[:, 0, 0, 0], [r for _, r in args['streams']])
        as_dicts = nw.compile_network(**dict(args, streams=[dict(lane=l, mode=0, choice=[[(r, 65536)]]) for l, r in args['streams']]))
        for f in dataclasses.fields(scn):
            x, y = getattr(scn, f.name), getattr(as_dicts, f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype, f.name
                np.testing.assert_array_equal(x, y, err_msg=f.name)
            else:
                assert x == y, f.name


def test_dict_streams_pad_their_tables():
    scn = nw.NETWORKS['forks'].scenario()
    assert scn.stream_choice.shape == (8, 1, 6, 2) and (scn.stream_mode == 1).all()
    K = (scn.stream_choice[:, 0, :, 0] >= 0).sum(axis=1).tolist()
    assert K == [2, 1, 3, 2, 2, 6, 2, 2] and scn.stream_choice[4, 0, 1].tolist() == [-1, 0] and scn.stream_choice[4, 0, 2].tolist() == [2, 65536]
    assert (scn.stream_choice[1, 0, 1:] == [-1, 0]).all()
    scn = nw.NETWORKS['ratios_in_time'].scenario()
    assert scn.stream_choice.shape == (4, 4, 3, 2) and scn.choice_interval_sec == nw.RATIOS_INTERVAL and scn.stream_mode.tolist() == [1, 1, 1, 0]
    assert (scn.stream_choice[3, :, 0] == [8, 65536]).all()            # a stream of one table repeats it in every interval
    scn = nw.NETWORKS['windows_on_lane'].scenario()
    assert scn.stream_origin.dtype == scn.stream_limit.dtype == np.float32
    assert float(scn.stream_origin[1]) != 61.7 and float(scn.stream_limit[1]) != 120.1     # (no float32 values)
    assert scn.stream_origin[2] + LEN == scn.stream_limit[2] and scn.stream_origin[3] + LEN > scn.stream_limit[3]


# ---- the hand-made networks -----------------------------------------------------------------------------------------------------------
def _by_stream(log):
    out = {}
    for e, t, s, k, r, x in log['rows']:
        out.setdefault(s, []).append((e, t, k, r, x))
    return out


def test_forks_reaches_every_edge_of_the_weight_lookup():
    net, scn, log = _log('forks')
    assert log['live'] > net.live_floor and min(x['arrived'] for x in log['totals']) > 20
    assert nw.reachable_prefix(scn) == 5 and (np.bincount(scn.stream_entry_lane) == [8]).all()
    per_second = {}
    for e, t, s, k, r, x in log['rows']:
        per_second[(e, t)] = per_second.get((e, t), 0) + 1
    crowded = sum(n >= 3 for n in per_second.values())
    print('forks: seconds with >= 3 insertions on the entry lane: %d; most in one second: %d' % (crowded, max(per_second.values())))
    assert crowded >= 6 and min(sum(n >= 3 for (e, _), n in per_second.items() if e == i) for i in range(net.E)) >= 1
    by = _by_stream(log)
    assert sorted(by) == list(range(8)) and all(len(v) >= 10 for v in by.values())       # every named edge is exercised
    took = {s: {r for _, _, _, r, _ in v} for s, v in by.items()}
    assert took[0] == {0}                       # the weight-0 route (1) is never taken from its stream ...
    assert 1 in took[3] | took[5] | took[6]     # ... and is taken from others
    assert took[1] == {2}                       # one choice at 65536
    assert took[2] == {1}                       # weights 1 and 65535: only the draws 0 and 65535 take another route
    assert took[3] == {0, 1}                    # a last weight of 40000: the draws past it take the last route
    past = [u for e, t, s, k, r, u in log['drawn'] if s == 3 and u >= 40000]
    assert len(past) >= 5
    assert took[4] == {0}                       # the pad ends the list: draws >= 30000 stay on route 0, route 2 behind the pad is never taken
    assert sum(1 for e, t, s, k, r, u in log['drawn'] if s == 4 and u >= 30000) >= 5
    assert took[5] == {0, 1, 2} and took[7] == {0, 2}
    # the draw that equals a weight: `draw < weight` is false, the vehicle takes the second route
    s6, k6 = nw.FORKS_EDGE
    edge = [(r, u) for e, t, s, k, r, u in log['drawn'] if (e, s, k) == (0, s6, k6)]
    assert edge == [(2, int(scn.stream_choice[s6, 0, 0, 1]))], edge
    assert 0 < edge[0][1] < 65536 and took[6] == {1, 2}


def test_ratios_in_time_crosses_boundaries_with_a_backlog():
    net, scn, log = _log('ratios_in_time')
    assert log['live'] > net.live_floor and min(x['arrived'] for x in log['totals']) > 20
    ilen, NI = int(scn.choice_interval_sec), scn.stream_choice.shape[1]
    assert (ilen, NI, scn.control_interval_sec) == (7, 4, 5) and scn.episode_length_sec > NI * ilen
    # lane 4 carries the routes 4 and 7 alone, and neither is in a table of the intervals 0 and 1: the live lanes include it all the same
    late = int(np.flatnonzero((scn.mv_next[:, [4, 7]] != -2).all(axis=1) & (np.delete(scn.mv_next, [4, 7], axis=1) == -2).all(axis=1))[0])
    ch = scn.stream_choice[..., 0]
    assert not np.isin(ch[:, :2], [4, 7]).any() and all((ch[:, 2:] == r).any() for r in (4, 7))
    assert nw.reachable_prefix(scn) == scn.n_lane == 8 and late < nw.reachable_prefix(scn)
    assert min(sum(r == q for _, _, _, _, r, _ in log['rows']) for q in (4, 7)) >= 10
    used = [{int(r) for r in ch[s].ravel() if r >= 0} for s in range(4)]
    assert not any(s in used[s] for s in range(4)) and sum(len(u) for u in used) == len(set().union(*used))      # no stream index, no shared route
    # every interval sees insertions of the mode-1 streams, in every instance; most of them come after the clamp
    for e in range(net.E):
        seen = {min(t // ilen, 99) for ee, t, s, k, r, u in log['drawn'] if ee == e}
        assert seen >= set(range(NI + 3)), (e, sorted(seen))
    # the held-back stream: vehicles emitted in one interval and inserted in a later one, whose route is not the one the table of
    # their emission second gives their draw
    late_rows = other = 0
    for e, t, s, k, r, u in log['drawn']:
        te = emission_second(scn, s, k)
        assert te <= t
        if s == 2 and interval_of(scn, te) < interval_of(scn, t):
            late_rows += 1
            other += r != nw.table_route(scn.stream_choice[s, interval_of(scn, te)], u)
    print('ratios_in_time: %d vehicles of stream 2 inserted in a later interval than emitted, %d on another route for it' % (late_rows, other))
    assert late_rows >= 12 and other >= 6
    waiting = {(e, t) for e, t, s, n, tail in log['blocked'] if s == 2}
    assert all((e, b) in waiting for e in range(net.E) for b in (ilen, 2 * ilen, 3 * ilen))         # a backlog at every boundary


@pytest.mark.parametrize('name', ['sinks_ragged', 'sinks_even'])
def test_sinks_instances_draw_different_routes(name):
    net, scn, log = _log(name)
    assert log['live'] > net.live_floor and min(x['arrived'] for x in log['totals']) > 20
    m2 = np.flatnonzero(scn.stream_mode == 2)
    K = (scn.stream_choice[m2, 0, :, 0] >= 0).sum(axis=1).tolist()
    assert K == ([5, 3, 2, 1, 2] if name == 'sinks_ragged' else [2] * 5) and sorted(scn.stream_mode.tolist()) == [0, 1, 2, 2, 2, 2, 2]
    routes = np.stack(log['routes'])
    assert len({tuple(r) for r in routes[:, m2].tolist()}) == net.E                    # the instances' draws differ
    fixed = np.flatnonzero(scn.stream_mode != 2)
    assert (routes[:, fixed] == scn.stream_choice[fixed, 0, 0, 0]).all()
    by = _by_stream(log)
    for s in m2:                                # every drawn stream inserts, in every instance, on the instance's route
        assert {e for e, _, _, _, _ in by[int(s)]} == set(range(net.E))
    assert any(routes[e, s] != scn.stream_choice[s, 0, 0, 0] for e in range(net.E) for s in m2)       # (not the fixed route)


@pytest.mark.parametrize('name', ['sinks_ragged', 'sinks_even'])
def test_route_draws_of_the_product_and_of_the_oracle_agree(name):
    """scenario.draw_stream_routes (ragged candidate lists: one stream after the other; equal counts: one vectorised draw) against
    the oracle's restatement, seeds 0 .. 199."""
    scn = _log(name)[1]
    K = (scn.stream_choice[scn.stream_mode == 2, 0, :, 0] >= 0).sum(axis=1)
    assert (len(set(K.tolist())) > 1) == (name == 'sinks_ragged')
    seen = set()
    for seed in range(200):
        got, want = draw_stream_routes(scn, seed), episode_stream_routes(scn, seed)
        assert got.dtype == want.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg='seed %d' % seed)
        seen.add(tuple(got.tolist()))
    assert len(seen) >= 15


def test_windows_on_lane():
    net, scn, log = _log('windows_on_lane')
    assert log['live'] > net.live_floor and min(x['arrived'] for x in log['totals']) > 20
    by = _by_stream(log)
    T = net.steps * scn.control_interval_sec
    o, hi = scn.stream_origin, scn.stream_limit
    assert 3 not in by                          # the narrow window: the serial stays 0 ...
    emitted3 = sum((max(0, min(T, en) - b) * vph + 3599) // 3600 for b, en, vph, s in scn.flows.tolist() if s == 3)
    assert emitted3 >= 30 and all(int(p[3]) == emitted3 for p in log['pending'])         # ... and the backlog holds every vehicle emitted
    for s in (0, 1, 2):
        xs = np.array([x for _, _, _, _, x in by[s]])
        assert len(xs) >= 3 * net.E and (xs >= o[s] + LEN).all() and (xs <= hi[s]).all(), s
    fit = by[2]
    assert {e for e, _, _, _, _ in fit} == set(range(net.E)) and all(x == np.float32(155.0) for _, _, _, _, x in fit)
    assert any(t == 0 for _, t, _, _, _ in fit) and any(t > 120 for _, t, _, _, _ in fit)      # on the empty lane at the start, and after it drained
    xs1 = np.array([x for _, _, _, _, x in by[1]])
    assert xs1.min() < 70.0 and xs1.max() > 110.0 and len(set(xs1.tolist())) > 20
    # stream 1 inserts and stream 2, whose window lies ahead, finds that vehicle as the tail in the same second: refused by the window
    ins1 = {(e, t): x for e, t, _, _, x in by[1]}
    behind = [(e, t) for e, t, s, n, tail in log['blocked'] if s == 2 and (e, t) in ins1 and tail == ins1[(e, t)]]
    assert len(behind) >= 3
    by_window = sum(bool(whole_lane_allows(scn, s, n, tail)) for e, t, s, n, tail in log['blocked'] if s in (1, 2))
    assert by_window >= 20


# ---- the generated networks -------------------------------------------------------------------------------------------------------
_survey = {}


def survey(seed):
    """The oracle's run of random_stream_network(seed) -> what the quotas count."""
    if seed not in _survey:
        net = nw.random_stream_network(seed)
        scn = net.scenario()
        log = insertion_log(scn, net)
        drawn = check_lookups(scn, net, log)
        took = {}
        for e, t, s, k, r, u in drawn:
            took.setdefault(s, set()).add(r)
        m2 = np.flatnonzero(scn.stream_mode == 2)
        inserted = {(e, s) for e, t, s, k, r, x in log['rows']}
        _survey[seed] = dict(
            net=net, scn=scn, modes=np.bincount(scn.stream_mode, minlength=3).tolist(),
            two_routes=any(len(v) >= 2 for v in took.values()),
            later_table=any(interval_of(scn, t) >= 1 and r != nw.table_route(scn.stream_choice[s, 0], u) for e, t, s, k, r, u in drawn),
            differ=any(log['routes'][0][s] != log['routes'][1][s] and (0, s) in inserted and (1, s) in inserted for s in m2),
            window_inserts=any(windowed(scn, s) for e, t, s, k, r, x in log['rows']),
            window_blocks=any(windowed(scn, s) and whole_lane_allows(scn, s, n, tail) for e, t, s, n, tail in log['blocked']),
            arrived=min(x['arrived'] for x in log['totals']), live=log['live'])
    return _survey[seed]


STREAM_QUOTAS = [
    ('a mode-1 stream whose vehicles took two or more routes', 'two_routes', 16),
    ('a vehicle of interval >= 1 on another route than the first table gives its draw', 'later_table', 8),
    ('a mode-2 stream with different routes in the two instances', 'differ', 8),
    ('a windowed stream that inserted', 'window_inserts', 12),
    ('a window that refused an insertion the whole lane allows', 'window_blocks', 4),
]


def test_stream_seed_list():
    assert len(nw.RANDOM_STREAM_SEEDS) == len(set(nw.RANDOM_STREAM_SEEDS)) == 24 and set(nw.RANDOM_STREAM_SEEDS) <= set(nw.RANDOM_SEEDS)


def test_random_stream_network_keeps_the_network_and_redraws_the_streams():
    """Everything but the stream tables (and the lane order, which follows the load the tables spread) is random_network's; built
    twice, the tables are equal; the tables are inside what the generator promises and inside the limits."""
    for seed in nw.RANDOM_STREAM_SEEDS:
        base, (args, run) = nw._random_tables(seed), nw._random_stream_tables(seed)
        assert run == base[1] and {k: v for k, v in args.items() if k not in ('streams', 'choice_interval_sec', 'name')} \
            == {k: v for k, v in base[0].items() if k not in ('streams', 'name')}
        assert [s['lane'] for s in args['streams']] == [l for l, _ in base[0]['streams']]
        a, b = nw.random_stream_network(seed).scenario(), nw.compile_network(**nw._random_stream_tables(seed)[0])
        for f in ('stream_entry_lane', 'stream_mode', 'stream_choice', 'stream_origin', 'stream_limit', 'mv_next', 'lane_len'):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg='%s of seed %d' % (f, seed))
        a.check_limits()
        NS, NI, KC, _ = a.stream_choice.shape
        assert 1 <= NI <= 4 and (NI == 1 or 3 <= a.choice_interval_sec <= 40), seed
        assert (a.stream_limit - a.stream_origin >= LEN).all() and (a.stream_origin >= 0).all(), seed
        assert (a.stream_limit <= a.lane_len[a.stream_entry_lane]).all(), seed
        w = a.stream_choice[..., 1].astype(np.int64)
        assert (np.diff(np.where(a.stream_choice[..., 0] >= 0, w, 1 << 20), axis=2) >= 0).all() and w.max() <= 65536, seed


def test_stream_quotas():
    """Networks of the 24 in which each event occurs, against its quota; every network has arrivals."""
    ss = [survey(s) for s in nw.RANDOM_STREAM_SEEDS]
    got = {name: sum(bool(s[key]) for s in ss) for name, key, _ in STREAM_QUOTAS}
    for name, _, least in STREAM_QUOTAS:
        print('%-82s %3d (>= %d)' % (name, got[name], least))
    print('streams by mode over the 24 networks: %s' % np.sum([s['modes'] for s in ss], axis=0).tolist())
    short = {name: (got[name], least) for name, _, least in STREAM_QUOTAS if got[name] < least}
    assert not short, short
    assert all(s['arrived'] > 0 for s in ss), [s['net'].name for s in ss if s['arrived'] == 0]
    # the first eight run under every kernel variant, recording included: they show most of it themselves
    first = ss[:8]
    assert sum(s['two_routes'] for s in first) >= 4 and sum(s['differ'] for s in first) >= 2 and sum(s['window_inserts'] for s in first) >= 4
