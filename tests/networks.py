"""Synthetic road networks for the simulator parity tests -- TEST INFRASTRUCTURE ONLY, host only (no GPU, no library).

step_kernel (csrc/tsc_env.hip) is the one kernel every configuration shares, and the three built-in scenarios visit a small corner of
what tsc_env_create accepts: at most 113 live lanes, 16 routes, 28 agents, three feeders per lane, link index 21, a 5 s / 2 s control
interval, one vehicle per second and stream.  Every network of NETWORKS exists because of one declared limit (INTEGRATION.md section 5,
"Supported scenarios"); the limit is named next to it.  Three tools build them:

* tile(scn, k): k disjoint copies of a compiled Scenario as one scenario;
* compile_network(...): a small compiler for hand-made networks (lanes, routes as lane sequences, phase strings, streams, flows);
* NETWORKS: name -> Net (factory, the limit it drives, the step plan tsc_env_step_plan must report, and the run: E, control steps,
  share of random actions, seed).

The runs of tests/test_networks_gpu.py are redrawn on the host by run_oracle / draw_actions of tests/env_harness.py, so that tests/test_networks_host.py
states conditions (the limit is reached, the roads are not empty) about the very runs the GPU tests compare.

The kernels around the step (controllers, pressure reward, recording walks, per-instance demand) run on the same networks: AUX, at the
end of this file, lists those runs for tests/test_networks_aux_host.py and tests/test_networks_aux_gpu.py; windows() and split_pieces()
exist for them.

random_network(seed), behind AUX, draws whole networks inside every limit at once -- the seeded sweep of
tests/test_networks_random_host.py and tests/test_networks_random_gpu.py over RANDOM_SEEDS.

The insertion streams -- route modes, choice tables that change in time, insertion windows -- have networks of their own (forks,
ratios_in_time, sinks, windows_on_lane) and random_stream_network(seed), which redraws the stream tables of random_network(seed):
tests/test_streams_host.py and tests/test_streams_gpu.py over RANDOM_STREAM_SEEDS.

Two-lane streets (MICROSIM_SPEC.md rule 10: lane choice and lane changing) come from compile_network's `siblings` and CHANGE hops:
random_street_network(seed) turns lanes of random_network(seed) into streets -- tests/test_streets_host.py and
tests/test_streets_gpu.py over RANDOM_STREET_SEEDS; two_lane() is the hand-made one behind the lane_sib refusals."""
import copy

import numpy as np

from deeprl_signal_control_amd.scenario import (DET_LEN, MAX_UP, Scenario, _obs_table, _signal_tables, _state_dims, build_large_grid,
                                                sort_lanes_by_load)
from tests.env_harness import run_oracle, with_rates         # noqa: F401 (with_rates: under this module's name for the cases' columns)
from tests.env_rules import greedy_rule


# ---------------------------------------------------------------------------
# tile
# ---------------------------------------------------------------------------
def _block_diag(m, k, fill, lane_off=0):
    """k copies of the [NL, NR] table m on the diagonal of a [k NL, k NR] table, `fill` off the blocks; entries >= 0 of copy j are
    moved by j * lane_off (tables that name lanes)."""
    m = np.asarray(m)
    NL, NR = m.shape
    out = np.full((k * NL, k * NR), fill, m.dtype)
    for j in range(k):
        out[j * NL:(j + 1) * NL, j * NR:(j + 1) * NR] = np.where(m >= 0, m + j * lane_off, m) if lane_off else m
    return out


def _offset(a, k, step):
    """k copies of the index array a along axis 0, entries >= 0 of copy j moved by j * step."""
    a = np.asarray(a)
    return np.concatenate([np.where(a >= 0, a + j * step, a) for j in range(k)]).astype(a.dtype)


def tile(scn, k, **env_kw):
    """k disjoint copies of `scn` as one scenario: lane, route, agent (and stream = route) indices of copy j moved by j times the
    base's counts, the movement tables block-diagonal (off the blocks: next -2, link -1, yield -1, prio 0, zip 0), the observation
    tables rebuilt from the moved neighbour lists, the lanes sorted by load again so that the live lanes are a prefix.  env_kw:
    Scenario fields to replace (episode_length_sec, ...).  Scenarios with declared insertion streams are not needed here."""
    assert scn.stream_entry_lane is None, 'tile: every route must be its own stream'
    NL, NR, A = scn.n_lane, scn.n_route, scn.n_agent
    t = copy.copy(scn)
    tag = lambda j, nm: 'c%d.%s' % (j, nm)
    t.name = '%s_x%d' % (scn.name, k)
    t.n_agent, t.n_route = k * A, k * NR
    t.node_names = [tag(j, n) for j in range(k) for n in scn.node_names]
    t.lane_names = [tag(j, n) for j in range(k) for n in scn.lane_names]
    t.lane_pieces = [[(tag(j, nm), st, ln) for nm, st, ln in ps] for j in range(k) for ps in scn.lane_pieces]
    for f in ('lane_len', 'lane_vmax', 'lane_det_start', 'lane_origin', 'agent_nlane', 'agent_nlink', 'agent_nphase', 'green_tab',
              'yellow_tab', 'link_foes'):
        setattr(t, f, np.concatenate([np.asarray(getattr(scn, f))] * k))
    t.lane_node = _offset(scn.lane_node, k, A)
    t.lane_up = _offset(scn.lane_up, k, NL)
    t.lane_sib = None if scn.lane_sib is None else _offset(scn.lane_sib, k, NL)
    t.mv_next = _block_diag(scn.mv_next, k, -2, NL)
    t.mv_link = _block_diag(scn.mv_link, k, -1)
    t.mv_yield = _block_diag(scn.mv_yield, k, -1, NL)
    t.mv_prio = _block_diag(scn.mv_prio, k, 0)
    t.mv_zip = _block_diag(scn.mv_zip, k, 0)
    t.route_entry_lane = _offset(scn.route_entry_lane, k, NL)
    t.route_names = [(tag(j, a), tag(j, b)) for j in range(k) for a, b in scn.route_names]
    t.agent_lanes = _offset(scn.agent_lanes, k, NL)
    t.link_lane = _offset(scn.link_lane, k, NL)
    t.phases = [list(p) for _ in range(k) for p in scn.phases]
    t.neighbors = [[n + j * A for n in ns] for j in range(k) for ns in scn.neighbors]
    t.n_a_ls = list(scn.n_a_ls) * k
    nlane = [int(x) for x in t.agent_nlane]
    t.n_s_ls, t.n_w_ls, t.n_f_ls = _state_dims(scn.agent, nlane, t.n_a_ls, t.neighbors, scn.has_wait_state)
    t.obs_kind, t.obs_src, t.obs_len = _obs_table(scn.agent, t.agent_lanes, nlane, t.n_a_ls, t.neighbors, scn.has_wait_state,
                                                  int(scn.green_tab.shape[1]))
    fl = np.asarray(scn.flows, np.int32)
    t.flows = np.concatenate([fl + np.array([0, 0, 0, j * NR], np.int32) for j in range(k)])
    t.extra = dict(scn.extra, tiles=k)
    for key, v in env_kw.items():
        assert key in Scenario.__dataclass_fields__, key
        setattr(t, key, v)
    t = sort_lanes_by_load(t)
    return t.streams_ready().check_limits()


def tile_block(t, base, j):
    """Copy j of tile(base, k) brought back to the base's numbering: dict of the tables a copy must share with the base (lanes
    matched by name, indices moved back), for the faithfulness test."""
    NL, NR, A = base.n_lane, base.n_route, base.n_agent
    at = {nm: i for i, nm in enumerate(t.lane_names)}
    rows = np.array([at['c%d.%s' % (j, nm)] for nm in base.lane_names])
    back = np.full(t.n_lane, -9, np.int64)
    back[rows] = np.arange(NL)

    def lanes(v):
        v = np.asarray(v)
        return np.where(v >= 0, back[np.clip(v, 0, None)], v)
    cols = slice(j * NR, (j + 1) * NR)
    ag = slice(j * A, (j + 1) * A)
    out = dict(lane_len=t.lane_len[rows], lane_vmax=t.lane_vmax[rows], lane_det_start=t.lane_det_start[rows],
               lane_origin=t.lane_origin[rows], lane_node=np.where(t.lane_node[rows] >= 0, t.lane_node[rows] - j * A, -1),
               lane_up=np.sort(lanes(t.lane_up[rows]), axis=1), mv_next=lanes(t.mv_next[rows, cols]), mv_link=t.mv_link[rows, cols],
               mv_yield=lanes(t.mv_yield[rows, cols]), mv_prio=t.mv_prio[rows, cols], mv_zip=t.mv_zip[rows, cols],
               route_entry_lane=lanes(t.route_entry_lane[cols]), agent_lanes=lanes(t.agent_lanes[ag]), link_lane=lanes(t.link_lane[ag]),
               green_tab=t.green_tab[ag], yellow_tab=t.yellow_tab[ag], agent_nlane=t.agent_nlane[ag],
               neighbors=[[n - j * A for n in ns] for ns in t.neighbors[ag]], n_s_ls=t.n_s_ls[ag], n_w_ls=t.n_w_ls[ag], n_f_ls=t.n_f_ls[ag],
               obs_kind=t.obs_kind[ag, :base.s_max])
    if base.lane_sib is not None:
        out['lane_sib'] = lanes(t.lane_sib[rows])
    src = t.obs_src[ag, :base.s_max].astype(np.int64)
    kind = out['obs_kind']
    src = np.where((kind >= 1) & (kind <= 3), back[np.clip(src, 0, t.n_lane - 1)], np.where(kind == 4, src - j * A * int(t.green_tab.shape[1]), src))
    out['obs_src'] = src
    fl = np.asarray(t.flows)
    mine = fl[(fl[:, 3] >= j * NR) & (fl[:, 3] < (j + 1) * NR)]
    out['flows'] = mine - np.array([0, 0, 0, j * NR])
    # everything outside the block is "no movement"
    other = np.ones(t.n_route, bool)
    other[cols] = False
    out['off_block'] = (bool((t.mv_next[rows][:, other] == -2).all()), bool((t.mv_link[rows][:, other] == -1).all()),
                        bool((t.mv_yield[rows][:, other] == -1).all()), bool((t.mv_prio[rows][:, other] == 0).all()),
                        bool((t.mv_zip[rows][:, other] == 0).all()))
    return out


def base_block(base):
    """The same dict for the base scenario itself."""
    out = {f: np.asarray(getattr(base, f)) for f in ('lane_len', 'lane_vmax', 'lane_det_start', 'lane_origin', 'lane_node', 'mv_next',
                                                     'mv_link', 'mv_yield', 'mv_prio', 'mv_zip', 'route_entry_lane', 'agent_lanes', 'link_lane',
                                                     'green_tab', 'yellow_tab', 'agent_nlane', 'obs_kind', 'obs_src', 'flows')}
    out['lane_up'] = np.sort(np.asarray(base.lane_up), axis=1)
    out.update(neighbors=[list(n) for n in base.neighbors], n_s_ls=list(base.n_s_ls), n_w_ls=list(base.n_w_ls), n_f_ls=list(base.n_f_ls))
    if base.lane_sib is not None:
        out['lane_sib'] = np.asarray(base.lane_sib)
    out['off_block'] = (True,) * 5
    return out


def reachable_prefix(scn):
    """The NU of the device: Scenario.live_lane_prefix (tsc_env_create's chain walk)."""
    return scn.live_lane_prefix()


# ---------------------------------------------------------------------------
# a compiler for hand-made networks
# ---------------------------------------------------------------------------
def stream_hash(seed, stream, serial, k):
    """The counter-based hash of MICROSIM_SPEC.md rule 6 in Python integers: draw k of the vehicle `serial` of `stream` under the
    instance's episode seed (k = 0 position, 1 and 2 speed factor, 3 route)."""
    m = 0xFFFFFFFF
    h = (seed * 0x9E3779B1 + stream * 0x85EBCA77 + serial * 0xC2B2AE3D + k * 0x27D4EB2F) & m
    h ^= h >> 16
    h = h * 0x85EBCA6B & m
    h ^= h >> 13
    h = h * 0xC2B2AE35 & m
    return h ^ h >> 16


def route_draw16(seed, stream, serial):
    """The 16-bit number a mode-1 stream's vehicle compares with the cumulative weights of its table."""
    return stream_hash(int(seed) & 0xFFFFFFFF, stream, serial, 3) >> 16


def table_route(table, u16):
    """The route a [KC, 2] table of (route, cumulative weight) pairs gives the draw u16: the first pair with u16 < weight; a pad
    (-1) ends the list, and a draw no weight exceeds takes the last route before it."""
    rt = int(table[0][0])
    for r, w in table:
        if r < 0:
            break
        rt = int(r)
        if u16 < w:
            break
    return rt


def _stream_tables(streams, lane_len):
    """The stream tables of compile_network's dict form -> keywords of Scenario.  A tuple (entry lane, route) among dicts is the
    mode-0 stream with the one choice (route, 65536).  A stream with fewer intervals than the longest repeats its last table."""
    full = [s if isinstance(s, dict) else dict(lane=s[0], mode=0, choice=[[(s[1], 65536)]]) for s in streams]
    NS, NI = len(full), max(len(s['choice']) for s in full)
    KC = max(len(row) for s in full for row in s['choice'])
    choice = np.zeros((NS, NI, KC, 2), np.int32)
    choice[..., 0] = -1
    for i, s in enumerate(full):
        assert set(s) <= {'lane', 'mode', 'choice', 'origin', 'limit'}, sorted(s)
        for iv in range(NI):
            row = s['choice'][min(iv, len(s['choice']) - 1)]
            choice[i, iv, :len(row)] = np.asarray(row, np.int32).reshape(-1, 2)
    entry = np.array([s['lane'] for s in full], np.int32)
    return dict(stream_entry_lane=entry, stream_mode=np.array([s['mode'] for s in full], np.int32), stream_choice=choice,
                stream_origin=np.array([s.get('origin', 0.0) for s in full], np.float32),
                stream_limit=np.array([s.get('limit', lane_len[s['lane']]) for s in full], np.float32))


CHANGE = -7                     # compile_network: the "link" of a path's hop that is left sideways, for the sibling lane (rule 10)


def compile_network(name, agent, lanes, routes, phases, neighbors, flows, streams=None, merge='zipper', check=True,
                    choice_interval_sec=None, siblings=None, **env_kw):
    """A Scenario from a hand-made network.
    lanes: (length m, speed limit m/s, downstream agent or -1) per lane.
    routes: per route index a list of paths; a path is a list of (lane, signal link of the hop that leaves it, -1 = none); the last
        lane of a path is where the route ends.  Disjoint parts of the network may share a route index -- the movement table is
        keyed by (lane, route) and a stream names its entry lane -- which keeps n_live_lanes x n_route small with many agents.
    siblings: [(l0, l1), ...], the two lanes of every two-lane street (MICROSIM_SPEC.md rule 10; lane_sib, symmetric).  A hop (l,
        CHANGE) of a path says that the connection of the hop before it enters l, which does not serve the route: the path's next
        element is l's sibling, where the vehicle moves over and which carries the route on (its link, its next lane, or the end
        of the route).  In the tables: mv_next[previous lane][r] = l, mv_next[l][r] stays "not served" (-2), mv_next[sibling][r] is
        the next lane or -1; lane_up lists a lane's sibling first, then its junction feeders (at most MAX_UP - 1), and the merge
        tables come from the junction feeders alone.  A stream may also insert on the lane of a street that does not serve its
        route (it names its entry lane).  None: no lane has a sibling (lane_sib None).
    phases: per agent its phase strings (one char per signal link); neighbors: per agent a list of agents.
    flows: (begin, end, veh/h, stream).  streams: (entry lane, route) per insertion stream; None = route r is stream r and enters at
        the first lane of its only path.  A stream may also be a dict: lane, mode (0 fixed route, 1 a draw per vehicle, 2 a route
        per instance and episode from the host), choice = per interval a list [(route, cumulative weight of 65536), ...] (padded
        with (-1, 0) to the longest, the k_choice of the scenario) and, optionally, origin and limit in metres, the stretch of the
        entry lane the stream inserts on (default: the whole lane).  choice_interval_sec: the length of a choice interval.
    merge: what arbitrates a lane with several feeders -- 'zipper' (mv_zip = rank | count << 8, rank = position among the ascending
        feeders) or 'yield' (the lowest feeder has priority, the others yield to its head).
    Derived: lane_up, the mv_* tables, the agents' lanes (dedup of their links' lanes in link order) and the signal / observation
    tables with the scenario compiler's own helpers.  Detectors cover the last 50 m of a signalised lane.  Ends with
    streams_ready().check_limits() (check=False: the caller wants a scenario past a limit)."""
    NL, NR, A = len(lanes), len(routes), len(phases)
    lane_len = np.array([l[0] for l in lanes], np.float32)
    lane_vmax = np.array([l[1] for l in lanes], np.float32)
    lane_node = np.array([l[2] for l in lanes], np.int32)
    mv_next = np.full((NL, NR), -2, np.int32)
    mv_link = np.full((NL, NR), -1, np.int32)
    lane_sib = None
    if siblings is not None:
        lane_sib = np.full(NL, -1, np.int32)
        for l0, l1 in siblings:
            assert l0 != l1 and lane_sib[l0] == lane_sib[l1] == -1, 'lanes %d and %d: a lane has one sibling' % (l0, l1)
            lane_sib[l0], lane_sib[l1] = l1, l0
    left = set()                                                    # (lane, route) of the hops that are left sideways
    for r, paths in enumerate(routes):
        for path in paths:
            for i, (l, k) in enumerate(path):
                assert mv_next[l, r] == -2 and (l, r) not in left, 'lane %d appears twice on route %d' % (l, r)
                if k == CHANGE:
                    assert lane_sib is not None and i + 1 < len(path) and path[i + 1][0] == lane_sib[l] and path[i + 1][1] != CHANGE, \
                        'route %d changes from lane %d to a lane that is not its sibling' % (r, l)
                    left.add((l, r))
                    continue
                mv_next[l, r] = path[i + 1][0] if i + 1 < len(path) else -1
                if i + 1 < len(path) and lane_node[l] >= 0:
                    mv_link[l, r] = k
    lane_up = np.full((NL, MAX_UP), -1, np.int32)
    mv_zip = np.zeros((NL, NR), np.int32)
    mv_yield = np.full((NL, NR), -1, np.int32)
    mv_prio = np.zeros((NL, NR), np.int32)
    for l2 in range(NL):
        ups = sorted({int(l) for l in np.nonzero((mv_next == l2).any(axis=1))[0]})
        slots = ups if lane_sib is None or lane_sib[l2] < 0 else [int(lane_sib[l2])] + ups      # lane changers are gathered first
        assert len(slots) <= MAX_UP, 'lane %d has %d feeders' % (l2, len(slots))
        lane_up[l2, :len(slots)] = slots
        if len(ups) > 1:
            for rank, l in enumerate(ups):
                into = mv_next[l] == l2
                if merge == 'zipper':
                    mv_zip[l, into] = rank | (len(ups) << 8)
                elif rank == 0:
                    mv_prio[l, into] = 1
                else:
                    mv_yield[l, into] = ups[0]
    kmax = max(len(p[0]) for p in phases)
    link_lane = np.full((A, kmax), -1, np.int32)
    for l, r in zip(*np.nonzero(mv_link >= 0)):
        a, k = int(lane_node[l]), int(mv_link[l, r])
        assert k < len(phases[a][0]), 'lane %d uses link %d, agent %d has %d' % (l, k, a, len(phases[a][0]))
        assert link_lane[a, k] in (-1, l), 'link %d of agent %d serves lanes %d and %d' % (k, a, link_lane[a, k], l)
        link_lane[a, k] = l
    per_agent = []
    for a in range(A):
        ded = []
        for l in link_lane[a]:
            if l >= 0 and int(l) not in ded:
                ded.append(int(l))
        assert ded, 'agent %d controls no lane' % a
        per_agent.append(ded)
    lmax = max(len(d) for d in per_agent)
    agent_lanes = np.full((A, lmax), -1, np.int32)
    for a, d in enumerate(per_agent):
        agent_lanes[a, :len(d)] = d
    nlane = [len(d) for d in per_agent]
    n_a_ls = [len(p) for p in phases]
    has_wait = bool(env_kw.get('has_wait_state', True))
    n_s, n_w, n_f = _state_dims(agent, nlane, n_a_ls, neighbors, has_wait)
    obs_kind, obs_src, lens = _obs_table(agent, agent_lanes, nlane, n_a_ls, neighbors, has_wait, max(n_a_ls))
    green, yellow = _signal_tables(phases, kmax)
    stream_kw = {}
    if streams is not None and any(isinstance(s, dict) for s in streams):
        stream_kw = _stream_tables(streams, lane_len)
        if choice_interval_sec is not None:
            stream_kw['choice_interval_sec'] = int(choice_interval_sec)
    elif streams is not None:
        choice = np.zeros((len(streams), 1, 1, 2), np.int32)
        choice[:, 0, 0, 0] = [s[1] for s in streams]
        choice[:, 0, 0, 1] = 65536
        stream_kw = dict(stream_entry_lane=np.array([s[0] for s in streams], np.int32), stream_choice=choice)
    scn = Scenario(
        name=name, agent=agent, node_names=['n%d' % a for a in range(A)], n_agent=A,
        lane_names=['l%d' % l for l in range(NL)], lane_len=lane_len, lane_vmax=lane_vmax, lane_node=lane_node,
        lane_det_start=np.where(lane_node >= 0, np.maximum(lane_len - DET_LEN, 0.0), 0.0).astype(np.float32), lane_up=lane_up,
        lane_sib=lane_sib, n_route=NR, mv_next=mv_next, mv_link=mv_link, mv_yield=mv_yield, mv_prio=mv_prio, mv_zip=mv_zip,
        route_entry_lane=np.array([paths[0][0][0] if paths else 0 for paths in routes], np.int32),
        route_names=[('r%d' % r, 'r%d' % r) for r in range(NR)],
        agent_lanes=agent_lanes, agent_nlane=np.array(nlane, np.int32), agent_nlink=np.array([len(p[0]) for p in phases], np.int32),
        agent_nphase=np.array(n_a_ls, np.int32), link_lane=link_lane, phases=[list(p) for p in phases], green_tab=green,
        yellow_tab=yellow, neighbors=[list(n) for n in neighbors], n_s_ls=n_s, n_w_ls=n_w, n_f_ls=n_f, n_a_ls=n_a_ls,
        obs_kind=obs_kind, obs_src=obs_src, flows=np.array(flows, np.int32).reshape(-1, 4), obs_len=lens, **stream_kw, **env_kw)
    scn = sort_lanes_by_load(scn).streams_ready()
    return scn.check_limits() if check else scn


# ---------------------------------------------------------------------------
# the networks
# ---------------------------------------------------------------------------
def isolated(n, agent='ia2c', live=None, streams_per_lane=None, **env_kw):
    """n one-lane junctions: an in lane of 150 m, an out lane of 100 m, phases G / r, ring neighbours, all on route 0.  Junction j
    has one stream (streams_per_lane: {junction: count} for those with more) whose rate differs from junction to junction, so that
    the local rewards differ between the agents; only the junctions of `live` (default: all) carry demand -- the lanes of the others
    are dead."""
    live = set(range(n) if live is None else live)
    episode = env_kw.setdefault('episode_length_sec', 600)
    lanes, paths, streams, flows = [], [], [], []
    for j in range(n):
        lanes += [(150.0, 13.89, j), (100.0, 13.89, -1)]
        paths.append([(2 * j, 0), (2 * j + 1, -1)])
        if j in live:
            nq = (streams_per_lane or {}).get(j, 1)
            for q in range(nq):                     # (a lane with several streams: each at 2 / nq of the rate, so that the lane still drains)
                flows.append((0, episode, (240 + 40 * ((7 * j + 3 * q) % 13)) // ((nq + 1) // 2), len(streams)))
                streams.append((2 * j, 0))
    return compile_network('isolated_%d' % n, agent, lanes, [paths], [['G', 'r']] * n, [[(j - 1) % n, (j + 1) % n] for j in range(n)],
                           flows, streams, **env_kw)


def few_threads():
    """100 junctions of which the LAST 30 carry demand (60 live lanes: one wavefront under TSC_ENV_HELP=0), nine of them with eight
    streams on the entry lane (kMaxEntry): 93 streams and 100 agents on 64 threads.  The agents that signal live lanes are 70 .. 99
    and the streams 64 .. 92 enter live lanes: what the two stride loops of step_kernel's prologue write -- the link states and
    prev_action of the agents, the pending vehicles and emissions of the streams past the first 64 -- decides the traffic."""
    return isolated(100, live=range(70, 100), streams_per_lane={j: 8 for j in range(70, 97, 3)}, episode_length_sec=450, teleport_sec=120)


def merge4(merge, phases0=('GGGG', 'GGrr', 'rrGG', 'GrGr'), **env_kw):
    """Four feeder lanes (links 0-3 of agent 0) into one lane, which agent 1 holds back at its own signal: every feeder carries
    900 veh/h, so the four heads compete for the lane in the same second -- as a zipper of four (rank | 4 << 8) or by right of
    way (the lowest feeder has priority, the other three yield to its head).  phases0: agent 0's four phase strings."""
    env_kw.setdefault('episode_length_sec', 400)
    lanes = [(150.0, 13.89, 0)] * 4 + [(120.0, 13.89, 1), (100.0, 13.89, -1)]
    routes = [[[(f, f), (4, 0), (5, -1)]] for f in range(4)]
    flows = [(0, 400, 900, f) for f in range(4)]
    return compile_network('merge4_%s' % merge, 'ia2c', lanes, routes, [list(phases0), ['G', 'r', 'G']], [[1], [0]], flows,
                           merge=merge, teleport_sec=90, **env_kw)


def link62(last=62, check=True):
    """One agent with 63 signal links (k_max = 63) and eight phases (p_max = 8): six lanes on links 0, 13, 31, 47, 61 and `last`
    (62 is the largest index the movement word holds), each with its own exit."""
    used = [0, 13, 31, 47, 61, last]
    nlink = max(63, last + 1)
    rng = np.random.RandomState(62)
    phases = []
    for p in range(8):
        s = rng.choice(list('Ggr'), size=nlink, p=[0.3, 0.1, 0.6])
        for i, k in enumerate(used):
            s[k] = 'G' if (i + p) % 3 == 0 else ('g' if (i + p) % 3 == 1 and p % 2 else 'r')
        phases.append(''.join(s))
    lanes = [(150.0, 13.89, 0)] * 6 + [(100.0, 13.89, -1)] * 6
    routes = [[[(i, used[i]), (6 + i, -1)]] for i in range(6)]
    flows = [(0, 400, 500 + 60 * i, i) for i in range(6)]
    return compile_network('link62', 'ia2c', lanes, routes, [phases], [[]], flows, check=check, episode_length_sec=400, teleport_sec=120)


def corridor(n=3, **env_kw):
    """n junctions in a row: the main road (route 0) passes all of them, every junction has a side street whose traffic crosses
    (route 1) or turns into the main road (route 2) and yields to it there.  Links per junction: 0 main, 1 side crossing, 2 side
    turning (the side street has one lane for both)."""
    episode = env_kw.setdefault('episode_length_sec', 500)
    lanes = [(120.0, 13.89, j if j < n else -1) for j in range(n + 1)]              # main lanes 0 .. n
    main = [(j, 0) for j in range(n)] + [(n, -1)]
    cross, turn, flows, streams = [], [], [], [(0, 0)]
    flows.append((0, episode, 700, 0))
    for j in range(n):
        s, x = len(lanes), len(lanes) + 1
        lanes += [(100.0, 11.0, j), (80.0, 11.0, -1)]
        cross.append([(s, 1), (x, -1)])
        streams += [(s, 1), (s, 2)]
        flows += [(0, episode, 300 + 50 * j, len(streams) - 2), (0, episode, 250, len(streams) - 1)]
    # route 2: side street j -> main lane j + 1 -> ... -> the end of the main road; one path per side street would put main lanes on
    # route 2 twice, so the turners of junction j take route 2 + j
    routes = [[main], cross] + [[[(n + 1 + 2 * j, 2)] + main[j + 1:]] for j in range(n)]
    streams = [(e, r if r < 2 else 2 + (e - n - 1) // 2) for e, r in streams]
    return compile_network('corridor_%d' % n, 'ma2c', lanes, routes, [['Grr', 'rGg', 'GrG']] * n,
                           [[k for k in (j - 1, j + 1) if 0 <= k < n] for j in range(n)], flows, streams, merge='yield', **env_kw)


def burst(peak=9000, begin=0, check=True):
    """One stream at 9000 veh/h (two or three vehicles a second) for 100 s into a 40 m lane that takes one insertion a second at
    best: `pending` backs up for most of the run.  The lane and a second feeder zip into a 30 m lane whose signal is red in two of
    three phases: it stays full up to its start, the two heads behind it compete for the little room it gives, and teleport_sec =
    20 makes the teleport surrogate fire -- heads pass the red signal after 20 s of standing, heads that still find no room are
    taken out of the network."""
    lanes = [(40.0, 13.89, 0), (150.0, 13.89, 0), (30.0, 13.89, 1), (100.0, 13.89, -1)]
    routes = [[[(0, 0), (2, 0), (3, -1)]], [[(1, 1), (2, 0), (3, -1)]]]
    flows = [(begin, 100, peak, 0), (150, 200, 7200, 0), (0, 300, 1200, 1)]
    return compile_network('burst', 'ia2c', lanes, routes, [['GG', 'rG', 'Gr'], ['r', 'r', 'G']], [[1], [0]], flows, check=check,
                           episode_length_sec=300, teleport_sec=20)


def zip254(n_lane=254, check=True):
    """Groups of three feeders zipping into one signalised lane with its exit, plus two isolated junctions: n_lane lanes (254: 50
    groups).  The feeders carry the least load, so after load sorting they have the highest indices -- up to 253, the largest a
    feeder byte of Smem::up4 holds (0xFF = none)."""
    groups = (n_lane - 4) // 5
    lanes, flows, streams = [], [], []
    paths = [[], [], []]
    for g in range(groups):
        m = len(lanes)
        lanes += [(150.0, 13.89, g), (100.0, 13.89, -1)]
        for f in range(3):
            lanes.append((100.0 + 10.0 * f, 13.89, -1))
            paths[f].append([(m + 2 + f, -1), (m, 0), (m + 1, -1)])
            flows.append((0, 400, 260 + 30 * ((g + 2 * f) % 5), len(streams)))
            streams.append((m + 2 + f, f))
    for j in range(2):
        m = len(lanes)
        lanes += [(150.0, 13.89, groups + j), (100.0, 13.89, -1)]
        paths[j].append([(m, 0), (m + 1, -1)])
        flows.append((0, 400, 500, len(streams)))
        streams.append((m, j))
    while len(lanes) < n_lane:                      # (n_lane not of the form 5 g + 4: dead lanes make up the count)
        lanes.append((50.0, 13.89, -1))
    A = groups + 2
    return compile_network('zip%d' % n_lane, 'ia2c', lanes, paths, [['G', 'r']] * A, [[(a + 1) % A] for a in range(A)], flows, streams,
                           check=check, episode_length_sec=400, teleport_sec=60)


WINDOWS_EPISODE = 120
# flow elements of windows(): (begin, end, veh/h, stream).  The emission tables hold the seconds [0, episode + 64) = [0, 184).
WINDOWS_FLOWS = [
    (1, 18, 1800, 0),           # begins at 1, ends at 2 mod 4
    (22, 43, 2400, 0),          # begins at 2, ends at 3 mod 4
    (47, 61, 1500, 0),          # begins at 3, ends at 1 mod 4
    (66, 67, 3600, 0),          # a one-second window
    (70, 70, 3600, 0),          # an empty window
    (5, 30, 1200, 1), (10, 23, 900, 1),         # two overlapping elements on one stream
    (40, 90, 0, 1),             # a zero-rate element
    (3, 119, 700, 2),
    (100, 300, 1000, 2),        # ends past the table
    (190, 250, 2000, 2),        # begins past the table
    (81, 84, 900, 3), (82, 86, 1800, 3),        # WINDOWS_PAIR: the second begins a second after the first, they share seconds 82 and 83
    (6, 78, 600, 3),            # (the stream's other element stays clear of the pair)
]
WINDOWS_PAIR = (11, 12)


def windows():
    """Three isolated one-lane junctions (as isolated(): in lane 150 m, out lane 100 m, phases G / r) under a 1 s control interval
    without yellow, four insertion streams (two on the first junction's lane) and the flow elements of WINDOWS_FLOWS: windows that
    begin and end at 1, 2 and 3 mod 4 (demand_kernel packs four seconds per thread and clamps tau at both ends of a window), one
    second long, empty, overlapping on one stream, of rate zero, and past the emission table at their end or altogether."""
    lanes, paths = [], []
    for j in range(3):
        lanes += [(150.0, 13.89, j), (100.0, 13.89, -1)]
        paths.append([(2 * j, 0), (2 * j + 1, -1)])
    streams = [(0, 0), (0, 0), (2, 0), (4, 0)]
    return compile_network('windows', 'ia2c', lanes, [paths], [['G', 'r']] * 3, [[(j - 1) % 3, (j + 1) % 3] for j in range(3)],
                           WINDOWS_FLOWS, streams, control_interval_sec=1, yellow_interval_sec=0, episode_length_sec=WINDOWS_EPISODE,
                           teleport_sec=60)


def windows_columns(scn):
    """The veh/h columns of the per-instance demand runs on windows(), int32 [4, n_flow]; with (a, b) = WINDOWS_PAIR:
    0: the scenario's own column;
    1: a = 3600 x 55, b = 3600 x 200: 55 + 200 = 255 vehicles in each of the two shared seconds (the limit: accepted);
    2: every rate redrawn (zero stays zero), one element of several vehicles a second;
    3: a = 3600 x 55 + 1, b = 3600 x 200: the bounds ceil(vph / 3600) add up to 56 + 200 = 256, but a emits its 56 only in its own
       first second, before b begins -- no second exceeds 255, and only the per-second path of the host check can tell."""
    nominal = np.asarray(scn.flows)[:, 2].astype(np.int32)
    a, b = WINDOWS_PAIR
    cols = np.tile(nominal, (4, 1))
    cols[1, a], cols[1, b] = 3600 * 55, 3600 * 200
    rng = np.random.RandomState(77)
    cols[2] = np.where(nominal > 0, rng.randint(300, 3000, len(nominal)), 0)
    cols[2, 1] = 9000
    cols[3, a], cols[3, b] = 3600 * 55 + 1, 3600 * 200
    return cols


def windows_refused_column(scn):
    """Column 1 of windows_columns with a = 3600 x 56: 256 vehicles in second 82 -> (column, flow named, second named): the sum
    passes 255 when the second element of the pair is added."""
    col = windows_columns(scn)[1].copy()
    col[WINDOWS_PAIR[0]] = 3600 * 56
    return col, WINDOWS_PAIR[1], 82


def demand254_columns(scn, E):
    """The veh/h columns of the isolated_254 demand run, int32 [E, 254]: every instance its own rates (the junctions still drain),
    the last stream of instance e at several vehicles a second."""
    rng = np.random.RandomState(254)
    cols = rng.randint(150, 700, (E, len(scn.flows))).astype(np.int32)
    cols[np.arange(E), -1] = 5000 + 1000 * np.arange(E)
    return cols


def ratios_columns(scn):
    """The veh/h columns of the per-instance demand run on ratios_in_time(), int32 [3, n_flow]: the scenario's own, every rate
    redrawn, and one with the held-back stream (2) at two vehicles a second and stream 3 silent."""
    nominal = np.asarray(scn.flows)[:, 2].astype(np.int32)
    cols = np.tile(nominal, (3, 1))
    cols[1] = np.random.RandomState(78).randint(200, 2500, len(nominal))
    by_stream = np.asarray(scn.flows)[:, 3]
    cols[2, by_stream == 2] = 7200
    cols[2, by_stream == 3] = 0
    return cols


def split_pieces(scn, cuts):
    """A copy of scn whose lanes named in cuts = {lane name: ascending cut positions in m} are made of len(cuts) + 1 SUMO lanes
    '<name>#0', '<name>#1', ... that each begin at 0: lane_pieces only, which the lane data and the trajectories' SUMO positions
    read (Scenario.lane_data_slots, sumo_lane_pos) -- the simulator's lanes stay whole."""
    out = copy.copy(scn)
    out.name = scn.name + '_pieces'
    pieces = [list(ps) for ps in scn.lane_pieces]
    for nm, cs in cuts.items():
        l = scn.lane_names.index(nm)
        assert len(pieces[l]) == 1 and 1 <= len(cs) <= 4 and list(cs) == sorted(cs) and 0.0 < cs[0] and cs[-1] < float(scn.lane_len[l]), nm
        edges = [0.0] + [float(c) for c in cs] + [float(scn.lane_len[l])]
        pieces[l] = [('%s#%d' % (nm, i), 0.0, edges[i + 1] - edges[i]) for i in range(len(edges) - 1)]
    out.lane_pieces = pieces
    return out


# merge4_zipper in pieces: the merged lane in five, a feeder in three, the exit in two; 33.3, 61.7, 20.1 and 90.9 are no float32 values
MERGE4_CUTS = {'l4': [20.1, 33.3, 61.7, 90.9], 'l0': [33.3, 100.1], 'l5': [61.7]}


class Net:
    """One entry of NETWORKS.  plan: (MAXT, HELP, REC, KF, SPEC, threads) of tsc_env_step_plan for a fresh handle under `env` (the
    TSC_ENV_* variables the case sets).  E instances run `steps` control steps; an action is random with probability p_random, else
    the greedy rule (greedy_action); peak: the control step after which the vehicle state is compared too (and at the end);
    live_floor: the least mean number of vehicles per instance the oracle must show over the run."""

    def __init__(self, factory, why, plan, E, steps, p_random, seed, peak, live_floor, env=None):
        self.factory, self.why, self.plan = factory, why, plan
        self.E, self.steps, self.p_random, self.seed, self.peak, self.live_floor = E, steps, p_random, seed, peak, live_floor
        self.env = dict(env or {})
        self._scn = None

    def scenario(self):
        """The compiled scenario (built once; callers do not modify it)."""
        if self._scn is None:
            self._scn = self.factory()
        return self._scn


_NARROW, _WIDE = (256, 1, 0, 1, 0), (1024, 1, 0, 4, 0)
NETWORKS = {
    # n_mv = NU x NR = 166 x 24 > 8 x 256 words: the copy_words fallback of the prologue, runtime dimensions (no kSpec row matches)
    'grid_x2': Net(lambda: tile(build_large_grid('ma2c'), 2, episode_length_sec=600), 'movement table past the register prefetch',
                   _NARROW + (256,), 3, 120, 0.3, 410, 90, 60.0),
    # the largest k tsc_env_create accepts (157,584 B of the 160 KiB of LDS; Krauss 163,728 B; k = 5: REFUSED): NU = 332 > 256 live lanes,
    # workgroups of NLA = 384 threads (6 wavefronts), 4-wide flat phase
    'grid_x4': Net(lambda: tile(build_large_grid('ma2c'), 4, episode_length_sec=500),
                   'more than 256 live lanes: the wide runtime-dimension kernel', _WIDE + (384,), 2, 100, 0.3, 420, 80, 120.0),
    # A > 128: numpy's np.sum splits the agents' rewards recursively; NU = 260 -> NLA = 320
    'isolated_130': Net(lambda: isolated(130, objective='hybrid'), 'more than 128 agents: np_sum past one block', _WIDE + (320,),
                        2, 120, 0.5, 430, 60, 200.0),
    'isolated_254': Net(lambda: isolated(254, objective='hybrid'), '254 insertion streams (the limit), 254 agents', _WIDE + (512,),
                        2, 120, 0.5, 440, 60, 400.0),
    # A > 256: np.sum's left half splits again (300 -> 144 + 156 -> 72 + 72, 72 + 84); 250 of the junctions carry demand (254 streams at most)
    'isolated_300': Net(lambda: isolated(300, live=[j for j in range(300) if j % 6 != 5], objective='hybrid'),
                        'more than 256 agents: np_sum two levels down the left', _WIDE + (512,), 2, 120, 0.5, 445, 60, 400.0),
    'few_threads': Net(few_threads, 'more streams and more agents than threads; eight streams on one entry lane', (256, 0, 0, 4, 0, 64),
                       3, 90, 0.5, 450, 50, 60.0, env={'TSC_ENV_HELP': '0'}),
    'merge4_zipper': Net(lambda: merge4('zipper'), 'four feeders of one lane as a zipper (TSC_MAX_UP)', _NARROW + (256,), 4, 80, 0.4, 460, 40, 25.0),
    'merge4_yield': Net(lambda: merge4('yield'), 'four feeders of one lane by right of way', _NARROW + (256,), 4, 80, 0.4, 461, 40, 25.0),
    'link62': Net(link62, 'signal link 62, k_max = 63, p_max = 8', _NARROW + (256,), 4, 80, 0.7, 470, 40, 15.0),
    'ctrl8': Net(lambda: corridor(3, control_interval_sec=8, yellow_interval_sec=3, episode_length_sec=500), 'control interval 8 s / yellow 3 s, '
                 'episode no multiple of 8', _NARROW + (256,), 3, 63, 0.5, 480, 30, 15.0),
    'ctrl1': Net(lambda: corridor(3, control_interval_sec=1, yellow_interval_sec=0, episode_length_sec=140), 'control interval 1 s, no yellow',
                 _NARROW + (256,), 3, 140, 0.1, 481, 100, 8.0),
    'burst': Net(burst, 'several vehicles per second from one stream, pending backs up, frequent teleports', _NARROW + (256,),
                 4, 60, 0.6, 490, 20, 8.0),
    # NLA = 256 live lanes: 256 threads, no helper wavefront
    'zip254': Net(zip254, 'feeder lane indices up to 253 in the merge arbitration bytes', _NARROW + (256,), 2, 80, 0.5, 500, 40, 100.0),
}
NETWORKS['windows'] = Net(windows, 'flow windows that begin and end inside a 4-second word of the emission table; 1 s control interval',
                          _NARROW + (256,), 3, 120, 0.3, 510, 60, 8.0)


# ---- insertion streams: route modes, choice tables in time, insertion windows (tests/test_streams_host.py, tests/test_streams_gpu.py)
FORKS_SEED = 520
FORKS_EDGE = (6, 0)             # (stream, serial): the vehicle of instance 0 whose draw equals its table's first weight


def forks():
    """One entry lane (0) whose road diverges twice -- route 0: 0 -> 1 -> 2, route 1: 0 -> 3, route 2: 0 -> 1 -> 4 -- and eight
    mode-1 streams on it (MAX_ENTRY), each with a table of its own (k_choice 6, one interval):
      0: a first choice of weight 0 (never taken);            1: one choice at 65536 (always taken; a table of one pair);
      2: weights 1 and 65535;                                 3: a last weight below 65536 (draws past it take the last route);
      4: a pad in the middle (it ends the list: route 2 behind it is never taken);
      5: six pairs;                                           7: two pairs;
      6: a first weight equal to the draw of its own first vehicle in instance 0 (FORKS_EDGE): `draw < weight` is false there
         and the vehicle takes the second route -- the one vehicle that tells < from <=.
    All eight emit a vehicle in second 0 and in every 30th second after it, on top of a light steady rate, so that several of them
    insert in one second on a lane that has drained in between."""
    lanes = [(150.0, 13.89, 0), (120.0, 13.89, 1), (100.0, 13.89, -1), (80.0, 11.0, -1), (80.0, 11.0, -1)]
    routes = [[[(0, 0), (1, 0), (2, -1)]], [[(0, 1), (3, -1)]], [[(0, 0), (1, 1), (4, -1)]]]
    edge = route_draw16(FORKS_SEED, *FORKS_EDGE)
    tables = [[(1, 0), (0, 65536)],
              [(2, 65536)],
              [(0, 1), (1, 65535), (2, 65536)],
              [(0, 20000), (1, 40000)],
              [(0, 30000), (-1, 0), (2, 65536)],
              [(0, 10000), (1, 20000), (2, 30000), (0, 40000), (1, 50000), (2, 65536)],
              [(1, edge), (2, 65536)],
              [(2, 16384), (0, 65536)]]
    streams = [dict(lane=0, mode=1, choice=[t]) for t in tables]
    flows = [(0, 300, 60 + 5 * s, s) for s in range(8)] + [(b, b + 1, 3600, s) for b in range(30, 300, 30) for s in range(8)]
    return compile_network('forks', 'ia2c', lanes, routes, [['GG', 'Gr', 'rG'], ['GG', 'rG', 'Gr']], [[1], [0]], flows, streams,
                           episode_length_sec=300, teleport_sec=120)


RATIOS_INTERVAL = 7


def ratios_in_time():
    """Mode-1 streams whose tables change every 7 s, four times (n_interval 4), under a 5 s control interval: the boundaries at 7,
    14 and 21 s fall inside control steps, and from 28 s on the last table stays in force.  Entry lane 0 diverges like forks():
    0 -> 1 -> 2 (routes 2 and 5), 0 -> 3 (routes 3 and 6), 0 -> 1 -> 4 (routes 4 and 7); stream 0 draws among 2, 3 and 4, stream 1
    among 5, 6 and 7.  Routes 4 and 7 appear in the intervals 2 and 3 only, and lane 4 is used by no other route -- the live lanes
    include it only if the walk reads every interval.  Entry lane 5 is 20.1 m short behind a signal that is red in three of four
    phases (routes 0 and 8: 5 -> 6, route 1: 5 -> 7): stream 2 emits a vehicle a second for 25 s, so its backlog stands across
    every boundary, and a vehicle draws from the table of the second it is inserted in.  Stream 3 is a mode-0 stream on the same
    lane.  No two streams share a route -- the trace knows a vehicle by (route, serial, entry lane) -- and no stream index equals
    a route the stream can take."""
    lanes = [(150.0, 13.89, 0), (120.0, 13.89, 1), (100.0, 13.89, -1), (80.0, 11.0, -1), (90.0, 11.0, -1),
             (20.1, 13.89, 2), (100.0, 13.89, -1), (100.0, 13.89, -1)]
    main, off, late = [(0, 0), (1, 0), (2, -1)], [(0, 1), (3, -1)], [(0, 0), (1, 1), (4, -1)]
    routes = [[[(5, 0), (6, -1)]], [[(5, 1), (7, -1)]], [main], [off], [late], [main], [off], [late], [[(5, 0), (6, -1)]]]
    streams = [
        dict(lane=0, mode=1, choice=[[(2, 40000), (3, 65536)], [(3, 65536)], [(4, 30000), (2, 65536)], [(2, 20000), (3, 40000), (4, 65536)]]),
        dict(lane=0, mode=1, choice=[[(6, 65536)], [(5, 65536)], [(5, 50000)], [(7, 65536)]]),
        dict(lane=5, mode=1, choice=[[(0, 65536)], [(1, 65536)], [(0, 32768), (1, 65536)], [(1, 20000), (0, 65536)]]),
        (5, 8)]
    flows = [(0, 60, 1800, 0), (60, 300, 500, 0), (0, 40, 1200, 1), (40, 300, 300, 1), (0, 25, 3600, 2), (100, 300, 300, 2), (30, 300, 200, 3)]
    return compile_network('ratios_in_time', 'ia2c', lanes, routes, [['GG', 'Gr', 'rG'], ['GG', 'rG', 'Gr'], ['rr', 'rr', 'rr', 'GG']],
                           [[1], [0], []], flows, streams, choice_interval_sec=RATIOS_INTERVAL, episode_length_sec=300, teleport_sec=120)


def sinks(ragged=True):
    """Mode-2 streams (the route of an instance's episode comes from the host, drawn among the stream's candidates) on two fans:
    lane 0 -> lanes 1 .. 5 (routes 0 .. 4) and lane 6 -> lanes 7 .. 9 (routes 5 .. 7).  ragged: 5, 3, 2, 1 and 2 candidates (k_choice
    5, the shorter lists padded), which scenario.draw_stream_routes draws one stream after the other; else two candidates each, its
    vectorised branch.  A mode-0 and a mode-1 stream sit between them: their entries of the host's route array are ignored."""
    lanes = [(200.0, 13.89, 0)] + [(80.0 + 5.0 * i, 11.0, -1) for i in range(5)] + [(150.0, 13.89, 1)] + [(90.0, 11.0, -1)] * 3
    routes = [[[(0, i), (1 + i, -1)]] for i in range(5)] + [[[(6, i), (7 + i, -1)]] for i in range(3)]
    cands = [[0, 1, 2, 3, 4], [5, 6, 7], [6, 7], [5], [4, 0]] if ragged else [[0, 4], [5, 7], [6, 7], [5, 6], [4, 0]]
    m2 = [dict(lane=l, mode=2, choice=[[(r, 65536) for r in c]]) for l, c in zip((0, 6, 6, 6, 0), cands)]
    streams = [m2[0], (0, 2), m2[1], dict(lane=0, mode=1, choice=[[(1, 30000), (3, 65536)]]), m2[2], m2[3], m2[4]]
    flows = [(0, 300, 300 + 40 * s, s) for s in range(7)]
    return compile_network('sinks_ragged' if ragged else 'sinks_even', 'ia2c', lanes, routes,
                           [['GGGGG', 'GGrrr', 'rrGGG', 'GrGrG'], ['GGG', 'Grr', 'rGG']], [[1], [0]], flows, streams,
                           episode_length_sec=300, teleport_sec=120)


WINDOW_FIT = (150.0, 155.0)     # exactly one vehicle length: on an empty lane xlo = 150 + 5 = xmax
WINDOW_NARROW = (30.0, 34.9)    # less than one: xmax < xlo always


def windows_on_lane():
    """One 200 m entry lane with four streams and their insertion windows: 0: [0, 200] given explicitly; 1: [61.7, 120.1] (no
    float32 values); 2: WINDOW_FIT, which takes a vehicle only at 155 m and only while no vehicle stands behind 162 m; 3:
    WINDOW_NARROW, which never inserts -- its backlog grows to the end.  Stream 2's window lies ahead of stream 1's: when both
    wait, stream 1 inserts first and its vehicle is the tail stream 2 finds.  Streams 0 and 1 pause (0 - 10 s, 120 - 170 s), so
    that the lane drains and stream 2 finds it empty.  Every stream has a route of its own over the same two lanes (the trace
    knows a vehicle by (route, serial, entry lane))."""
    lanes = [(200.0, 13.89, 0), (100.0, 13.89, -1)]
    windows = [(0.0, 200.0), (61.7, 120.1), WINDOW_FIT, WINDOW_NARROW]
    streams = [dict(lane=0, mode=0, choice=[[(s, 65536)]], origin=o, limit=hi) for s, (o, hi) in enumerate(windows)]
    flows = [(10, 120, 400, 0), (170, 300, 400, 0), (20, 120, 400, 1), (170, 300, 300, 1), (0, 300, 240, 2), (0, 300, 360, 3)]
    return compile_network('windows_on_lane', 'ia2c', lanes, [[[(0, 0), (1, -1)]]] * 4, [['G', 'r']], [[]], flows, streams,
                           episode_length_sec=300, teleport_sec=120)


NETWORKS['forks'] = Net(forks, 'eight mode-1 streams on one lane: every edge of the cumulative-weight lookup', _NARROW + (256,),
                        3, 60, 0.4, FORKS_SEED, 30, 5.0)
NETWORKS['ratios_in_time'] = Net(ratios_in_time, 'choice tables that change inside control steps; a backlog across the boundaries',
                                 _NARROW + (256,), 3, 60, 0.8, 530, 8, 5.0)
NETWORKS['sinks_ragged'] = Net(sinks, 'mode-2 streams with 1, 2, 3 and 5 candidates between streams of the other modes',
                               _NARROW + (256,), 3, 60, 0.4, 546, 30, 5.0)
NETWORKS['windows_on_lane'] = Net(windows_on_lane, 'insertion windows: whole lane, inner, exactly one vehicle, less than one',
                                  _NARROW + (256,), 3, 60, 0.4, 550, 30, 3.0)
SINKS_EVEN = Net(lambda: sinks(ragged=False), 'mode-2 streams with two candidates each: the vectorised draw', _NARROW + (256,),
                 3, 60, 0.4, 546, 30, 5.0)
STREAM_NETWORKS = ['forks', 'ratios_in_time', 'sinks_ragged', 'windows_on_lane']
# grid_x4: the one plan behind the LDS budget (whether k = 4 fits); the stream networks: the plan of the generic kernel with the stream
# tables uploaded.  As reported by an MI355X handle
RECORDED = ['grid_x4'] + STREAM_NETWORKS


def _routes255():
    """255 junctions, each on a route (and so a stream) of its own."""
    n = 255
    lanes = [(150.0, 13.89, j) for j in range(n)] + [(100.0, 13.89, -1) for j in range(n)]
    return compile_network('routes255', 'ia2c', lanes, [[[(j, 0), (n + j, -1)]] for j in range(n)], [['G', 'r']] * n, [[] for _ in range(n)],
                           [(0, 100, 300, j) for j in range(n)], check=False, episode_length_sec=100)


def _no_route():
    scn = copy.copy(isolated(2))
    NL = scn.n_lane
    scn.n_route = 0
    for f in ('mv_next', 'mv_link', 'mv_yield', 'mv_prio', 'mv_zip'):
        setattr(scn, f, np.zeros((NL, 0), np.int32))
    scn.route_entry_lane, scn.flows, scn.route_names = np.zeros(0, np.int32), np.zeros((0, 4), np.int32), []
    scn.stream_entry_lane = scn.stream_origin = scn.stream_limit = scn.stream_mode = scn.stream_choice = None
    return scn


def _zip_rank16():
    scn = copy.copy(merge4('zipper'))
    scn.mv_zip = np.where(scn.mv_zip == (3 | 4 << 8), 16 | 4 << 8, scn.mv_zip).astype(np.int32)
    return scn


# Scenarios one step past a limit: name -> (factory, what Scenario.check_limits says (None: only the library can tell), what tsc_env_create
# says).  Host checks on both sides: nothing is ever launched with them.
REFUSED = {
    'routes255': (_routes255, 'at most 254 each', 'n_route 255 > 254'),
    'streams255': (lambda: isolated(255, check=False), 'at most 254 each', 'n_stream 255 > 254'),
    'entry9': (lambda: isolated(2, streams_per_lane={0: 9}, check=False), '9 streams enter lane', 'more than 8 streams enter lane'),
    'link63': (lambda: link62(last=63, check=False), 'signal link index 63', 'signal link index 63 > 62'),
    'ctrl9': (lambda: corridor(3, control_interval_sec=9, yellow_interval_sec=3, check=False), 'control_interval_sec 9 > 8', 'control interval 9 > 8 s'),
    'rate256': (lambda: burst(peak=256 * 3600, check=False), 'emit 256 vehicles in one second', 'emit more than 255 vehicles per second'),
    'zip256': (lambda: zip254(256, check=False), '256 lanes with zipper merges', 'zipper merges need lane indices < 255'),
    'zip_rank16': (_zip_rank16, 'zipper slot overflow: rank 16', 'zipper slot overflow: rank 16'),
    'grid_x5': (lambda: tile(build_large_grid('ma2c'), 5), None, 'LDS need [0-9]+ B > 160 KiB'),
    'no_route': (_no_route, 'at least one of each', 'at least one of each'),
    'scratch': (lambda: isolated(130, live=range(30), check=False), 'too few live lanes \\(60 of 260, 130 agents\\)',
                'too few live lanes \\(60 of 260, 130 agents\\)'),
    'begin_neg': (lambda: burst(begin=-5, check=False), 'flow 0 begins at second -5', 'flow 0 begins at second -5'),
}


# ---------------------------------------------------------------------------
# the kernels around the step: controllers, pressure reward, recording walks, per-instance demand
# ---------------------------------------------------------------------------
_aux_scn = {}


def aux_scenario(key):
    """The scenario of an AUX case (built once; callers do not modify it): a registry entry's own, or one of its variants."""
    if key not in _aux_scn:
        if key == 'isolated_130_ma2c':
            scn = isolated(130, agent='ma2c', objective='hybrid')
        elif key == 'isolated_130_200s':            # (an episode of 200 s: the walks run to its end)
            scn = isolated(130, objective='hybrid', episode_length_sec=200)
        elif key == 'merge4_n3':
            scn = merge4('zipper', norm_wave=3.0, clip_wave=1.5)
        elif key == 'merge4_pieces':
            scn = split_pieces(NETWORKS['merge4_zipper'].scenario(), MERGE4_CUTS)
        elif key == 'merge4_krauss':
            scn = copy.copy(NETWORKS['merge4_zipper'].scenario())
            scn.car_following, scn.krauss_sigma = 'krauss', 0.5
        else:
            scn = NETWORKS[key].scenario()
        _aux_scn[key] = scn
    return _aux_scn[key]


class Aux:
    """One run of the AUX table: the scenario `key` (aux_scenario) under the run of the registry entry `net` (its seed, its share of
    random actions) with E instances for `steps` control steps; what else a family needs is in `kw` (read as attributes)."""

    def __init__(self, key, net, E, steps, **kw):
        self.key, self.net_name, self.E, self.steps = key, net, E, steps
        self.__dict__.update(kw)

    def scenario(self):
        return aux_scenario(self.key)

    def net(self):
        n = copy.copy(NETWORKS[self.net_name])
        n.E, n.steps = self.E, self.steps
        return n

    def compared(self, t):
        """Is the state after control step t one the case compares?  Every `every` steps and at the entry's peak."""
        return (t > 0 and t % self.every == 0) or t == NETWORKS[self.net_name].peak or t == self.steps - 1

    def __repr__(self):
        return self.key


# E, steps, seeds and actions of the runs below are run_oracle's (train mode: instance e runs seed net.seed + e); the walks draw their
# own actions (uniform_actions) from RandomState(rng_seed) and run the train-mode seeds seed + e.
AUX = {
    # pressure_kernel against loop_pressure, both measures.  isolated_130: 260 walked lanes (chunk 2); isolated_300: 600 walked lanes
    # (chunk 3), 300 agents and 600 (agent, phase) pairs; grid_x4: 664 walked lanes (chunk 3), 1104 movements (five rounds of zeroing)
    'pressure': [Aux('isolated_130', 'isolated_130', 2, 61, every=10), Aux('isolated_300', 'isolated_300', 2, 61, every=10),
                 Aux('grid_x4', 'grid_x4', 2, 91, every=15), Aux('link62', 'link62', 3, 41, every=5),
                 Aux('merge4_yield', 'merge4_yield', 3, 41, every=5), Aux('burst', 'burst', 3, 31, every=5)],
    # the hold state [E][A][2] with A > 256: `steps` control steps of run_oracle's actions first, then the controller drives
    'hold': Aux('isolated_300', 'isolated_300', 2, 8, min_green=3, least=30, most=60),
    # pressure_reward_kernel against trainer.pressure_reward
    'reward': [Aux('isolated_130_ma2c', 'isolated_130', 2, 41, every=8, measure='count', train_mode=True, record=False),
               Aux('isolated_300', 'isolated_300', 2, 41, every=8, measure='queue', train_mode=True, record=False),
               Aux('grid_x2', 'grid_x2', 3, 61, every=12, measure='count', train_mode=False, record=False),
               Aux('ctrl8', 'ctrl8', 3, 40, every=8, measure='count', train_mode=True, record=True)],
    # greedy_kernel against the float64 rule on the oracle's observations
    'greedy': [Aux('link62', 'link62', 4, 80), Aux('merge4_zipper', 'merge4_zipper', 4, 80), Aux('grid_x2', 'grid_x2', 2, 60),
               Aux('merge4_n3', 'merge4_zipper', 4, 80)],
    # fixed_time_kernel: steps_per_phase s over `steps` control steps, twice
    'fixed': [Aux('isolated_300', 'isolated_300', 3, 9, s=2), Aux('ctrl8', 'ctrl8', 2, 9, s=1), Aux('ctrl8', 'ctrl8', 2, 9, s=3)],
    # the trace and the lane data of one handle against the oracle's vehicles after every second; steps None: to the end of the episode;
    # watch: the instances an oracle follows
    'walk': [Aux('isolated_130_200s', 'isolated_130', 2, None, period=55, watch=[1], seed=21, rng_seed=3),
             Aux('burst', 'burst', 3, None, period=40, watch=[0, 2], seed=22, rng_seed=4),
             Aux('ctrl8', 'ctrl8', 2, None, period=56, watch=[0, 1], seed=23, rng_seed=5),
             Aux('ctrl1', 'ctrl1', 2, None, period=7, watch=[0, 1], seed=24, rng_seed=6),
             Aux('merge4_pieces', 'merge4_zipper', 3, None, period=60, watch=[0, 2], seed=25, rng_seed=7),
             Aux('grid_x2', 'grid_x2', 2, 60, period=60, watch=[1], seed=26, rng_seed=8),
             Aux('merge4_krauss', 'merge4_zipper', 3, None, period=60, watch=[1, 2], seed=27, rng_seed=9),
             # the insertion windows and the choice tables in time, vehicle by vehicle (every stream has routes of its own there)
             Aux('windows_on_lane', 'windows_on_lane', 3, None, period=45, watch=[0, 2], seed=29, rng_seed=11),
             Aux('ratios_in_time', 'ratios_in_time', 3, None, period=50, watch=[0, 1], seed=30, rng_seed=12)],
    'trace254': Aux('isolated_254', 'isolated_254', 2, 12, watch=[1], seed=28, rng_seed=10),
    # tsc_env_set_demand on windows(): instance e runs column e of windows_columns; isolated_254: demand_kernel on a 254 x 3 grid
    'demand': Aux('windows', 'windows', 4, WINDOWS_EPISODE, seed=600),
    'demand254': Aux('isolated_254', 'isolated_254', 3, 40, seed=610),
}


def aux_run(case, **kw):
    """run_oracle over an AUX case."""
    return run_oracle(case.scenario(), case.net(), E=case.E, **kw)


def walk_steps(case):
    scn = case.scenario()
    return -(-int(scn.episode_length_sec) // int(scn.control_interval_sec)) if case.steps is None else case.steps


# the exhaustive check of greedy_kernel's float32 -> float64 recovery: agent 0 of merge4, every tuple of 0 .. 8 vehicles on its four
# lanes.  Under the registry's phases the first candidate ('GGGG') holds every lane and always wins, and candidates of two lanes each
# can only tie on the same two addends; here one lane alone comes first and pairs follow, so that 3 / 5 against 1 / 5 + 2 / 5 -- a tie
# on the float32 entries, which the first candidate would win, and 0.6 < 0.6000000000000001 in float64 -- decides the action
GREEDY_PHASES = ('rrrG', 'GGrr', 'GrGr', 'rGGr')
GREEDY_NORMS = [(3.0, 1.5), (5.0, 1.1), (7.0, 0.9)]         # (norm_wave, clip_wave): the clip lies below 8 / norm_wave


def greedy_exhaustive(norm, clip):
    """-> (scn, counts int [6561, 4], the float32 observation entries [6561, 4] = float32(min(c / norm, clip)), the float64 rule's
    action [6561], the action of the rule on the float32 entries added in float64 [6561], ... added in float32 [6561])."""
    import itertools
    scn = merge4('zipper', phases0=GREEDY_PHASES, norm_wave=norm, clip_wave=clip)
    n_cand, term, action = scn.greedy_controller_tables()
    assert int(scn.agent_nlane[0]) == 4 and int(n_cand[0]) == 4
    tab = (term[0], action[0], n_cand[0])
    counts = np.array(list(itertools.product(range(9), repeat=4)), np.int64)
    ob64 = np.clip(counts.astype(np.float64) / norm, 0, clip)           # (OracleEnv._norm_clip)
    ob32 = ob64.astype(np.float32)
    want = np.array([greedy_rule(tab, row)[0] for row in ob64], np.int32)
    naive64 = np.array([greedy_rule(tab, row.astype(np.float64))[0] for row in ob32], np.int32)
    naive32 = np.zeros(len(counts), np.int32)
    for i, row in enumerate(ob32):
        flows = []
        for c in range(4):
            f = np.float32(0.0)
            for j in term[0][c]:
                if j >= 0:
                    f = np.float32(f + row[j])
            flows.append(f)
        naive32[i] = action[0][int(np.argmax(flows))]
    return scn, counts, ob32, want, naive64, naive32


# ---------------------------------------------------------------------------
# generated networks: the seeded sweep of tests/test_networks_random_host.py / tests/test_networks_random_gpu.py
# ---------------------------------------------------------------------------
# Lane lengths in m: float32 values (12, 17, 30, 50, 75, 120, 150, 200) mixed with values float32 cannot hold (15.3, 20.1, 23.4, 24.9,
# 33.3, 41.7, 49.9, 61.7, 99.9, 187.3, 209.9); ten lie below 50 m (the detector starts at 0), six below 25 m; 209.9 m is just inside
# the 28 x 7.5 m check_limits accepts, and only lanes from about 175 m up can hold the 25 standing vehicles past the hand-off cap.
RANDOM_SHORT = (12.0, 15.3, 17.0, 20.1, 23.4, 24.9, 30.0, 33.3, 41.7, 49.9)
RANDOM_MID = (50.0, 61.7, 75.0, 99.9, 120.0, 150.0)
RANDOM_LONG = (187.3, 200.0, 209.9)
RANDOM_VMAX = (5.0, 7.3, 8.33, 11.0, 13.89, 16.7, 20.0, 25.0)           # m/s
_RANDOM_NET = {}


def _random_tables(seed):
    """The draws of random_network(seed): -> (arguments of compile_network, the run).  One RandomState(seed), consumed in one fixed
    order; nothing else is random."""
    rng = np.random.RandomState(seed)
    pick = lambda seq: seq[int(rng.randint(len(seq)))]
    A = int(rng.randint(1, 9))
    merge = 'zipper' if rng.rand() < 0.5 else 'yield'
    interval = int(rng.randint(1, 9))
    yellow = int(rng.randint(0, min(3, interval - 1) + 1))
    steps = int(rng.randint(30, 61))
    T = steps * interval
    lanes, routes, entries = [], [[] for _ in range(12)], []       # entries: (entry lane, the routes that begin on it)
    nlink, linkof = [0] * A, {}

    def lane(kind, node):
        """A new lane: kind -> the share of short, middle and long lengths."""
        p = {'main': (0.35, 0.35, 0.30), 'feeder': (0.45, 0.40, 0.15), 'short': (0.8, 0.2, 0.0), 'exit': (0.4, 0.5, 0.1)}[kind]
        table = (RANDOM_SHORT, RANDOM_MID, RANDOM_LONG)[int(rng.choice(3, p=p))]
        lanes.append((pick(table), pick(RANDOM_VMAX), node))
        return len(lanes) - 1

    def link(l, nx):
        """The signal link of the movement l -> nx (-1: l has no signal): one link per movement, now and then behind a link that no
        lane uses."""
        a = lanes[l][2]
        if a < 0:
            return -1
        if (l, nx) not in linkof:
            if nlink[a] < 10 and rng.rand() < 0.15:
                nlink[a] += 1
            linkof[(l, nx)] = nlink[a]
            nlink[a] += 1
        return linkof[(l, nx)]

    def path(seq):
        return [(l, link(l, seq[i + 1]) if i + 1 < len(seq) else -1) for i, l in enumerate(seq)]

    def part(ag, max_lanes):
        """One connected part over the agents ag: a main road of at least three signalised lanes in a row (route 0), an unsignalised
        lane inside it, exits where the main road diverges (one lane, several routes, different next lanes and links), feeders that
        merge into main-road lanes (2 - 4 feeders per lane, the merged lane held back by its own junction) and enter on routes of
        their own.  Route indices start at 0 in every part."""
        n, first = len(ag), len(lanes)
        room = lambda k: len(lanes) - first + k <= max_lanes
        m = max(n, int(rng.randint(3, 6)))
        main = [lane('main', ag[i * n // m]) for i in range(m)]
        if rng.rand() < 0.4:
            main.insert(int(rng.randint(1, m)), lane('short', -1))
        main.append(lane('exit', -1))
        r, starts = 1, [0]
        exits = {}                                                  # position on the main road -> its exit lane
        for _ in range(int(rng.randint(0, 3))):
            i = int(rng.randint(0, len(main) - 1))
            a = lanes[main[i]][2]
            if i in exits or not room(1) or r >= 12 or (a >= 0 and nlink[a] > 8):
                continue
            exits[i] = lane('exit', -1)
            routes[r].append(path(main[:i + 1] + [exits[i]]))
            starts.append(r)
            r += 1
        routes[0].append(path(main))
        entries.append((main[0], starts))
        for j in range(1, len(main)):
            if rng.rand() >= 0.55:
                continue
            for _ in range(int(rng.choice([1, 2, 3], p=[0.35, 0.3, 0.35]))):
                a = lanes[main[j - 1]][2]
                if a < 0 or rng.rand() < 0.15 or nlink[a] > 9:
                    a = -1
                if not room(1) or r >= 12:
                    break
                f = lane('feeder', a)
                after = [i for i in exits if i >= j]
                if after and rng.rand() < 0.4:
                    i = pick(after)
                    routes[r].append(path([f] + main[j:i + 1] + [exits[i]]))
                else:
                    routes[r].append(path([f] + main[j:]))
                entries.append((f, [r]))
                r += 1

    if A >= 4 and rng.rand() < 0.4:                                 # two disjoint parts that share their route indices
        cut = int(rng.randint(1, A))
        part(list(range(cut)), 18)
        part(list(range(cut, A)), 18)
    else:
        part(list(range(A)), 36)
    for _ in range(int(rng.randint(0, 4))):                         # lanes no route uses
        lane('exit', -1)
    while routes and not routes[-1]:
        routes.pop()

    phases = []
    for a in range(A):
        used = sorted(k for (l, _), k in linkof.items() if lanes[l][2] == a)
        nl = min(12, nlink[a] + int(rng.randint(0, 3)))
        P = int(rng.randint(2, 9))
        rows = [list(rng.choice(list('Ggr'), size=nl, p=[0.35, 0.15, 0.5])) for _ in range(P)]
        dead = int(rng.randint(P)) if P >= 3 and rng.rand() < 0.3 else -1          # a phase that opens nothing
        if dead >= 0:
            rows[dead] = ['r'] * nl
        for k in used:                                              # every used link is open in some phase
            if not any(row[k] in 'Gg' for row in rows):
                p = int(rng.choice([q for q in range(P) if q != dead]))
                rows[p][k] = 'G' if rng.rand() < 0.7 else 'g'
        phases.append([''.join(row) for row in rows])

    streams, flows = [], []
    heavy = int(rng.randint(len(entries)))
    for i, (l, starts) in enumerate(entries):
        ns = int(rng.choice([1, 2, 3, 4, 6, 8], p=[0.35, 0.25, 0.15, 0.1, 0.08, 0.07]))
        base = float(pick((150, 400, 800, 1400, 2200, 3000)))
        for q in range(ns):
            s = len(streams)
            streams.append((l, int(pick(starts))))
            for _ in range(int(rng.choice([1, 2, 3], p=[0.6, 0.3, 0.1]))):           # (several elements of a stream may overlap)
                begin = int(rng.randint(0, max(1, (2 * T) // 3)))
                kind = rng.rand()
                end = begin if kind < 0.06 else begin + int(rng.randint(1, T + 1)) if kind < 0.8 else T + int(rng.randint(1, 90))
                vph = 0 if rng.rand() < 0.05 else int(base * rng.uniform(0.3, 1.2) / np.sqrt(ns))
                flows.append((begin, end, vph, s))
            if i == heavy and q == 0:                               # one stream heavy enough to queue
                flows.append((int(rng.randint(0, 4)), T + int(rng.randint(0, 70)), int(rng.randint(1800, 3001)), s))

    agent = str(rng.choice(['ia2c', 'ma2c', 'greedy'], p=[0.3, 0.45, 0.25]))
    neighbors = []
    for a in range(A):
        others = [b for b in range(A) if b != a]
        k = int(rng.randint(0, min(4, len(others)) + 1))
        neighbors.append([int(b) for b in rng.choice(others, size=k, replace=False)] if k else [])
    env_kw = dict(control_interval_sec=interval, yellow_interval_sec=yellow, episode_length_sec=T,
                  teleport_sec=int(pick((15, 40, 120, 600))), objective=pick(('queue', 'wait', 'hybrid')),
                  has_wait_state=bool(rng.rand() < 0.6), queue_cap=int(pick((-1, 3, 10))), coop_gamma=float(pick((0.5, 0.75, 0.9))),
                  norm_wave=float(pick((1.0, 3.0, 5.0))), clip_wave=float(pick((0.8, 2.0, 30.0))),
                  norm_wait=float(pick((7.0, 30.0, 100.0))), clip_wait=float(pick((0.5, 2.0, 100.0))),
                  coef_wait=float(pick((0.05, 0.2, 1.0))))
    run = dict(E=2, steps=steps, p_random=float(rng.uniform(0.1, 0.9)), seed=30000 + 16 * int(seed),
               peak=int(rng.randint(steps // 2, steps)), sigma=float(pick((0.0, 0.3, 0.5, 1.0))))
    args = dict(name='random_%d' % seed, agent=agent, lanes=lanes, routes=routes, phases=phases, neighbors=neighbors, flows=flows,
                streams=streams, merge=merge, **env_kw)
    return args, run


def random_network(seed):
    """The Net of a generated network, a pure function of the seed (one np.random.RandomState(seed), no global state; the Net is
    kept, so that every caller shares one compiled scenario).  The scenario goes through compile_network with check = True: it is one
    that Scenario.check_limits and tsc_env_create accept, and a draw they refuse is a bug of the generator.

    What is drawn, every axis inside its declared limit:
    * size: 1 - 8 agents, at most 40 lanes and 12 route indices (two disjoint parts share theirs), 2 - 8 phases and 1 - 12 signal
      links per agent, some links used by no lane;
    * lanes: lengths from RANDOM_SHORT / RANDOM_MID / RANDOM_LONG (12 - 209.9 m), speed limits from RANDOM_VMAX (5 - 25 m/s), so
      that many lanes have a limit above their length (a vehicle may cross the whole lane in one second);
    * topology: a main road of at least three signalised lanes on one route, an unsignalised lane inside it, exits where a lane
      diverges (several routes, different next lanes and links), merges of 2 - 4 feeders under the network's one merge kind
      ('zipper' or 'yield'), merged lanes held back by their own junction, lanes no route uses;
    * phases: strings over G, g, r; every used link is open in some phase of its agent; some phases open nothing;
    * demand: 1 - 8 streams per entry lane, 0 - 3000 veh/h, windows that begin and end at any second, overlap, are empty or end past
      the episode, and one stream heavy enough to queue;
    * configuration: control interval 1 - 8 s, yellow 0 - min(3, interval - 1) s, teleport after 15 / 40 / 120 / 600 s, agent kind
      (MA2C and IA2C with neighbour lists of 0 - 4 agents, MA2C with a drawn coop_gamma), objective, has_wait_state, queue_cap,
      norms, clips and coef_wait;
    * run: E = 2, 30 - 60 control steps (the episode ends with the last one), 10 - 90 % random actions, peak in the second half;
      net.sigma is the Krauss sigma of the Krauss variant.
    Not drawn: two-lane streets (lane_sib, MICROSIM_SPEC.md rule 10) -- random_street_network(seed) adds them to the same
    networks from a generator of its own -- nor per-instance demand, trace and lane data, whose walks run on the hand-made networks
    and on street_walks()."""
    if seed not in _RANDOM_NET:
        args, run = _random_tables(seed)
        net = Net(lambda: compile_network(**_random_tables(seed)[0]), 'generated network, seed %d' % seed, None, run['E'], run['steps'],
                  run['p_random'], run['seed'], run['peak'], 5.0)
        net.sigma, net.name = run['sigma'], args['name']
        _RANDOM_NET[seed] = net
    return _RANDOM_NET[seed]


# The 96 seeds of the sweep, chosen on the host: tests/test_networks_random_host.py states what the sample must reach (coverage
# quotas over the oracle's runs).  0 - 98 without 22, 26 and 78: in those three no vehicle reaches the end of its route before the
# episode ends (the used links open late or the only exit is held), a run that compares little.
RANDOM_SEEDS = [s for s in range(99) if s not in (22, 26, 78)]
# the 24 networks of the kernel-variant and controller cases: 14 with teleports, 13 with a lane at 25 or more vehicles, 14 zipper and
# 10 yield networks, every control interval from 1 to 8 s
RANDOM_VARIANT_SEEDS = RANDOM_SEEDS[:24]


# ---------------------------------------------------------------------------
# generated networks with redrawn stream tables: tests/test_streams_host.py / tests/test_streams_gpu.py
# ---------------------------------------------------------------------------
_RANDOM_STREAM_NET = {}
VEH_LEN_M = 5.0                 # MICROSIM_SPEC.md rule 6: a window shorter than one vehicle never inserts


def _random_stream_tables(seed):
    """The arguments of random_network(seed) with the stream tables redrawn from a generator of their own, RandomState(10000 + seed):
    -> (arguments of compile_network, the run).  Lanes, routes, phases, flows and the configuration are _random_tables' own."""
    args, run = _random_tables(seed)
    rng = np.random.RandomState(10_000 + seed)
    pick = lambda seq: seq[int(rng.randint(len(seq)))]
    lanes, routes = args['lanes'], args['routes']
    NI, ilen = int(rng.randint(1, 5)), int(rng.randint(3, 41))
    streams = []
    for l, r in args['streams']:
        starts = [q for q, paths in enumerate(routes) if any(p[0][0] == l for p in paths)]      # the routes that begin on the lane
        assert r in starts
        u = rng.rand()
        mode = 0 if len(starts) < 2 or u >= 0.85 else 1 if u < 0.5 else 2
        if mode == 1:                           # per interval 1 .. len(starts) + 1 pairs, ascending weights that need not reach 65536
            choice = []
            for _ in range(NI):
                k = int(rng.randint(1, len(starts) + 2))
                w = sorted(int(x) for x in rng.randint(0, 65537, k))
                if rng.rand() < 0.5:
                    w[-1] = 65536
                choice.append([(int(pick(starts)), x) for x in w])
        elif mode == 2:
            choice = [[(int(pick(starts)), 65536) for _ in range(int(rng.randint(1, len(starts) + 2)))]]
        else:
            choice = [[(r, 65536)]]
        s = dict(lane=l, mode=mode, choice=choice)
        L = lanes[l][0]
        cuts = [0.0] + [x for x in RANDOM_SHORT + RANDOM_MID + RANDOM_LONG if x <= L]
        pairs = [(a, b) for a in cuts for b in cuts if b - a >= VEH_LEN_M and (a, b) != (0.0, L)]
        if rng.rand() < 0.5 and pairs:          # a window inside the lane, at least one vehicle long
            s['origin'], s['limit'] = pick(pairs)
        streams.append(s)
    return dict(args, name='random_stream_%d' % seed, streams=streams, choice_interval_sec=ilen), run


def random_stream_network(seed):
    """random_network(seed) with other stream tables -- the network, the demand, the configuration and the run are the same, a pure
    function of the seed.  A stream on an entry lane where two or more routes begin is a mode-1 stream (50 %: 1 - 4 intervals of
    3 - 40 s for the whole scenario, per interval 1 to len(starts) + 1 pairs with ascending weights that reach 65536 half of the
    time), a mode-2 stream (35 %: 1 to len(starts) + 1 candidates, repeats allowed) or keeps its route; half of all streams
    insert on a window inside their lane whose ends come from the length tables."""
    if seed not in _RANDOM_STREAM_NET:
        args, run = _random_stream_tables(seed)
        net = Net(lambda: compile_network(**_random_stream_tables(seed)[0]), 'generated network with redrawn stream tables, seed %d' % seed,
                  None, run['E'], run['steps'], run['p_random'], run['seed'], run['peak'], 5.0)
        net.sigma, net.name = run['sigma'], args['name']
        _RANDOM_STREAM_NET[seed] = net
    return _RANDOM_STREAM_NET[seed]


# The 24 seeds of the stream sweep, chosen on the host among RANDOM_SEEDS: few generated networks have an entry lane on which two routes
# begin, and only those can carry a mode-1 or a mode-2 stream.  tests/test_streams_host.py states what the sample must reach.  The
# first eight also run under every kernel variant: small networks in which most of the events occur.
RANDOM_STREAM_SEEDS = [10, 90, 27, 51, 20, 24, 83, 41, 87, 30, 25, 12, 14, 17, 23, 33, 38, 40, 44, 45, 48, 71, 77, 85]


# ---------------------------------------------------------------------------
# generated networks with two-lane streets (MICROSIM_SPEC.md rule 10): tests/test_streets_host.py / tests/test_streets_gpu.py
# ---------------------------------------------------------------------------
_RANDOM_STREET_NET = {}
STREET_MAX_LANES = 40
STREET_MAX_LINKS = 12
HEAVY_WINDOW = (12.0, 17.0)     # m: x <= 12 on the twin, x >= 17 + 5 on the serving lane, and 22 - 5 - 12 >= the standstill gap of 2
ROOM_LEN_M = 187.3              # the shortest length of RANDOM_LONG: 26 standing vehicles, more than the CAP - 8 = 20 of the room test


def _random_street_tables(seed):
    """The arguments of random_network(seed) with some lanes turned into two-lane streets, from a generator of its own,
    RandomState(20000 + seed), consumed in one fixed order: -> (arguments of compile_network, the run).  A street is a lane of
    _random_tables and a twin of the same length and downstream agent behind the last lane; per route through it a draw says which
    of the two the connection enters and which one serves the next hop."""
    args, run = _random_tables(seed)
    rng = np.random.RandomState(20_000 + seed)
    pick = lambda seq: seq[int(rng.randint(len(seq)))]
    lanes = list(args['lanes'])
    routes = [[list(p) for p in paths] for paths in args['routes']]
    phases = [list(p) for p in args['phases']]
    streams, flows = list(args['streams']), list(args['flows'])
    T = int(args['episode_length_sec'])
    n_old = len(lanes)

    uses = {}                                                       # lane -> [(route, path index)] of the paths through it
    for r, paths in enumerate(routes):
        for pi, path in enumerate(paths):
            for l, _ in path:
                uses.setdefault(l, []).append((r, pi))
    at = lambda path, l: [x[0] for x in path].index(l)
    hops = lambda: [(path, j) for paths in routes for path in paths for j in range(len(path))]
    # the junction feeders of a lane and the lanes its connections enter, as the paths stand now (a CHANGE hop hands over sideways)
    feeders = lambda l: {path[j - 1][0] for path, j in hops() if path[j][0] == l and j > 0 and path[j - 1][1] != CHANGE}
    nexts = lambda l: {path[j + 1][0] for path, j in hops() if path[j][0] == l and j + 1 < len(path) and path[j][1] != CHANGE}
    paired = lambda l: any(l in pair for pair in siblings)
    entry_lanes = {l for l, _ in streams}
    ends = {path[-1][0] for paths in routes for path in paths}
    chosen, siblings, twin_link = [], [], {}
    behind = []                                                     # the streams that insert on the heavy street's twin

    def fits(l):
        a = lanes[l][2]
        return (l in uses and l not in chosen and len(feeders(l)) <= MAX_UP - 1 and len(lanes) < STREET_MAX_LANES
                and all(len(feeders(nx)) + 1 + paired(nx) <= MAX_UP for nx in nexts(l))        # (the twin feeds them too)
                and (a < 0 or len(phases[a][0]) + len(nexts(l)) <= STREET_MAX_LINKS))

    def twin(l):
        """The second lane of the street of lane l: the same length and downstream agent, half of the time another speed limit."""
        length, vmax, node = lanes[l]
        lanes.append((length, vmax if rng.rand() < 0.5 else pick(RANDOM_VMAX), node))
        chosen.append(l)
        siblings.append((l, len(lanes) - 1))
        return len(lanes) - 1

    def link(l2, nx):
        """The signal link of the twin's movement l2 -> nx: a link of its own behind the agent's last one, open in some phase."""
        a = lanes[l2][2]
        if a < 0 or nx is None:
            return -1
        if (l2, nx) not in twin_link:
            twin_link[(l2, nx)] = len(phases[a][0])
            col = list(rng.choice(list('Ggr'), size=len(phases[a]), p=[0.35, 0.15, 0.5]))
            if not any(c in 'Gg' for c in col):
                col[int(rng.randint(len(col)))] = 'G'
            phases[a] = [p + c for p, c in zip(phases[a], col)]
        return twin_link[(l2, nx)]

    def connect(l, l2, r, pi, mode):
        """Route r's hop over the street (l, l2) -- 'stay': enters l, which serves it; 'change': enters l, l2 serves it; 'twin':
        enters l2, which serves it; 'back': enters l2, l serves it."""
        path = routes[r][pi]
        i = at(path, l)
        k = path[i][1]
        nx = path[i + 1][0] if i + 1 < len(path) else None
        hop = {'stay': [(l, k)], 'change': [(l, CHANGE), (l2, link(l2, nx))], 'twin': [(l2, link(l2, nx))],
               'back': [(l2, CHANGE), (l, k)]}[mode]
        path[i:i + 1] = hop

    # the designated heavy street: the entry lane of the heaviest stream, made long enough to hold more than CAP - 8 vehicles; the
    # heavy stream inserts on the lane that serves it, the lane's other streams mostly on the other one (one is added if there is
    # none).  The streams of the twin insert within HEAVY_WINDOW[0] m, those of the serving lane beyond HEAVY_WINDOW[1] m (`windows`,
    # written into the stream tables at the end): a vehicle inserted on the twin stands behind the serving lane's tail by more
    # than the gap test asks, so that what keeps it out is the serving lane's count alone
    windows = {}
    load = [sum(max(0, min(e, T) - b) * v for b, e, v, s_ in flows if s_ == s) for s in range(len(streams))]
    hs = int(np.argmax(load))
    lh = streams[hs][0]
    if fits(lh):
        if lanes[lh][0] < ROOM_LEN_M:
            lanes[lh] = (pick(RANDOM_LONG),) + tuple(lanes[lh][1:])
        l2 = twin(lh)
        for s, (l, r) in enumerate(streams):
            if l == lh and s != hs and rng.rand() < 0.7:
                streams[s] = (l2, r)
                behind.append(s)
        if not behind:
            streams.append((l2, streams[hs][1]))
            flows.append((int(rng.randint(0, 10)), T + int(rng.randint(0, 30)), int(rng.randint(400, 1201)), len(streams) - 1))
            behind.append(len(streams) - 1)
        windows = {s: (0.0, HEAVY_WINDOW[0]) if s in behind else (HEAVY_WINDOW[1], lanes[lh][0])
                   for s, (l, _) in enumerate(streams) if l in (lh, l2)}

    # one street per kind (when the network has a lane of the kind and the draw says so), then up to two more
    kinds = [
        ('entry', 0.6, lambda l: l in entry_lanes),
        ('merge', 0.75, lambda l: len(feeders(l)) >= 2),
        ('fast', 0.9, lambda l: lanes[l][1] > lanes[l][0]),
        ('short', 0.75, lambda l: lanes[l][0] < 50.0),
        ('unsignalised', 0.7, lambda l: lanes[l][2] < 0 and l not in ends),
        ('end', 1.0, lambda l: l in ends and len(uses[l]) == max(len(uses[x]) for x in ends)),
        ('any', 0.5, lambda l: True), ('any', 0.5, lambda l: True)]
    for kind, p, is_kind in kinds:
        cand = [l for l in range(n_old) if fits(l) and is_kind(l)]
        if rng.rand() >= p or not cand:
            continue
        l = pick(cand)
        l2 = twin(l)
        if rng.rand() < 0.12:                                       # a second lane that no route uses
            continue
        inner = [(r, pi) for r, pi in uses[l] if at(routes[r][pi], l) > 0]
        first = [(r, pi) for r, pi in uses[l] if at(routes[r][pi], l) == 0]
        modes = [str(rng.choice(['stay', 'change', 'twin', 'back'], p=[0.25, 0.35, 0.15, 0.25])) for _ in inner]
        if kind == 'end':                                           # both lanes carry traffic that leaves at speed
            modes = [('stay', 'change', 'twin', 'back')[j % 4] for j in range(len(inner))]
        moved = any(m in ('change', 'back') for m in modes)
        for r, pi in first:                                         # a route that begins on the street: one lane serves it (the
            serve = l if rng.rand() < 0.6 else l2                   # path names that one), its streams insert on either
            if serve == l2:
                connect(l, l2, r, pi, 'twin')
            for s in [s for s, (le, rs) in enumerate(streams) if le == l and rs == r]:
                on_wrong = bool(rng.rand() < 0.5) or not moved
                streams[s] = ((l2 if serve == l else l) if on_wrong else serve, r)
                moved |= on_wrong
        if not moved and inner:                                     # every street that routes use carries a change
            modes[0] = 'change' if modes[0] == 'stay' else 'back'
        for (r, pi), mode in zip(inner, modes):
            connect(l, l2, r, pi, mode)
    for s, (lo, hi) in windows.items():
        l, r = streams[s]
        streams[s] = dict(lane=l, mode=0, choice=[[(r, 65536)]], origin=lo, limit=hi)
    return dict(args, name='random_street_%d' % seed, lanes=lanes, routes=routes, phases=phases, streams=streams, flows=flows,
                siblings=siblings), run


def random_street_network(seed):
    """random_network(seed) with two-lane streets (MICROSIM_SPEC.md rule 10) -- the lanes, routes, phases, demand, configuration and
    run of _random_tables(seed), a pure function of the seed.  Drawn, inside the declared limits (at most 40 lanes, 12 links per
    agent and MAX_UP lane_up slots, the sibling among them):
    * which lanes become streets: the entry lane of the heaviest stream, made at least 187.3 m long (the heavy stream inserts on
      the lane that serves it and fills it past the CAP - 8 vehicles of the room test, other streams insert on the lane beside it);
      then, each with its own probability and where the network has one, another entry lane, a merge target with two or three
      junction feeders, a lane whose speed limit exceeds its length, a lane shorter than 50 m, an unsignalised lane, the lane on
      which the most routes end (always: its routes take the four connection kinds in turn, so that both lanes carry traffic that
      leaves at speed and a changer behind a vehicle that has just left finds the sibling's tail moving a few metres ahead -- what
      makes the clamp behind that tail bind), and up to two more of any kind;
    * the twin: the same length and downstream agent, another speed limit half of the time;
    * per route through a street which lane the connection enters and which serves the next hop -- stay, change, enter the twin,
      or enter the twin and change back, so that streets carry changes in both directions, routes end on the sibling, and the twin
      of a merge target is a merge target itself; per stream on an entry street the lane it inserts on; every street that routes
      use carries a change; one street in eight has a twin that no route uses (it lies beyond the live prefix);
    * signals: every movement of a twin has a signal link of its own behind the agent's last one, open in some phase."""
    if seed not in _RANDOM_STREET_NET:
        args, run = _random_street_tables(seed)
        net = Net(lambda: compile_network(**_random_street_tables(seed)[0]), 'generated network with two-lane streets, seed %d' % seed,
                  None, run['E'], run['steps'], run['p_random'], run['seed'], run['peak'], 5.0)
        net.sigma, net.name = run['sigma'], args['name']
        _RANDOM_STREET_NET[seed] = net
    return _RANDOM_STREET_NET[seed]


# The 48 seeds of the street sweep, chosen on the host: 0 - 49 without 22 (no vehicle is inserted before the episode ends: no lane
# change, no arrival) and 26 (no vehicle reaches the end of its route) -- the seeds RANDOM_SEEDS leaves out for the same reason.
# tests/test_streets_host.py states what the sample must reach (floors over the oracle's runs).
RANDOM_STREET_SEEDS = [s for s in range(50) if s not in (22, 26)]
# the 16 networks of the kernel-variant, controller, trace and lane-data cases
RANDOM_STREET_VARIANT_SEEDS = RANDOM_STREET_SEEDS[:16]


# Cut positions in m, none of them a float32 value
STREET_CUTS = (13.3, 20.1, 33.3, 61.7, 90.9, 120.1, 150.7)


def street_walk_scenario(seed, krauss=False):
    """random_street_network(seed) for the trace and lane-data walk.  The trace knows a vehicle by (route, serial, entry lane) and
    serials count per stream: the streams that share an entry lane and a route become one (their flow elements add up on the
    first).  The longest street is in pieces: the lane with the lower index in four (or as many as STREET_CUTS allows below its
    length, at least two), its sibling in two or three at other positions.  krauss: under Krauss with the network's sigma."""
    args, run = _random_street_tables(seed)
    lane_route = lambda s: (s['lane'], s['choice'][0][0][0]) if isinstance(s, dict) else tuple(s)
    first, streams, renum = {}, [], []
    for s in args['streams']:
        key = lane_route(s)
        if key not in first:
            first[key] = len(streams)
            streams.append(s)
        renum.append(first[key])
    flows = [(b, e, v, renum[s]) for b, e, v, s in args['flows']]
    scn = compile_network(**dict(args, name='random_street_%d_walk' % seed, streams=streams, flows=flows))
    sib = np.asarray(scn.lane_sib)
    l = max((l for l in range(scn.n_lane) if sib[l] > l), key=lambda l: (float(scn.lane_len[l]), -l))
    below = [c for c in STREET_CUTS if c < float(scn.lane_len[l]) - 1.0]
    assert len(below) >= 2, (seed, scn.lane_len[l])
    scn = split_pieces(scn, {scn.lane_names[l]: below[:3], scn.lane_names[sib[l]]: below[1:3] if len(below) > 2 else below[1:]})
    if krauss:
        scn.car_following, scn.krauss_sigma = 'krauss', run['sigma']
    return scn


class StreetWalk(Aux):
    """A walk case (AUX['walk']) over street_walk_scenario(seed)."""

    def __init__(self, seed, krauss, period_steps):
        net = random_street_network(seed)
        scn = street_walk_scenario(seed, krauss)
        Aux.__init__(self, 'street_%d%s' % (seed, '_krauss' if krauss else ''), None, net.E, None, watch=[0, 1], seed=net.seed,
                     rng_seed=700 + seed, period=period_steps * int(scn.control_interval_sec))
        self._scn = scn

    def scenario(self):
        return self._scn


_STREET_WALKS = []


def street_walks():
    """The six walk cases of the street sweep, built once: six of RANDOM_STREET_VARIANT_SEEDS (episodes of 52 to 228 s; zipper and
    yield; room refusals in 3, 11 and 15, teleports in 4 and 8), two of them under Krauss with sigma 1.0.  The lane-data period is a
    number of control steps that does not divide the episode: the last interval is a partial one."""
    if not _STREET_WALKS:
        _STREET_WALKS.extend(StreetWalk(seed, krauss, steps) for seed, krauss, steps in
                             ((2, False, 20), (3, True, 11), (4, False, 9), (8, True, 17), (11, False, 12), (15, False, 7)))
    return _STREET_WALKS


def wrong_lane_pairs(scn):
    """(lane, route) pairs of signalised lanes that do not serve the route while their sibling does."""
    sib, nxt = np.asarray(scn.lane_sib), np.asarray(scn.mv_next)
    return [(l, r) for l in range(scn.n_lane) if sib[l] >= 0 and scn.lane_node[l] >= 0 for r in range(scn.n_route)
            if nxt[l, r] < -1 and nxt[sib[l], r] >= -1]


def walk_lane_changes(case):
    """{watched instance: the lane changes the oracle counts (ms.lanechange_counts) over the walk of `case`}: the oracle's side of
    the walk alone, under the walk's own actions."""
    from tests import env_harness as H
    scn = case.scenario()
    with H.walk_context(case):
        orc = H.WalkOracles(case)
        rng = np.random.RandomState(case.rng_seed)
        for _ in range(walk_steps(case)):
            orc.step(H.uniform_actions(scn, rng, case.E))
    return {e: int(o.ms.lanechange_counts()['changes']) for e, o in orc.orc.items()}


def _stream_tables_changed(change, base=ratios_in_time):
    """ratios_in_time with its stream tables changed in place by change(scn): a scenario for REFUSED (never run)."""
    scn = copy.copy(base())
    scn.stream_mode, scn.stream_choice = scn.stream_mode.copy(), scn.stream_choice.copy()
    change(scn)
    return scn


def _set(scn, field, index, value):
    getattr(scn, field)[index] = value


# the stream tables: the refusals of Scenario.check_limits and of tsc_env_create have the same words
REFUSED.update({
    'stream_route9': (lambda: _stream_tables_changed(lambda scn: _set(scn, 'stream_choice', (1, 3, 0, 0), scn.n_route)),
                      'stream 1 names route 9 of 9', 'stream 1 names route 9 of 9'),
    'stream_mode3': (lambda: _stream_tables_changed(lambda scn: _set(scn, 'stream_mode', 2, 3)), 'stream 2 has mode 3', 'stream 2 has mode 3'),
    'stream_no_route': (lambda: _stream_tables_changed(lambda scn: _set(scn, 'stream_choice', (3, 0, 0, 0), -1)),     # (a mode-0 stream)
                        'stream 3 has no route in interval 0', 'stream 3 has no route in interval 0'),
    # a mode-1 stream whose table of interval 2 begins with a pad: in that interval the kernel would take route -1
    'stream_no_route_later': (lambda: _stream_tables_changed(lambda scn: _set(scn, 'stream_choice', (1, 2, 0, 0), -1)),
                              'stream 1 has no route in interval 2', 'stream 1 has no route in interval 2'),
    'stream_interval0': (lambda: _stream_tables_changed(lambda scn: setattr(scn, 'choice_interval_sec', 0)),
                         'incomplete stream tables', 'incomplete stream tables'),
})


def two_lane():
    """An entry lane (0) into a two-lane street (1, 2) with one exit (3): route 0 stays on lane 1, route 1 enters lane 1 and moves
    over to lane 2.  The smallest network with a sibling that is also fed by a junction: lane_up[1] = (2, 0)."""
    lanes = [(100.0, 13.89, 0), (150.0, 13.89, 1), (150.0, 13.89, 1), (100.0, 13.89, -1)]
    routes = [[[(0, 0), (1, 0), (3, -1)]], [[(0, 0), (1, CHANGE), (2, 1), (3, -1)]]]
    return compile_network('two_lane', 'ia2c', lanes, routes, [['G', 'r'], ['GG', 'Gr', 'rG']], [[1], [0]],
                           [(0, 300, 500, 0), (0, 300, 500, 1)], siblings=[(1, 2)], episode_length_sec=300, teleport_sec=120)


def _two_lane_changed(change):
    """two_lane with its street tables changed in place by change(scn, l, s), l a street lane with a junction feeder and s its
    sibling: a scenario for REFUSED (never run)."""
    scn = copy.copy(two_lane())
    scn.lane_sib, scn.lane_len, scn.lane_up = scn.lane_sib.copy(), scn.lane_len.copy(), scn.lane_up.copy()
    l = int(np.flatnonzero((scn.lane_sib >= 0) & (scn.lane_up[:, 1] >= 0))[0])
    change(scn, l, int(scn.lane_sib[l]))
    return scn


def _swap_first_two(scn, l, s):
    scn.lane_up[l, :2] = scn.lane_up[l, 1::-1]


# the domain of lane_sib (MICROSIM_SPEC.md rule 10): the refusals of Scenario.check_limits and of tsc_env_create have the same words
REFUSED.update({
    'sib_one_way': (lambda: _two_lane_changed(lambda scn, l, s: _set(scn, 'lane_sib', s, -1)),
                    'names sibling lane [0-9]+, whose sibling is lane -1', 'names sibling lane [0-9]+, whose sibling is lane -1'),
    'sib_length': (lambda: _two_lane_changed(lambda scn, l, s: _set(scn, 'lane_len', s, 149.0)),
                   'are siblings of different length', 'are siblings of different length'),
    'sib_not_first': (lambda: _two_lane_changed(_swap_first_two), 'does not list its sibling lane [0-9]+ first in lane_up',
                      'does not list its sibling lane [0-9]+ first in lane_up'),
})
