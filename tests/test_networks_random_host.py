"""The generated networks of tests/networks.py (random_network, RANDOM_SEEDS, RANDOM_VARIANT_SEEDS) on the host (no GPU, no library):
every network is run through the CPU oracle alone, over the very (E, steps, actions, seeds) tests/test_networks_random_gpu.py compares,
and what makes the sample worth running is stated as assertions -- quotas of networks in which a rule of MICROSIM_SPEC.md is reached
that the hand-made networks keep plain.  The quotas are conditions on the inputs: a changed generator or seed list that stops meeting
them fails here, not silently on the GPU.  One oracle walk per network (survey), shared by every test of the module."""
import ctypes as C

import numpy as np

from tests import env_harness as H
from tests import networks as nw

ACC = np.float32(5.0)                           # MICROSIM_SPEC.md rule 2: a head is ready when L - x < v + ACC
FULL = 25                                       # rule 4: a lane accepts hand-offs only while it holds <= 24 vehicles
_survey = {}


class _Heads:
    """Read-only view of an oracle's lanes through its own C getters, with buffers allocated once."""

    def __init__(self, ms):
        self.ms, cap = ms, ms.cap
        self.x, self.v, self.sf = (np.zeros(cap, np.float32) for _ in range(3))
        self.w, self.r, self.i = (np.zeros(cap, np.int32) for _ in range(3))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self.args = (self.x.ctypes.data_as(fp), self.v.ctypes.data_as(fp), self.w.ctypes.data_as(ip), self.r.ctypes.data_as(ip),
                     self.i.ctypes.data_as(ip), self.sf.ctypes.data_as(fp))

    def count(self, l):
        return self.ms.L.ms_lane_count(self.ms.h, l)

    def head(self, l):
        """(x, v, route, id) of lane l's first vehicle, or None."""
        if not self.count(l):
            return None
        self.ms.L.ms_lane_vehicles(self.ms.h, l, *self.args)
        return np.float32(self.x[0]), np.float32(self.v[0]), int(self.r[0]), int(self.i[0])

    def routes(self, l):
        n = self.count(l)
        if n:
            self.ms.L.ms_lane_vehicles(self.ms.h, l, *self.args)
        return self.r[:n].tolist()


def survey(seed):
    """The oracle's run of random_network(seed) -> dict of what the scenario is and of the events its run reaches (see the quota
    table of test_coverage_quotas).  Built once per seed."""
    if seed in _survey:
        return _survey[seed]
    net = nw.random_network(seed)
    scn = net.scenario()
    NL, E = scn.n_lane, net.E
    length, vmax, node = (np.asarray(x) for x in (scn.lane_len, scn.lane_vmax, scn.lane_node))
    nxt, link = np.asarray(scn.mv_next), np.asarray(scn.mv_link)
    wide = [l for l in range(NL) if (scn.lane_up[l] >= 0).sum() >= 3]
    fast = [l for l in range(NL) if vmax[l] > length[l]]
    fork = [l for l in range(NL) if len({int(x) for x in nxt[l] if x >= 0}) >= 2]
    inner = [l for l in range(NL) if node[l] < 0 and (nxt[l] >= 0).any() and (scn.lane_up[l] >= 0).any()]
    short_sig = [l for l in range(NL) if length[l] < 50.0 and node[l] >= 0 and l in set(scn.agent_lanes.ravel().tolist())]
    ev = dict(pending=False, full=False, fast=False, fork=False, inner=False, short_det=False, compete=False, clip_wave=False,
              clip_wait=False, queue_cap=False, yellow_pass=0, overlap=False)
    heads, watch = {}, {}

    def on_second(e, ms):
        h = heads[e]
        ev['pending'] |= ms.totals()['pending'] > 0
        ev['overlap'] |= ms.check() != 0            # (two yielding feeders sent into one lane in the same second: the later arrival is clamped)
        counts = [h.count(l) for l in range(NL)]
        ev['full'] |= max(counts) >= FULL
        ev['fast'] |= any(counts[l] for l in fast)
        ev['inner'] |= any(counts[l] for l in inner)
        for l in fork:
            if counts[l] >= 2 and not ev['fork']:
                ev['fork'] = len({int(nxt[l, r]) for r in h.routes(l) if nxt[l, r] >= 0}) >= 2
        for l in wide:                          # heads of two feeders want the lane: their route leads into it and they are ready
            ready = 0
            for u in scn.lane_up[l]:
                hd = h.head(int(u)) if u >= 0 and counts[u] else None
                ready += hd is not None and nxt[u, hd[2]] == l and np.float32(length[u]) - hd[0] < hd[1] + ACC
            ev['compete'] |= ready >= 2
        for l, vid in watch.pop(e, []):         # a head that could not stop at its yellow link a second ago: has it left the lane?
            hd = h.head(l) if counts[l] else None
            ev['yellow_pass'] += hd is None or hd[3] != vid

    def hook(e, o):
        heads[e] = _Heads(o.ms)
        plain = o.ms.set_links

        def set_links(a, ch):
            plain(a, ch)
            ch = bytes(ch)
            if b'y' not in ch:
                return
            for l in scn.agent_lanes[a, :scn.agent_nlane[a]]:       # called ahead of the second: the oracle's state is the old state
                hd = heads[e].head(int(l))
                if hd is None:
                    continue
                x, v, r, vid = hd
                k = int(link[l, r])
                if k >= 0 and nxt[l, r] >= 0 and ch[k:k + 1] == b'y' and np.float32(length[l]) - x < np.float32(v * v) / np.float32(20.0):
                    watch.setdefault(e, []).append((int(l), vid))
        o.ms.set_links = set_links

    live, done, orc = [], [None] * E, None
    for t, acts, pols, res, orc in H.run_oracle(scn, net, on_second=on_second):
        if t < 0:
            for e, o in enumerate(orc):
                hook(e, o)
            continue
        live.append(np.mean([o.ms.totals()['live'] for o in orc]))
        for e, (o, r) in enumerate(zip(orc, res)):
            if r[2] and done[e] is None:
                done[e] = t
            wave, wait, halt = o._measure()
            ev['short_det'] |= any(o.ms.lane_stats(l)[0] > 0 for l in short_sig)
            ev['clip_wave'] |= scn.clip_wave >= 0 and any((w / scn.norm_wave > scn.clip_wave).any() for w in wave)
            ev['clip_wait'] |= scn.has_wait_state and scn.agent != 'greedy' and any((w / scn.norm_wait > scn.clip_wait).any() for w in wait)
            ev['queue_cap'] |= scn.queue_cap >= 0 and scn.objective != 'wait' and any((q > scn.queue_cap).any() for q in halt)
    tot = [o.ms.totals() for o in orc]
    out = dict(ev, seed=seed, net=net, scn=scn, live=float(np.mean(live)), done=done, arrived=min(x['arrived'] for x in tot),
               teleported=sum(x['teleported'] for x in tot), merge='zipper' if scn.mv_zip.any() else 'yield' if (scn.mv_yield >= 0).any() else None,
               wide=bool(wide), interval=int(scn.control_interval_sec), yellow=int(scn.yellow_interval_sec), objective=scn.objective,
               ma2c_nb=scn.agent == 'ma2c' and any(len(n) for n in scn.neighbors))
    _survey[seed] = out
    return out


def test_random_network_is_a_pure_function_of_the_seed():
    """Built twice, the tables are equal; and the draws do not touch numpy's global generator."""
    import dataclasses
    for seed in nw.RANDOM_SEEDS:
        np.random.seed(seed)
        before = np.random.get_state()[1].copy()
        a, b = nw.compile_network(**nw._random_tables(seed)[0]), nw.compile_network(**nw._random_tables(seed)[0])
        assert (np.random.get_state()[1] == before).all()
        assert nw._random_tables(seed)[1] == nw._random_tables(seed)[1]
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype
                np.testing.assert_array_equal(x, y, err_msg='%s of seed %d' % (f.name, seed))
            else:
                assert x == y, (f.name, seed)


def test_seed_lists():
    assert len(nw.RANDOM_SEEDS) == len(set(nw.RANDOM_SEEDS)) == 96
    assert len(nw.RANDOM_VARIANT_SEEDS) == len(set(nw.RANDOM_VARIANT_SEEDS)) == 24 and set(nw.RANDOM_VARIANT_SEEDS) <= set(nw.RANDOM_SEEDS)


def test_every_network_is_inside_the_declared_limits():
    for seed in nw.RANDOM_SEEDS:
        net = nw.random_network(seed)
        scn = net.scenario().check_limits()
        used = int((np.asarray(scn.mv_next) != -2).any(axis=0).sum())
        assert 1 <= scn.n_agent <= 8 and scn.n_lane <= 40 and used == scn.n_route <= 12, seed
        assert all(2 <= n <= 8 for n in scn.n_a_ls) and all(1 <= k <= 12 for k in scn.agent_nlink), seed
        assert 12.0 <= scn.lane_len.min() and scn.lane_len.max() <= np.float32(209.9) and 5.0 <= scn.lane_vmax.min() and scn.lane_vmax.max() <= 25.0
        assert scn.lane_sib is None and np.bincount(scn.stream_entry_lane).max() <= 8 and all(len(n) <= 4 for n in scn.neighbors), seed
        assert 1 <= scn.control_interval_sec <= 8 and 0 <= scn.yellow_interval_sec <= min(3, scn.control_interval_sec - 1), seed
        assert net.E == 2 and 30 <= net.steps <= 60 and net.steps // 2 <= net.peak < net.steps and 0.1 <= net.p_random <= 0.9, seed
        assert scn.episode_length_sec == net.steps * scn.control_interval_sec and scn.teleport_sec in (15, 40, 120, 600), seed
        for a in range(scn.n_agent):            # every used link is open in some phase of its agent
            for k in {int(x) for x in scn.mv_link[scn.lane_node == a].ravel() if x >= 0}:
                assert any(p[k] in 'Gg' for p in scn.phases[a]), (seed, a, k)
    # the counterpart: every network of the street sweep has two-lane streets (its own limits: tests/test_streets_host.py)
    for seed in nw.RANDOM_STREET_SEEDS:
        scn = nw.random_street_network(seed).scenario()
        assert scn.lane_sib is not None and (scn.lane_sib >= 0).sum() >= 2 and scn.n_lane <= 40, seed


def test_every_episode_ends_inside_its_run_and_few_runs_are_degenerate():
    good = 0
    for seed in nw.RANDOM_SEEDS:
        s = survey(seed)
        assert all(d is not None and d < s['net'].steps for d in s['done']), (seed, s['done'])
        good += s['arrived'] > 0 and s['live'] >= s['net'].live_floor
    print('vehicles arrive and the mean live count is >= 5 in %d of 96 networks' % good)
    assert good >= 80


QUOTAS = [
    ('teleport removals', lambda s: s['teleported'] > 0, 16),
    ('pending > 0 at some second', lambda s: s['pending'], 32),
    ('a lane at >= 25 vehicles', lambda s: s['full'], 8),
    ('a lane with speed limit > length carries traffic', lambda s: s['fast'], 24),
    ('a signalised lane shorter than 50 m with a non-empty detector', lambda s: s['short_det'], 24),
    ('two heads want a lane of >= 3 feeders in one second', lambda s: s['compete'], 12),
    ('zipper', lambda s: s['merge'] == 'zipper', 30),
    ('yield', lambda s: s['merge'] == 'yield', 30),
    ('a diverging lane used by >= 2 routes', lambda s: s['fork'], 24),
    ('an unsignalised interior lane', lambda s: s['inner'], 12),
    ('yellow 0', lambda s: s['yellow'] == 0, 8),
    ('ma2c with a neighbour', lambda s: s['ma2c_nb'], 24),
    ('clip_wave binds', lambda s: s['clip_wave'], 12),
    ('clip_wait binds', lambda s: s['clip_wait'], 8),
    ('queue_cap binds', lambda s: s['queue_cap'], 6),
    ('a y link passed by a vehicle that can no longer stop', lambda s: s['yellow_pass'] > 0, 12),
] + [('control interval %d' % i, lambda s, i=i: s['interval'] == i, 4) for i in range(1, 9)] \
  + [('objective %s' % o, lambda s, o=o: s['objective'] == o, 16) for o in ('queue', 'wait', 'hybrid')]


def quota_counts(seeds):
    return {name: sum(bool(f(survey(s))) for s in seeds) for name, f, _ in QUOTAS}


def test_coverage_quotas():
    """Networks of the 96 in which each event occurs, against its quota."""
    got = quota_counts(nw.RANDOM_SEEDS)
    for name, _, least in QUOTAS:
        print('%-62s %3d (>= %d)' % (name, got[name], least))
    short = {name: (got[name], least) for name, _, least in QUOTAS if got[name] < least}
    assert not short, short
    # each clip also never binds in some networks
    assert got['clip_wave binds'] <= 84 and got['clip_wait binds'] <= 84


def test_variant_subset():
    ss = [survey(s) for s in nw.RANDOM_VARIANT_SEEDS]
    assert sum(s['teleported'] > 0 for s in ss) >= 6
    assert sum(s['full'] for s in ss) >= 3
    assert {s['merge'] for s in ss} >= {'zipper', 'yield'}
    assert len({s['interval'] for s in ss}) >= 4
    assert all(s['arrived'] > 0 for s in ss)          # in every instance: the recorded variant compares a trip table that is not empty
