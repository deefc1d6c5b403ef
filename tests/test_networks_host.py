"""The synthetic networks of tests/networks.py on the host (no GPU, no library): every entry of NETWORKS is run through the CPU oracle
alone, over the very (E, steps, actions, seeds) tests/test_networks_gpu.py compares, and the limit the entry exists for is stated as
an assertion -- a network that stops reaching its limit (a changed compiler, another seed) fails here, not silently on the GPU."""
import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import build_large_grid
from tests import networks as nw

ACC = 5.0                                       # MICROSIM_SPEC.md: a head is ready when L - x < v + ACC (the zipper's test)


def _run(name, on_second=None, on_step=None):
    """The oracle's run of an entry -> dict(live = mean vehicles per instance and control step, done = [E] first step with done,
    orc = the OracleEnvs after the run)."""
    net = nw.NETWORKS[name]
    scn = net.scenario()
    live, done, orc = [], [None] * net.E, None
    for t, acts, pols, res, orc in nw.run_oracle(scn, net, on_second=on_second):
        if t < 0:
            continue
        live.append(np.mean([o.ms.totals()['live'] for o in orc]))
        for e, r in enumerate(res):
            if r[2] and done[e] is None:
                done[e] = t
        if on_step is not None:
            on_step(t, res, orc)
    for o in orc:
        assert o.ms.check() == 0
    return dict(live=float(np.mean(live)), done=done, orc=orc, net=net, scn=scn)


def _eight_accumulators(a):
    """numpy's sum of one block (n <= 128), whatever n: the order csrc/tsc_env.hip's np_sum had for every n before it split."""
    a = [float(x) for x in a]
    r = a[:8]
    i = 8
    while i < len(a) - len(a) % 8:
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[i:]:
        res += x
    return res


def _common(out):
    """What every entry must show: the run reaches `done` inside its steps, and the roads are not empty."""
    net = out['net']
    print('%s: mean live vehicles %.1f (floor %.1f), done at %s of %d steps' % (out['scn'].name, out['live'], net.live_floor, out['done'], net.steps))
    assert out['live'] > net.live_floor
    assert all(d is not None and d < net.steps for d in out['done']), out['done']
    assert 0 <= net.peak < net.steps


def test_numpy_pairwise_sum_is_np_sum_for_every_length_to_300():
    """oracle.env_oracle.numpy_pairwise_sum, the plain restatement of np.sum's order that csrc/tsc_env.hip's np_sum follows: equal to
    np.sum bit for bit for every length from 1 to 300 (one block up to 128, one split up to 256, two levels above), on values whose
    sum depends on the order."""
    from oracle.env_oracle import numpy_pairwise_sum
    rng = np.random.RandomState(0)
    differs = 0
    for n in range(1, 301):
        for rep in range(3):
            a = -(rng.rand(n) * 40.0 + 0.2 * rng.randint(0, 500, n))
            assert numpy_pairwise_sum(a) == float(np.sum(a)), n
            differs += n > 128 and _eight_accumulators(a) != float(np.sum(a))
    assert differs > 100                        # (the vectors do tell the two orders apart)


@pytest.mark.parametrize('k', [2, 3])
def test_tile_is_faithful(k):
    """Copy j of tile(scn, k), restricted to its own lanes, routes and agents and brought back to the base's numbering, has the
    tables of scn; everything off the blocks is 'no movement'; the live lanes are a prefix."""
    base = build_large_grid('ma2c')
    t = nw.tile(base, k)
    assert (t.n_lane, t.n_route, t.n_agent, len(t.flows)) == (k * base.n_lane, k * base.n_route, k * base.n_agent, k * len(base.flows))
    want = nw.base_block(base)
    for j in range(k):
        got = nw.tile_block(t, base, j)
        assert sorted(got) == sorted(want)
        for key in want:
            if isinstance(want[key], np.ndarray):
                np.testing.assert_array_equal(got[key], want[key], err_msg='%s of copy %d' % (key, j))
            else:
                assert list(got[key]) == list(want[key]), (key, j)
    nu = nw.reachable_prefix(t)
    assert nu == k * nw.reachable_prefix(base)
    from deeprl_signal_control_amd.scenario import lane_load
    load = lane_load(t)
    assert (load[:nu] > 0).all() and (load[nu:] == 0).all() and (np.diff(load) <= 0).all()      # sorted by load: the live lanes are the prefix


def test_registry_names_a_plan_and_a_run_for_every_network():
    for name, net in nw.NETWORKS.items():
        assert len(net.plan) == 6 and 2 <= net.E <= 4 and 60 <= net.steps <= 150, name
        scn = net.scenario()
        assert scn.episode_length_sec <= net.steps * scn.control_interval_sec, name
    assert set(nw.RECORDED) <= set(nw.NETWORKS)


def test_grid_x2_tables_pass_the_register_prefetch():
    out = _run('grid_x2')
    _common(out)
    scn = out['scn']
    nu = nw.reachable_prefix(scn)
    assert nu * scn.n_route > 8 * 256 and (nu * scn.n_route + 3) // 4 <= 4 * 256      # movement words past 8 per thread; the zipper bytes fit
    assert nu <= 192 and scn.n_lane > 256       # 256 threads; NLP = 384 matches no kSpec row


def test_grid_x4_has_more_than_256_live_lanes():
    out = _run('grid_x4')
    _common(out)
    nu = nw.reachable_prefix(out['scn'])
    assert 256 < nu <= 384 and out['scn'].n_lane <= 1024


@pytest.mark.parametrize('name,least', [('isolated_130', 10), ('isolated_254', 10), ('isolated_300', 10)])
def test_isolated_rewards_tell_np_sum_from_one_block(name, least):
    """More than 128 agents: in at least 10 control steps (of every instance together) np.sum of the local rewards differs from the
    8-accumulator order, so a device that sums one block is caught on global_reward."""
    from oracle.env_oracle import numpy_pairwise_sum
    differs = []

    def on_step(t, res, orc):
        for o, r in zip(orc, res):
            _, wait, halt = o._measure()
            local = o._reward(wait, halt)
            assert float(np.sum(local)) == r[3] == numpy_pairwise_sum(local)
            differs.append(_eight_accumulators(local) != r[3])
    out = _run(name, on_step=on_step)
    _common(out)
    print('%s: np.sum differs from one block in %d of %d (instance, step) pairs' % (name, sum(differs), len(differs)))
    assert sum(differs) >= least
    scn = out['scn']
    assert scn.n_agent > 128 and nw.reachable_prefix(scn) == 2 * scn.n_stream > 256
    if name == 'isolated_300':                  # np.sum's left half (144 elements) splits again; 254 streams at most: 50 junctions are dead
        assert scn.n_agent // 2 - (scn.n_agent // 2) % 8 > 128 and 240 <= scn.n_stream <= 254
    else:
        assert scn.n_stream == scn.n_agent


def test_few_threads_has_more_streams_and_agents_than_threads():
    net = nw.NETWORKS['few_threads']
    scn = net.scenario()
    double = [0]
    eight = {int(l) for l in np.flatnonzero(np.bincount(scn.stream_entry_lane, minlength=scn.n_lane) == 8)}
    last = {}

    def on_second(e, ms):
        for l in eight:
            n = ms.lane_vehicles(l)['n']
            double[0] += n - last.get((e, l), 0) >= 2           # two of the lane's streams inserted in the same second
            last[(e, l)] = n
    # the agents past the first 64 (the prologue's stride loop sets their link states and prev_action) signal live lanes: they switch
    # phase during the run, and vehicles stand in front of their red signal
    far = [a for a in range(64, scn.n_agent) if (scn.agent_lanes[a, :scn.agent_nlane[a]] < nw.reachable_prefix(scn)).all()]
    switches, held, prev = [0], [0], {}

    def on_step(t, res, orc):
        for e, o in enumerate(orc):
            for a in far:
                switches[0] += prev.get((e, a), 0) != o.prev_action[a]
                prev[(e, a)] = o.prev_action[a]
                held[0] += o.prev_action[a] == 1 and o.ms.lane_stats(int(scn.agent_lanes[a, 0]))[1] > 0
    out = _run('few_threads', on_second=on_second, on_step=on_step)
    _common(out)
    print('few_threads: %d agents >= 64 on live lanes, %d phase switches, %d (agent, step) pairs with a queue at red' % (len(far), switches[0], held[0]))
    assert len(far) == 30 and min(far) >= 64 and switches[0] >= 100 and held[0] >= 100
    assert int(np.asarray(scn.stream_entry_lane)[64:].max()) < 64 and scn.n_stream - 64 >= 20       # streams past the first 64 enter live lanes
    assert nw.reachable_prefix(scn) <= 64 and scn.n_stream > 64 and scn.n_agent > 64 and len(eight) >= 1
    assert net.env == {'TSC_ENV_HELP': '0'} and net.plan[5] == 64
    # more than 64 streams emit, and what they emitted entered the network: departed + pending = emitted, per instance
    T = net.steps * scn.control_interval_sec
    fl = np.asarray(scn.flows, np.int64)
    emitted = np.zeros(scn.n_stream, np.int64)
    for b, en, vph, s_ in fl.tolist():
        tau = max(0, min(T, en) - b)
        emitted[s_] += (tau * vph + 3599) // 3600
    assert (emitted > 0).sum() > 64
    for o in out['orc']:
        tot = o.ms.totals()
        assert tot['departed'] + tot['pending'] == emitted.sum() and tot['departed'] > 0.9 * emitted.sum(), tot
    assert double[0] >= 10, double
    dead = [a for a in range(scn.n_agent) if (scn.agent_lanes[a, :scn.agent_nlane[a]] >= nw.reachable_prefix(scn)).all()]
    assert dead == list(range(70))              # the junctions without demand: dead lanes, observations and rewards of zero


@pytest.mark.parametrize('name', ['merge4_zipper', 'merge4_yield'])
def test_merge4_feeders_compete(name):
    """In at least 10 seconds (per instance) all four feeders hold a head that wants to cross: within reach of its stop line by the
    zipper's own test, on a lane whose movement leads into the merged lane."""
    scn = nw.NETWORKS[name].scenario()
    merged = int(np.flatnonzero((scn.lane_up >= 0).sum(axis=1) == 4)[0])
    feeders = [int(u) for u in scn.lane_up[merged]]
    compete = {}

    def on_second(e, ms):
        ready = 0
        for f in feeders:
            d = ms.lane_vehicles(f)
            ready += d['n'] > 0 and float(scn.lane_len[f]) - float(d['x'][0]) < float(d['v'][0]) + ACC
        compete[e] = compete.get(e, 0) + (ready == 4)
    out = _run(name, on_second=on_second)
    _common(out)
    print('%s: seconds with four ready heads per instance: %s' % (name, compete))
    assert min(compete.values()) >= 10
    if name == 'merge4_zipper':
        assert sorted(int(z) for z in scn.mv_zip[feeders].max(axis=1)) == [r | 4 << 8 for r in range(4)]
        assert (scn.mv_yield < 0).all() and not scn.mv_prio.any()
    else:
        assert not scn.mv_zip.any() and int(scn.mv_prio.sum()) == 1 and sorted(set(scn.mv_yield.ravel().tolist())) == [-1, feeders[0]]
        assert int((scn.mv_yield >= 0).sum()) == 3


def test_link62_uses_the_last_link_of_the_movement_word():
    out = _run('link62')
    _common(out)
    scn = out['scn']
    assert int(scn.mv_link.max()) == 62 and scn.green_tab.shape[1:] == (8, 63) and scn.n_a_ls == [8]
    tot = [o.ms.totals() for o in out['orc']]
    assert min(t['arrived'] for t in tot) > 50


@pytest.mark.parametrize('name,ctrl,yellow', [('ctrl8', 8, 3), ('ctrl1', 1, 0)])
def test_control_intervals(name, ctrl, yellow):
    out = _run(name)
    _common(out)
    scn = out['scn']
    assert (scn.control_interval_sec, scn.yellow_interval_sec) == (ctrl, yellow)
    if ctrl == 8:
        assert scn.episode_length_sec % 8 != 0 and out['done'] == [scn.episode_length_sec // 8] * out['net'].E
    assert int((scn.mv_yield >= 0).sum()) >= 3 and scn.agent == 'ma2c'


def test_burst_backs_up_and_teleports():
    pend = []

    def on_second(e, ms):
        pend.append(ms.totals()['pending'] > 0)
    out = _run('burst', on_second=on_second)
    _common(out)
    scn = out['scn']
    assert scn.peak_emission()[0] >= 3 and int(scn.flows[:, 2].max()) >= 7200 and scn.teleport_sec == 20
    tele = [o.ms.totals()['teleported'] for o in out['orc']]
    print('burst: pending > 0 in %.0f %% of the seconds, teleported %s' % (100.0 * np.mean(pend), tele))
    assert np.mean(pend) >= 0.25 and min(tele) > 0


def test_zip254_feeders_reach_lane_253():
    out = _run('zip254')
    _common(out)
    scn = out['scn']
    assert scn.n_lane == 254 and int(scn.lane_up.max()) == 253 and int((scn.mv_zip >> 8).max()) == 3
    merged = int(np.flatnonzero((scn.lane_up == 253).any(axis=1))[0])
    # the last feeder does send: vehicles of its route reach the merged lane's exit
    r253 = int(np.flatnonzero(scn.mv_next[253] == merged)[0])
    assert nw.reachable_prefix(scn) == 254
    arrived = [o.ms.totals()['arrived'] for o in out['orc']]
    assert min(arrived) > 500 and r253 in (0, 1, 2)


def test_limits_agree_between_check_limits_and_the_registry():
    """Scenario.check_limits refuses, with the remedy, what tsc_env_create refuses (tests/test_networks_gpu.py asks the library for the
    same scenarios): past 254 routes / streams, a ninth stream on a lane, link 63, a zipper rank past four bits, 256 lanes with a
    zipper, a 9 s control interval, 256 vehicles a second, and an empty scenario."""
    for what, (make, text, _) in nw.REFUSED.items():
        if text is None:
            make().streams_ready().check_limits()              # (the LDS need is the library's to tell)
            continue
        with pytest.raises(ValueError, match=text):
            make().streams_ready().check_limits()


def test_windows_emits_what_the_integer_rule_says():
    """The create-time emission table over windows that begin and end inside a 4-second word, overlap, are empty or lie past the
    table: per instance, departed + pending is the integer rule's count over the run's seconds, stream by stream."""
    out = _run('windows')
    _common(out)
    scn, net = out['scn'], out['net']
    T = net.steps * scn.control_interval_sec
    assert (scn.control_interval_sec, scn.yellow_interval_sec) == (1, 0) and T == scn.episode_length_sec
    emitted = np.zeros(scn.n_stream, np.int64)
    for b, en, vph, s_ in np.asarray(scn.flows, np.int64).tolist():
        emitted[s_] += (max(0, min(T, en) - b) * vph + 3599) // 3600
    assert (emitted > 0).all() and {int(b) % 4 for b in scn.flows[:, 0]} >= {1, 2, 3} and {int(x) % 4 for x in scn.flows[:, 1]} >= {1, 2, 3}
    for o in out['orc']:
        tot = o.ms.totals()
        assert tot['departed'] + tot['pending'] == emitted.sum() and tot['departed'] > 0.8 * emitted.sum(), (tot, emitted)
