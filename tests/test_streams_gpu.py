"""The insertion code of step_kernel (csrc/tsc_env.hip: the block after `for (int q = 0; q < kMaxEntry; ++q)`) against the CPU oracle:
the three route modes of a stream (fixed, a draw per vehicle from cumulative weights that change in time, a route per instance and
episode from the host) and its insertion window, on the stream networks of tests/networks.py (forks, ratios_in_time, sinks_ragged /
sinks_even, windows_on_lane) and on the generated networks with redrawn stream tables (random_stream_network over
RANDOM_STREAM_SEEDS), under the library's own plan and under the kernel variants of tests/test_networks_random_gpu.py; identities
between two device handles that need no oracle; and tsc_env_set_stream_routes' contract (staged until the next reset, candidates
only).  tests/test_streams_host.py states, on the oracle alone, which edge of the insertion code each of these runs reaches.  The
trace and the lane data of windows_on_lane and ratios_in_time are rows of networks.AUX['walk'] (tests/test_networks_aux_gpu.py).

Nothing here has a tolerance: the comparison is env_harness.compare_with_oracle / follow / lockstep, bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import env_harness as H
from tests import networks as nw
from tests.test_networks_random_gpu import VARIANTS

pytestmark = pytest.mark.gpu

HAND_MADE = nw.STREAM_NETWORKS + ['sinks_even']
CHUNK = 8
STREAM_CHUNKS = [nw.RANDOM_STREAM_SEEDS[i:i + CHUNK] for i in range(0, len(nw.RANDOM_STREAM_SEEDS), CHUNK)]
_ids = lambda chunk: 'seeds%d-%d' % (chunk[0], chunk[-1])


@pytest.fixture(autouse=True)
def _library_chooses_the_plan(monkeypatch):
    for k in ('TSC_ENV_THREADS', 'TSC_ENV_KF', 'TSC_ENV_HELP', 'TSC_ENV_SPEC'):
        monkeypatch.delenv(k, raising=False)


def _net(name):
    return nw.SINKS_EVEN if name == 'sinks_even' else nw.NETWORKS[name]


def _compare(net, monkeypatch, variant=None, label=None, sigma=0.5, scn=None, **kw):
    """compare_with_oracle over `net` under a kernel variant of VARIANTS (None: the library's own plan)."""
    scn = net.scenario() if scn is None else scn
    kw = dict(VARIANTS[variant] if variant else {}, label=label, **kw)
    if variant == 'krauss':
        scn = copy.copy(scn)
        scn.car_following, scn.krauss_sigma = 'krauss', sigma
        with H.oracle_krauss(sigma):
            return H.compare_with_oracle(scn, net, monkeypatch, **kw)
    return H.compare_with_oracle(scn, net, monkeypatch, **kw)


# ---- the hand-made networks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', HAND_MADE)
def test_stream_network_vs_oracle_under_its_recorded_plan(name, monkeypatch):
    """Observations, rewards and done at every step, the vehicle state at the peak and at the end, the counters."""
    net = _net(name)
    tot = _compare(net, monkeypatch, plan=net.plan, label=name)
    assert min(x['arrived'] for x in tot) > 20


@pytest.mark.parametrize('name', ['windows_on_lane', 'forks'])
def test_backlog_and_serial_of_every_stream(name):
    """pending and serial of get_state, stream by stream, against the oracle's at the end of the run: on windows_on_lane the
    stream whose window is too narrow has inserted nothing and holds every vehicle it emitted."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    net = _net(name)
    scn = net.scenario()
    env = VecTrafficEnv(scn, net.E, seed=net.seed)
    try:
        side = H.run_oracle(scn, net)
        next(side)
        env.reset()
        orc = H.follow(env, side, state_at=[net.steps - 1], counters=True)
        for e, o in enumerate(orc):
            pend, ser = o.ms.stream_state()
            st = env.get_state(e)
            np.testing.assert_array_equal(st['pending'], pend, err_msg='pending e=%d' % e)
            np.testing.assert_array_equal(st['serial'], ser, err_msg='serial e=%d' % e)
            if name == 'windows_on_lane':
                assert ser[3] == 0 and pend[3] >= 30 and ser[2] >= 3
    finally:
        env.close()


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', ['forks', 'ratios_in_time'])
def test_stream_network_under_kernel_variants(name, variant, monkeypatch):
    """forks and ratios_in_time at 512 and 1024 threads, without the helper wavefronts, with the 2- and 4-wide flat phase, in test
    mode, under Krauss (sigma 0.5) and with recording on: there the trip log is compared too, whose {route, serial} rows two
    streams of forks can share."""
    net = _net(name)
    kw = dict(least_trips=50) if variant == 'record' else {}
    tot = _compare(net, monkeypatch, variant, label='%s (%s)' % (name, variant), lds_limit=160 * 1024, **kw)
    assert min(x['arrived'] for x in tot) > 20


def test_ratios_in_time_with_a_demand_column_per_instance():
    """tsc_env_set_demand on ratios_in_time: flows[f][3] is a stream there, and no stream's index is a route it takes."""
    scn = nw.NETWORKS['ratios_in_time'].scenario()
    vph = nw.ratios_columns(scn)
    assert not any(s in {int(r) for r in scn.stream_choice[s, :, :, 0].ravel() if r >= 0} for s in range(scn.n_stream))
    env, _ = H.demand_parity(scn, len(vph), 60, 620, vph, rng_seed=14)
    env.close()


# ---- the generated networks -------------------------------------------------------------------------------------------------------
def _compare_generated(seed, monkeypatch, variant=None):
    net = nw.random_stream_network(seed)
    label = 'stream seed %d%s' % (seed, ' (%s)' % variant if variant else '')
    kw = dict(least_trips=1) if variant == 'record' else {}     # (tests/test_streams_host.py: vehicles arrive in every one of these runs)
    return _compare(net, monkeypatch, variant, label=label, sigma=net.sigma, lds_limit=160 * 1024, **kw)


@pytest.mark.parametrize('chunk', STREAM_CHUNKS, ids=_ids)
def test_generated_stream_networks_vs_oracle_with_the_librarys_own_plan(chunk, monkeypatch):
    for seed in chunk:
        _compare_generated(seed, monkeypatch)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_generated_stream_networks_under_kernel_variants(variant, monkeypatch):
    """The first eight of RANDOM_STREAM_SEEDS under every variant (Krauss: the network's own sigma)."""
    for seed in STREAM_CHUNKS[0]:
        _compare_generated(seed, monkeypatch, variant)


# ---- identities between two handles ---------------------------------------------------------------------------------------------------
def _tables(scn, **fields):
    """A copy of scn with the given stream tables in place of its own: the lanes keep their order."""
    out = copy.copy(scn)
    for k, v in fields.items():
        assert k.startswith('stream_')
        setattr(out, k, v)
    return out


def _handles(scns, E, seed):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    return [VecTrafficEnv(s, E, seed=seed) for s in scns]


def _same_episode(scns, E=3, seed=700, steps=60):
    """Handles of the scenarios scns under the same seeds and actions: bit-equal reset observations, step results and state."""
    envs = _handles(scns, E, seed)
    try:
        obs = [env.reset().cpu().numpy().copy() for env in envs]
        for o in obs[1:]:
            np.testing.assert_array_equal(obs[0], o)
        rng = np.random.RandomState(seed)
        out = H.lockstep(envs, steps, lambda t: (H.uniform_actions(scns[0], rng, E), None), state_of=range(E))
        assert all(bool(d) for d in out[-1][2])                     # to the end of the episode
        for e in range(E):
            a, b = envs[0].get_state(e), envs[1].get_state(e)
            for k in ('pending', 'serial'):
                np.testing.assert_array_equal(a[k], b[k], err_msg='%s e=%d' % (k, e))
            assert int(a['serial'].sum()) > 100
    finally:
        for env in envs:
            env.close()


def test_a_single_choice_at_65536_is_a_fixed_route():
    """(a) mode 1 with the one choice {r, 65536} = mode 0 with route r."""
    base = nw.SINKS_EVEN.scenario()
    route = np.array([0, 2, 5, 3, 7, 6, 4], np.int32)           # a route that begins on each stream's lane
    assert all(base.mv_next[base.stream_entry_lane[s], r] >= 0 for s, r in enumerate(route))
    choice = np.stack([route, np.full(7, 65536, np.int32)], 1).reshape(7, 1, 1, 2)
    _same_episode([_tables(base, stream_mode=np.ones(7, np.int32), stream_choice=choice),
                   _tables(base, stream_mode=np.zeros(7, np.int32), stream_choice=choice)])


def test_four_identical_tables_are_one_table():
    """(c) n_interval = 4 with the same table four times = n_interval = 1."""
    base = nw.NETWORKS['ratios_in_time'].scenario()
    one = base.stream_choice[:, 3:4].copy()
    _same_episode([_tables(base, stream_choice=np.ascontiguousarray(np.repeat(one, 4, axis=1))), _tables(base, stream_choice=one)])


def test_the_whole_lane_given_as_a_window_is_no_window():
    """(d) origin 0 and limit = the lane's length, written out, = no window tables at all."""
    base = nw.NETWORKS['sinks_ragged'].scenario()
    assert (base.stream_origin == 0).all() and (base.stream_limit == base.lane_len[base.stream_entry_lane]).all()
    _same_episode([_tables(base, stream_origin=base.stream_origin.copy(), stream_limit=base.stream_limit.copy()),
                   _tables(base, stream_origin=None, stream_limit=None)])


def test_one_window_among_whole_lanes_vs_oracle(monkeypatch):
    """(d) one stream with an origin of 33.3 m and the others on the whole lane: the window table is on the device, and its rows
    of the whole-lane streams change nothing -- against the oracle."""
    base = nw.SINKS_EVEN.scenario()
    origin = base.stream_origin.copy()
    origin[3] = 33.3
    tot = _compare(nw.SINKS_EVEN, monkeypatch, scn=_tables(base, stream_origin=origin), label='one window')
    assert min(x['arrived'] for x in tot) > 20


def test_a_route_from_the_host_is_a_fixed_route_per_instance():
    """(b) a mode-2 stream given r through tsc_env_set_stream_routes = the mode-0 stream with route r, instance by instance, with
    another r in every instance: instance e of the mode-2 handle against instance e of a mode-0 handle with the routes of e."""
    from deeprl_signal_control_amd.scenario import draw_stream_routes
    base, E, seed = nw.NETWORKS['sinks_ragged'].scenario(), 3, nw.NETWORKS['sinks_ragged'].seed
    routes = [draw_stream_routes(base, seed + e) for e in range(E)]
    assert len({tuple(r.tolist()) for r in routes}) == E
    fixed = []
    for r in routes:
        choice = base.stream_choice.copy()
        choice[:, 0, 0, 0] = r
        fixed.append(_tables(base, stream_mode=np.where(base.stream_mode == 2, 0, base.stream_mode).astype(np.int32), stream_choice=choice))
    envs = _handles([base] + fixed, E, seed)
    try:
        obs = [env.reset().cpu().numpy() for env in envs]
        for e in range(E):
            np.testing.assert_array_equal(obs[0][e], obs[1 + e][e])
        rng = np.random.RandomState(seed)
        for t in range(60):
            acts = H.upload(envs[0], H.uniform_actions(base, rng, E))
            outs = [[x.cpu().numpy().copy() for x in env.step(acts)] for env in envs]
            for e in range(E):
                for name, x, y in zip(('obs', 'reward', 'done', 'global_reward'), outs[0], outs[1 + e]):
                    np.testing.assert_array_equal(x[e], y[e], err_msg='%s t=%d e=%d' % (name, t, e))
        for e in range(E):
            H.assert_state_equal(envs[0], envs[1 + e], [e], 59)
            assert int(envs[0].get_state(e)['serial'].sum()) > 100
    finally:
        for env in envs:
            env.close()


# ---- tsc_env_set_stream_routes ----------------------------------------------------------------------------------------------------
def _set_routes(env, routes):
    """tsc_env_set_stream_routes with int32 [E, NS] -> (rc, tsc_last_error)."""
    routes = np.ascontiguousarray(routes, np.int32)
    assert routes.shape == (env.E, env.scn.n_stream)
    rc = env._L.tsc_env_set_stream_routes(env._h, routes.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, env._L.tsc_last_error().decode() if rc else ''


def _other_routes(scn, routes):
    """Per instance another candidate for every mode-2 stream that has one."""
    out = np.array(routes, np.int32)
    for e in range(len(out)):
        for s in np.flatnonzero(scn.stream_mode == 2):
            cand = [int(r) for r in scn.stream_choice[s, 0, :, 0] if r >= 0 and r != out[e, s]]
            if cand:
                out[e, s] = cand[(e + int(s)) % len(cand)]
    return out


def _second_episode_vs_oracle(env, scn, routes, seed, monkeypatch, steps=60):
    """The handle's next episode, reset without a draw of its own, against oracles that are given `routes` [E, NS]."""
    import oracle.env_oracle as eo
    E = env.E
    by_seed = {seed + e: routes[e] for e in range(E)}
    monkeypatch.setattr(eo, 'episode_stream_routes', lambda s, sd: np.asarray(by_seed[sd], np.int32))
    monkeypatch.setattr(env, '_draws_routes', False)            # reset() stages nothing: the routes already staged take effect
    orc = [eo.OracleEnv(scn, seed=seed + e) for e in range(E)]
    dev_obs = env.reset().cpu().numpy()
    obs = [o.reset() for o in orc]
    for e in range(E):
        for a in range(scn.n_agent):
            np.testing.assert_array_equal(dev_obs[e, a, :len(obs[e][a])], obs[e][a].astype(np.float32))
    rng = np.random.RandomState(seed)
    H.follow(env, H.oracle_steps(scn, orc, obs, steps, lambda t, obs: (H.uniform_actions(scn, rng, E), None)), state_at=[20, steps - 1],
             counters=True)
    for e, o in enumerate(orc):                 # every stream inserted what the oracle's stream inserted
        np.testing.assert_array_equal(env.get_state(e)['serial'], o.ms.stream_state()[1])


def test_routes_set_during_an_episode_wait_for_the_next_reset(monkeypatch):
    """A call after the reset and 10 steps leaves the running episode bit-equal to a handle nobody touched, to its end; the next
    reset runs the new routes, as the oracle does when it is given them."""
    net = nw.NETWORKS['sinks_ragged']
    scn, E, seed = net.scenario(), 3, net.seed
    envs = _handles([scn, scn], E, seed)
    try:
        for env in envs:
            env.reset()
        from oracle.env_oracle import episode_stream_routes
        drawn = np.stack([episode_stream_routes(scn, seed + e) for e in range(E)])
        new = _other_routes(scn, drawn)
        assert (new != drawn).any(axis=1).all()
        rng = np.random.RandomState(seed)

        def before(t):
            if t == 10:
                assert _set_routes(envs[0], new) == (0, '')
        out = H.lockstep(envs, 60, lambda t: (H.uniform_actions(scn, rng, E), None), state_of=range(E), before=before)
        assert all(bool(d) for d in out[-1][2])
        _second_episode_vs_oracle(envs[0], scn, new, seed + E, monkeypatch)
    finally:
        for env in envs:
            env.close()


def test_routes_that_are_no_candidates_are_refused_and_change_nothing(monkeypatch):
    """A route that is not among the stream's candidates and a route outside the table both return non-zero, tsc_last_error names
    instance, stream and route, and the following episode runs the routes the handle had -- also those of instance 0, which the
    refused arrays changed to other candidates."""
    from oracle.env_oracle import episode_stream_routes
    net = nw.NETWORKS['sinks_ragged']
    scn, E, seed = net.scenario(), 3, net.seed
    env = _handles([scn], E, seed)[0]
    try:
        env.reset()
        drawn = np.stack([episode_stream_routes(scn, seed + e) for e in range(E)])
        s1 = int(np.flatnonzero((scn.stream_mode == 2) & ((scn.stream_choice[:, 0, :, 0] >= 0).sum(axis=1) == 1))[0])       # one candidate
        only = int(scn.stream_choice[s1, 0, 0, 0])
        stranger = next(r for r in range(scn.n_route) if r != only and scn.mv_next[scn.stream_entry_lane[s1], r] >= 0)
        for e_bad, route, words in ((1, stranger, 'instance 1 stream %d: route %d is not one of' % (s1, stranger)),
                                    (2, scn.n_route, 'instance 2 stream %d: route %d of %d' % (s1, scn.n_route, scn.n_route)),
                                    (1, -1, 'instance 1 stream %d: route -1 of %d' % (s1, scn.n_route))):
            bad = _other_routes(scn, drawn)
            assert (bad[0] != drawn[0]).any()
            bad[e_bad, s1] = route
            rc, text = _set_routes(env, bad)
            assert rc != 0 and words in text, (rc, text)
        rng = np.random.RandomState(1)
        for t in range(5):                      # the running episode goes on
            env.step(H.upload(env, H.uniform_actions(scn, rng, E)))
        _second_episode_vs_oracle(env, scn, drawn, seed + E, monkeypatch)
    finally:
        env.close()
