"""Krauss car following on the device (tsc_env_set_car_following, step_kernel's Krauss instantiations) against the CPU oracle's
Krauss path (ms_set_krauss, MICROSIM_SPEC.md "Krauss car following"): obs, rewards, done and the full vehicle state bit-exact, for
every kernel path a Krauss handle can take -- the flat phase at every workgroup size and flat-phase width, the plain walk, the
recording walk -- and for the scenarios whose vehicles key the dawdling differently (stream != route, drawn routes, merges).
The oracle's switch is process-wide: every test turns it off again in a `finally`."""
import json
import os

import numpy as np
import pytest
import torch

from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net, build_small_grid
from tests import env_harness as H
from tests.env_harness import oracle_krauss
from tests.env_rules import assert_trips_equal, device_trips

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_vs_oracle(scn, E, steps, sigma, seed, sample=None, p_change=0.5, rng_seed=0):
    """E device instances (seeds seed + e) against oracle instances of the sampled ones; random phase changes and fingerprints."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from oracle.env_oracle import OracleEnv
    sample = list(range(E)) if sample is None else list(sample)
    with oracle_krauss(sigma):
        env = VecTrafficEnv(scn, E, seed=seed)
        orc = {e: OracleEnv(scn, seed=seed + e) for e in sample}
        env.reset()
        obs = {e: o.reset() for e, o in orc.items()}
        assert env.car_following() == ('krauss', pytest.approx(sigma))
        rng = np.random.RandomState(rng_seed)
        act = np.zeros((E, scn.n_agent), np.int32)

        def draw(t, obs):
            pol = H.agent_policies(scn, rng, E)
            H.change_actions(scn, rng, act, p_change)
            return act, pol
        H.follow(env, H.oracle_steps(scn, orc, obs, steps, draw), state_at=[steps - 1])
        live = env.mean_live_vehicles()
        env.close()
    return live


@pytest.mark.parametrize('E,steps,sigma,threads,kf', [(48, 150, 0.5, '256', ''), (48, 150, 0.5, '256', '2'), (48, 150, 0.5, '256', '4'),
                                                      (48, 150, 0.5, '512', ''), (48, 150, 0.5, '1024', ''),
                                                      (8, 720, 0.5, '', ''), (48, 150, 0.0, '256', '')])
def test_large_grid_krauss_vs_oracle(E, steps, sigma, threads, kf, monkeypatch):
    """large_grid MA2C under Krauss: every workgroup size / flat-phase width (TSC_ENV_THREADS / TSC_ENV_KF), a whole episode, and
    sigma = 0 (plain Krauss following, no hash)."""
    if threads:
        monkeypatch.setenv('TSC_ENV_THREADS', threads)
    if kf:
        monkeypatch.setenv('TSC_ENV_KF', kf)
    scn = build_large_grid('ma2c', car_following='krauss', krauss_sigma=sigma)
    assert _run_vs_oracle(scn, E, steps, sigma, seed=100, rng_seed=E) > 50


def test_large_grid_krauss_at_the_benchmarked_instance_count():
    """E = 1024 under the handle's own workgroup choice; 16 sampled instances (they are independent) against the oracle."""
    scn = build_large_grid('ma2c', car_following='krauss', krauss_sigma=0.5)
    sample = np.random.RandomState(5).choice(1024, 16, replace=False)
    assert _run_vs_oracle(scn, 1024, 300, 0.5, seed=7, sample=sorted(int(e) for e in sample), rng_seed=1) > 100


@pytest.mark.parametrize('name', ['large_grid_init', 'small_grid', 'real_net'])
def test_routes_that_key_the_dawdling_differently(name):
    """large_grid with init_density > 0 (insertion stream != route), small_grid (routes drawn per vehicle), Monaco (contracted
    chains, zipper merges): the hash is keyed by the vehicle's own route and its serial within its stream."""
    if name == 'large_grid_init':
        scn = build_large_grid('ma2c', init_density=0.3, car_following='krauss')
    elif name == 'small_grid':
        scn = build_small_grid('ma2c', car_following='krauss')
    else:
        scn = build_real_net('ma2c', car_following='krauss')
    _run_vs_oracle(scn, 4, 240, 0.5, seed=60, p_change=0.25, rng_seed=2)


def test_krauss_flat_phase_equals_plain_walk(monkeypatch):
    """step_kernel's Krauss flat phase (helper threads) against its Krauss plain walk at a congested load: bit-identical."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = build_large_grid('ma2c', car_following='krauss', krauss_sigma=0.5)
    E = 96
    monkeypatch.setenv('TSC_ENV_HELP', '1')
    a = VecTrafficEnv(scn, E, seed=7)
    monkeypatch.setenv('TSC_ENV_HELP', '0')
    b = VecTrafficEnv(scn, E, seed=7)
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    g = torch.Generator(device='cuda'); g.manual_seed(3)
    H.lockstep([a, b], 400, lambda t: (torch.randint(0, 5, (E, 25), generator=g, device='cuda', dtype=torch.int32),
                                       torch.rand(E, 25, 5, generator=g, device='cuda')), state_of=(0, 17, 95))
    assert a.mean_live_vehicles() > 400
    a.close(); b.close()


def test_recording_under_krauss_trip_table():
    """The recording walk under Krauss: the trip rows (route, serial, depart, arrival, waiting seconds, waiting count) equal the
    oracle's -- the serial each vehicle carries is checked directly -- and so do obs and rewards along the way."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from oracle.env_oracle import OracleEnv
    scn = build_large_grid('greedy', car_following='krauss', krauss_sigma=0.5)
    E = 3
    with oracle_krauss(0.5):
        env = VecTrafficEnv(scn, E, seed=20)
        env.set_record(True)
        orc = [OracleEnv(scn, seed=20 + e, is_record=True) for e in range(E)]
        env.reset()
        obs = [o.reset() for o in orc]
        rng = np.random.RandomState(9)
        H.follow(env, H.oracle_steps(scn, orc, obs, 360, lambda t, obs: (rng.randint(0, 5, (E, 25)).astype(np.int32), None)))
        for e in range(E):
            dev = device_trips(env, e)
            ref = np.array(orc[e].ms.trips(), np.int32).reshape(-1, 6)
            assert len(dev) == len(ref) > 500
            assert_trips_equal(dev, ref, 'trips e=%d' % e)
            assert len({(int(r_), int(s_)) for r_, s_ in dev[:, :2]}) == len(dev)        # (route, serial) names a vehicle once
        env.close()


def test_explicit_idm_is_the_default():
    """car_following = idm in the config (and an explicit TSC_CF_IDM call) runs exactly what a handle without the key runs."""
    from deeprl_signal_control_amd.env import VecTrafficEnv, scenario_from_config
    cfg = dict(scenario='large_grid', agent='ma2c', seed='12', test_seeds='10000', car_following='idm')
    scn_i = scenario_from_config(cfg)[0]
    scn_d = build_large_grid('ma2c')
    E = 32
    a, b = VecTrafficEnv(scn_d, E, seed=5), VecTrafficEnv(scn_i, E, seed=5)
    b._L.tsc_env_set_car_following(b._h, 1, 0.5)          # Krauss requested, then IDM again before the reset: IDM holds
    assert b._L.tsc_env_set_car_following(b._h, 0, 0.0) == 0
    assert b._L.tsc_env_set_car_following(b._h, 2, 0.0) != 0 and b._L.tsc_env_set_car_following(b._h, 1, 1.5) != 0
    assert torch.equal(a.reset(), b.reset())
    assert a.car_following() == b.car_following() == ('idm', 0.0)
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    H.lockstep([a, b], 200, lambda t: (torch.randint(0, 5, (E, 25), generator=g, device='cuda', dtype=torch.int32), None), state_of=(0, 31))
    a.close(); b.close()


def test_greedy_episodes_reproduce_the_oracle_sweep():
    """Greedy large_grid episodes under Krauss sigma = 0.5 on the test seeds 10000 ... 40000, all four as one batch on the device:
    the mean step rewards and trip counts of profiles/r06_krauss_sweep.json (the oracle's, tools/sweep_krauss.py)."""
    from deeprl_signal_control_amd.env import VecTrafficEnv
    ref = json.load(open(os.path.join(ROOT, 'profiles', 'r06_krauss_sweep.json')))['results']['large_grid | Krauss sigma 0.5 (SUMO default)']
    seeds = (10000, 20000, 30000, 40000)
    scn = build_large_grid('greedy', norm_wave=1.0, norm_wait=1.0, clip_wave=-1.0, clip_wait=-1.0, car_following='krauss', krauss_sigma=0.5)
    env = VecTrafficEnv(scn, 4, seed=0, test_seeds=seeds)
    env.train_mode = False
    env.reset(test_ind=np.arange(4))
    gs = []
    while True:
        _, _, d, g = env.step(env.greedy_actions())
        gs.append(g.cpu().numpy().copy())
        if bool(d.cpu().numpy().all()):
            break
    rew = np.mean(np.array(gs), axis=0)
    arrived, teleported = env.counters()
    for e in range(4):
        assert rew[e] == pytest.approx(ref[e]['reward'], rel=1e-12, abs=1e-9), (seeds[e], rew[e], ref[e]['reward'])
        assert (int(arrived[e]), int(teleported[e])) == (ref[e]['arrived'], ref[e]['teleported'])
    env.close()
