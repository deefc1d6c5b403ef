"""The flat phase of step_kernel (csrc/tsc_env.hip) at the boundaries of its super-rounds, on a synthetic network that fills up
within a minute: 63 junctions with three 200 m entry lanes each (189 streams at 2700 - 3600 veh/h), signals mostly red.  The queued
vehicles of an instance grow by ~120 a second to ~5000, so one run passes every boundary of every workgroup size: a super-round holds
kF x T vehicles (T threads, kF per thread), and the seconds of interest are those with at most (kF - 1) x T queued vehicles, with
more than that but at most kF x T (the last slot of the threads is in use), and with more than kF x T (a second super-round: the LDS
carry of the chain scan and the saved old state of the previous round's last vehicle).

The cases are the 2-wide flat phase at 256 threads (TSC_ENV_KF=2) and the wide runtime-dimension kernel (4-wide) at 512 and 1024.
A 3-wide flat phase (768 vehicles per super-round at 256 threads) was built with this file and measured slower than the 2-wide one
(profiles/env_scalar_bench.json), so no kernel of that width exists and TSC_ENV_KF=3 is no value of the knob.

Nothing here has a tolerance: observations, rewards and the vehicle state are the oracle's bit for bit.  The oracle walk is computed
once and shared; test_the_run_reaches_every_boundary states on the oracle alone (no GPU) that the run contains what the cases are for."""
import functools

import numpy as np
import pytest

from tests import env_harness as H
from tests import networks as nw

E, STEPS, SEED = 3, 13, 40
# (TSC_ENV_THREADS, TSC_ENV_KF or None, the row and threads step_plan() reports)
CASES = [('256', '2', (256, 1, 0, 2, 0, 256)), ('512', None, (1024, 1, 0, 4, 0, 512)), ('1024', None, (1024, 1, 0, 4, 0, 1024))]


@functools.lru_cache(maxsize=None)
def scenario():
    J, episode = 63, 100
    lanes, routes, streams, flows = [], [[], [], []], [], []
    for j in range(J):
        lanes += [(200.0, 13.89, j)] * 3 + [(100.0, 13.89, -1)]
        for k in range(3):
            routes[k].append([(4 * j + k, k), (4 * j + 3, -1)])
            flows.append((0, episode, 3600 - 300 * ((j + k) % 4), len(streams)))
            streams.append((4 * j + k, k))
    return nw.compile_network('fill_63', 'ia2c', lanes, routes, [['GGG', 'rrr', 'Grr', 'rGr']] * J,
                              [[(j - 1) % J, (j + 1) % J] for j in range(J)], flows, streams, episode_length_sec=episode, teleport_sec=300)


@functools.lru_cache(maxsize=None)
def oracle_walk():
    """-> (per control step (actions, results of OracleEnv.step per instance, vehicle state per instance at the steps of STATE_AT),
    per instance and simulated second the lanes' vehicle counts at the START of the second)."""
    from oracle.env_oracle import OracleEnv
    scn = scenario()
    orc = [OracleEnv(scn, seed=SEED + e) for e in range(E)]
    counts = [[] for _ in range(E)]
    for e, o in enumerate(orc):
        def stepper(n=1, _ms=o.ms, _step=o.ms.step, _c=counts[e]):
            for _ in range(n):
                _c.append(np.asarray(_ms.snapshot()['n']).copy())
                _step(1)
        o.ms.step = stepper
    obs = [o.reset() for o in orc]
    for c in counts:
        del c[:]                                    # (seconds of the reset, if any, are no seconds of the run)
    rng = np.random.RandomState(SEED)

    def draw(t, obs):                               # red (phase 1) with a few random phases: some platoons cross every step
        return np.where(rng.rand(E, scn.n_agent) < 0.15, rng.randint(0, 4, (E, scn.n_agent)), 1).astype(np.int32), None
    steps = []
    for t, acts, _, res, _ in H.oracle_steps(scn, orc, obs, STEPS, draw):
        steps.append((acts.copy(), list(res), [o.ms.snapshot() for o in orc] if t in STATE_AT else None))
    return steps, counts


STATE_AT = (1, 4, 8, STEPS - 1)


def boundaries(counts, T, kf, nla):
    """Which of the four conditions the seconds of `counts` (lane counts at the start of a second) meet for T threads, kf per thread."""
    got = set()
    for n in counts:
        c = np.maximum(n[:nla] - 1, 0)              # queued vehicles per lane: all but the head, in the kernel's flat order
        q, first = int(c.sum()), np.cumsum(c) - c
        got.add('low' if q <= (kf - 1) * T else 'last_slot' if q <= kf * T else 'two_rounds')
        # a lane whose queue lies in two wavefronts of one super-round: its first and last flat index in different blocks of 64 x kf
        rnd, wav = first // (kf * T), first // (64 * kf)
        last = first + c - 1
        if np.any((c > 0) & (last // (kf * T) == rnd) & (last // (64 * kf) != wav)):
            got.add('straddle')
    return got


@pytest.mark.parametrize('threads,kf,plan', CASES)
def test_the_run_reaches_every_boundary(threads, kf, plan):
    scn = scenario()
    _, counts = oracle_walk()
    nla = scn.n_lane                                # (the scenario's lanes are in the device's order; the kernel pads with empty ones)
    assert scn.n_lane <= 256 and len(counts[0]) == STEPS * scn.control_interval_sec
    got = boundaries([n for c in counts for n in c], plan[5], plan[3], nla)
    assert got == {'low', 'last_slot', 'two_rounds', 'straddle'}, got


@pytest.mark.gpu
@pytest.mark.parametrize('threads,kf,plan', CASES)
def test_flat_phase_at_super_round_boundaries_vs_oracle(threads, kf, plan, monkeypatch):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    for k in ('TSC_ENV_THREADS', 'TSC_ENV_KF', 'TSC_ENV_HELP', 'TSC_ENV_SPEC'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('TSC_ENV_THREADS', threads)
    if kf:
        monkeypatch.setenv('TSC_ENV_KF', kf)
    scn = scenario()
    steps, _ = oracle_walk()
    env = VecTrafficEnv(scn, E, seed=SEED)
    try:
        env.reset()
        got = env.step_plan()
        assert got['row'] + (got['threads'],) == plan, got
        for t, (acts, res, snaps) in enumerate(steps):
            out = [x.cpu().numpy() for x in env.step(H.upload(env, acts))]
            H.assert_step_equal(scn, t, out, res)
            if snaps is not None:
                for e in range(E):
                    st = env.get_state(e)
                    for k in H.STATE_KEYS:
                        np.testing.assert_array_equal(st[k], snaps[e][k], err_msg='state %s t=%d e=%d' % (k, t, e))
    finally:
        env.close()
