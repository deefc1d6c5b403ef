"""step_kernel / reset_kernel and the controller kernels (csrc/tsc_env.hip) against the CPU oracle on the generated networks of
tests/networks.py (random_network over RANDOM_SEEDS): a seeded differential sweep over the interactions the hand-made networks keep
apart -- float32 corner cases of L - x, v^2 / 20, 3 s v + 10 m and x_tail - 7 on lengths float32 cannot hold, detectors on lanes
shorter than 50 m, vehicles that cross a whole lane in a second, hand-offs into lanes at the 24-vehicle cap under a yellow feeder,
merges of three and four feeders next to a teleporting head.  tests/test_networks_random_host.py states, on the oracle alone, how many
of the 96 runs reach each of these.

The comparison is env_harness.compare_with_oracle, the one of tests/test_networks_gpu.py: nothing here has a tolerance.  A failure
names the seed, the control step, the instance and the first field that differs.  The seed lists are fixed: no test draws seeds."""
import copy

import numpy as np
import pytest

from tests import env_harness as H
from tests import networks as nw
from tests.env_rules import hold_state, hold_update, loop_pressure

pytestmark = pytest.mark.gpu

CHUNK = 8
BASE_CHUNKS = [nw.RANDOM_SEEDS[i:i + CHUNK] for i in range(0, len(nw.RANDOM_SEEDS), CHUNK)]
VARIANT_CHUNKS = [nw.RANDOM_VARIANT_SEEDS[i:i + CHUNK] for i in range(0, len(nw.RANDOM_VARIANT_SEEDS), CHUNK)]
_ids = lambda chunk: 'seeds%d-%d' % (chunk[0], chunk[-1])

# kernel variant -> keywords of compare_with_oracle
VARIANTS = {
    'threads512': dict(env={'TSC_ENV_THREADS': '512'}),
    'threads1024': dict(env={'TSC_ENV_THREADS': '1024'}),
    'help0': dict(env={'TSC_ENV_HELP': '0'}),
    'kf2': dict(env={'TSC_ENV_KF': '2'}),
    'kf4': dict(env={'TSC_ENV_KF': '4'}),
    'test_mode': dict(train_mode=False),
    'krauss': dict(),
    'record': dict(record=True, least_trips=1),     # (tests/test_networks_random_host.py: vehicles arrive in every one of these runs)
}


def _compare(seed, monkeypatch, variant=None, network=nw.random_network):
    """One generated network (network(seed): random_network, or random_street_network for tests/test_streets_gpu.py) against the
    oracle under the library's own plan or a kernel variant."""
    net = network(seed)
    scn = net.scenario()
    label = 'seed %d%s' % (seed, ' (%s)' % variant if variant else '')
    kw = dict(VARIANTS[variant]) if variant else {}
    if variant == 'krauss':
        scn = copy.copy(scn)
        scn.car_following, scn.krauss_sigma = 'krauss', net.sigma
        with H.oracle_krauss(net.sigma):
            return H.compare_with_oracle(scn, net, monkeypatch, label=label, lds_limit=160 * 1024, **kw)
    return H.compare_with_oracle(scn, net, monkeypatch, label=label, lds_limit=160 * 1024, **kw)


@pytest.mark.parametrize('chunk', BASE_CHUNKS, ids=_ids)
def test_generated_networks_vs_oracle_with_the_librarys_own_plan(chunk, monkeypatch):
    """All 96 networks under the plan the library chooses (printed; the plan rules have tests/test_step_plan_gpu.py)."""
    for seed in chunk:
        _compare(seed, monkeypatch)


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_kernel_variants(variant, chunk, monkeypatch):
    """RANDOM_VARIANT_SEEDS under 512 and 1024 threads, without the helper wavefronts, with the 2- and 4-wide flat phase, in test
    mode (local rewards, the evaluation seeds), under Krauss with the network's own sigma (0, 0.3, 0.5 or 1.0) and with recording
    on (per-second rows, control rows and the trip log as test_recording_rows_and_trip_log compares them)."""
    for seed in chunk:
        _compare(seed, monkeypatch, variant)


# ---- controllers, in closed loop: the queues they see are their own ------------------------------------------------------------------
def _named(seed, what, call):
    try:
        return call()
    except AssertionError as ex:
        raise AssertionError('seed %d (%s): %s' % (seed, what, ex)) from ex


def _handle_and_oracles(seed, network=nw.random_network):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from oracle.env_oracle import OracleEnv
    net = network(seed)
    scn = net.scenario()
    env = VecTrafficEnv(scn, net.E, seed=net.seed)
    orc = [OracleEnv(scn, seed=net.seed + e) for e in range(net.E)]
    return net, scn, env, orc


def _greedy_loop(seed, network=nw.random_network):
    """greedy_kernel on the handle's observations chooses; its actions equal trainer.greedy_actions on the oracles' observations
    after the reset and every control step, and handle and oracles stay bit-equal under them."""
    from deeprl_signal_control_amd.trainer import greedy_actions
    net, scn, env, orc = _handle_and_oracles(seed, network)
    try:
        env.reset()
        obs = [o.reset() for o in orc]
        width = int(scn.agent_nlane.max())

        def draw(t, obs):
            wave = np.zeros((net.E, scn.n_agent, width))
            for e in range(net.E):
                for a in range(scn.n_agent):
                    wave[e, a, :scn.agent_nlane[a]] = obs[e][a][:scn.agent_nlane[a]]
            act = env.greedy_actions()
            np.testing.assert_array_equal(act.cpu().numpy(), greedy_actions(scn, wave), err_msg='action t=%d' % t)
            return act, H.agent_policies(scn, np.random.RandomState(net.seed + t), net.E) if scn.agent == 'ma2c' else None
        H.follow(env, H.oracle_steps(scn, orc, obs, net.steps, draw), state_at=[net.steps - 1], counters=True)
    finally:
        env.close()


def _pressure_loop(seed, measure, min_green, network=nw.random_network):
    """pressure_kernel chooses: at every step the full pressure array and the action equal the loop rule over the oracles' state and
    the hold bookkeeping of tests/test_pressure_gpu.py's test_hold (the action is the held phase)."""
    net, scn, env, orc = _handle_and_oracles(seed, network)
    tb = scn.pressure_tables()
    try:
        env.reset()
        obs = [o.reset() for o in orc]
        state = hold_state(net.E, scn.n_agent, min_green)

        def draw(t, obs):
            act, prs = env.max_pressure_actions(measure=measure, min_green=min_green, return_pressure=True)
            act_h, prs_h = act.cpu().numpy(), prs.cpu().numpy()
            for e in range(net.E):
                p_star, want = loop_pressure(scn, tb, orc[e].ms.snapshot(), measure)
                np.testing.assert_array_equal(prs_h[e], want, err_msg='pressure t=%d e=%d' % (t, e))
                hold_update(state, e, p_star, t, min_green)
                np.testing.assert_array_equal(act_h[e], state[0][e], err_msg='action t=%d e=%d' % (t, e))
            return act, H.agent_policies(scn, np.random.RandomState(net.seed + t), net.E) if scn.agent == 'ma2c' else None
        H.follow(env, H.oracle_steps(scn, orc, obs, net.steps, draw), state_at=[net.steps - 1], counters=True)
    finally:
        env.close()


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
def test_greedy_controller_in_closed_loop(chunk):
    for seed in chunk:
        _named(seed, 'greedy', lambda: _greedy_loop(seed))


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
def test_max_pressure_controller_in_closed_loop(chunk):
    """Both measures, min_green 1 and 3."""
    for seed in chunk:
        for measure in ('count', 'queue'):
            for g in (1, 3):
                _named(seed, 'pressure %s, min_green %d' % (measure, g), lambda: _pressure_loop(seed, measure, g))


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
@pytest.mark.parametrize('rule', ['actuated', 'sotl'])
def test_actuated_controllers_in_closed_loop(rule, chunk):
    """closed_loop of tests/test_actuated_gpu.py: actions, per-phase counts and the controller's state at every step."""
    from tests.test_actuated_gpu import RULES, closed_loop
    for seed in chunk:
        net = nw.random_network(seed)
        env = _named(seed, rule, lambda: closed_loop((net.scenario(), net.seed), net.E, net.steps, rule, RULES[rule], state_every=1))[0]
        env.close()
