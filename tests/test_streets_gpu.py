"""step_kernel's lane choice and lane changing (MICROSIM_SPEC.md rule 10; csrc/tsc_env.hip: the head walk's room and gap tests, the
third leader, the teleport of a wrong-lane head, the gather phase that takes lane changers before the junction's arrivals) and the
kernels around the step against the CPU oracle on the generated networks with two-lane streets of tests/networks.py
(random_street_network over RANDOM_STREET_SEEDS).  large_grid and its tilings reach rule 10 on one geometry -- 200 m signalised
streets entered from junctions under one connection pattern; here the streets are shorter than a detector or than a second's
travel, unsignalised, entry lanes, merge targets of two and three feeders, ends of routes, under control intervals of 1 to 8 s and
teleports after 15 s.  tests/test_streets_host.py states, on the oracle alone, how many of the 48 runs reach each clause and how
many tell a mutated rule from the true one.

Nothing here has a tolerance: the comparisons are env_harness.compare_with_oracle / follow and env_rules.check_lane_data /
check_trace.  A failure names the seed, the control step, the instance and the first field that differs.  The seed lists are fixed."""
import pytest

from tests import networks as nw
from tests import test_networks_random_gpu as R

pytestmark = pytest.mark.gpu

CHUNK = 8
BASE_CHUNKS = [nw.RANDOM_STREET_SEEDS[i:i + CHUNK] for i in range(0, len(nw.RANDOM_STREET_SEEDS), CHUNK)]
VARIANT_CHUNKS = [nw.RANDOM_STREET_VARIANT_SEEDS[i:i + CHUNK] for i in range(0, len(nw.RANDOM_STREET_VARIANT_SEEDS), CHUNK)]
_ids = R._ids
street = nw.random_street_network


@pytest.mark.parametrize('chunk', BASE_CHUNKS, ids=_ids)
def test_street_networks_vs_oracle_with_the_librarys_own_plan(chunk, monkeypatch):
    """All 48 networks under the plan the library chooses (printed): observations, rewards, done, the counters and the full vehicle
    state at the peak and at the end."""
    for seed in chunk:
        R._compare(seed, monkeypatch, network=street)


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
@pytest.mark.parametrize('variant', list(R.VARIANTS))
def test_kernel_variants(variant, chunk, monkeypatch):
    """RANDOM_STREET_VARIANT_SEEDS under every entry of test_networks_random_gpu.VARIANTS: 512 and 1024 threads, without the helper
    wavefronts, the 2- and 4-wide flat phase, test mode, Krauss with the network's own sigma, and with recording on (tests/
    test_streets_host.py: vehicles arrive in every instance of these runs)."""
    for seed in chunk:
        R._compare(seed, monkeypatch, variant, network=street)


# ---- trace and lane data --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.street_walks(), ids=repr)
def test_trace_and_lane_data_vs_oracle(case):
    """The walk of tests/test_networks_aux_gpu.py on six of the variant networks, the longest street and its sibling in pieces cut at
    positions that are no float32 values: every second's trajectory rows and every slot's sums of every interval equal the oracle's
    vehicles; laneChangedFrom and laneChangedTo each add up to the lane changes the oracle itself counts."""
    from tests.test_networks_aux_gpu import _walk
    ids, sums = _walk(case)
    want = nw.walk_lane_changes(case)
    assert sorted(sums) == sorted(want) == sorted(case.watch)
    for e in case.watch:
        assert sums[e]['laneChangedFrom'] == sums[e]['laneChangedTo'] == want[e], (e, sums[e], want[e])
    assert sum(want.values()) > 0 and min(ids.values()) > 0
    assert min(s['departed'] for s in sums.values()) > 0


# ---- controllers, in closed loop: the queues they see are their own ------------------------------------------------------------------
@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
def test_greedy_controller_in_closed_loop(chunk):
    for seed in chunk:
        R._named(seed, 'greedy', lambda: R._greedy_loop(seed, street))


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
def test_max_pressure_controller_in_closed_loop(chunk):
    """Both measures, min_green 1 and 3.  The movement tables leave the wrong-lane (lane, route) pairs out (lane_route_mov == -1:
    a vehicle that has to move over counts for no movement), and such pairs occur on signalised lanes of the chunk."""
    pairs = {seed: nw.wrong_lane_pairs(street(seed).scenario()) for seed in chunk}
    assert sum(len(p) for p in pairs.values()) > 0
    for seed in chunk:
        mov = street(seed).scenario().pressure_tables()['lane_route_mov']
        assert all(mov[l, r] == -1 for l, r in pairs[seed]), seed
        for measure in ('count', 'queue'):
            for g in (1, 3):
                R._named(seed, 'pressure %s, min_green %d' % (measure, g), lambda: R._pressure_loop(seed, measure, g, street))


@pytest.mark.parametrize('chunk', VARIANT_CHUNKS, ids=_ids)
@pytest.mark.parametrize('rule', ['actuated', 'sotl'])
def test_actuated_controllers_in_closed_loop(rule, chunk):
    """closed_loop of tests/test_actuated_gpu.py: actions, per-phase counts and the controller's state at every step."""
    from tests.test_actuated_gpu import RULES, closed_loop
    for seed in chunk:
        net = street(seed)
        env = R._named(seed, rule, lambda: closed_loop((net.scenario(), net.seed), net.E, net.steps, rule, RULES[rule], state_every=1))[0]
        env.close()
