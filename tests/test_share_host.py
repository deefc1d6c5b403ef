"""Parameter sharing across like-shaped agents (INTEGRATION.md "Parameter sharing"), the host side: the classes of the built-in
scenarios, the config key, and share_mean -- the float64 restatement of share_reduce_kernel (csrc/tsc_model.hip) that
tests/test_share_gpu.py requires the kernel to equal bit for bit.  No GPU, no library."""
import numpy as np
import pytest

from deeprl_signal_control_amd.agents import (A2C_DEFAULTS, PPO_DEFAULTS, SHARE_DEFAULTS, check_share_config, coerce_config,
                                              share_classes)
from tests.layouts import Layout


def share_mean(grads, class_of):
    """grads float32 [A, per_agent], class_of [A] -> a new array in which every member of a class of two or more agents holds the class
    mean: a float64 sum over the members in ascending agent order, times the float64 1 / k, rounded once to float32.  Agents alone
    in their class keep their values."""
    grads = np.asarray(grads, np.float32)
    out = grads.copy()
    for c in sorted(set(class_of)):
        members = [a for a, x in enumerate(class_of) if x == c]
        k = len(members)
        if k < 2:
            continue
        acc = np.zeros(grads.shape[1], np.float64)
        for a in members:
            acc = acc + grads[a].astype(np.float64)
        with np.errstate(over='ignore'):
            mean = (acc * (1.0 / k)).astype(np.float32)
        for a in members:
            out[a] = mean
    return out


def class_sizes(class_of):
    return sorted((list(class_of).count(c) for c in set(class_of)), reverse=True)


def _classes(scenario, agent):
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(scenario, agent)
    n_f = list(scn.n_f_ls) if agent == 'ma2c' else [0] * scn.n_agent
    n_wave = [s - w - f for s, w, f in zip(scn.n_s_ls, scn.n_w_ls, n_f)]
    dims = list(zip(n_wave, scn.n_w_ls, n_f, scn.n_a_ls))
    return share_classes(n_wave, scn.n_w_ls, n_f, scn.n_a_ls), dims


@pytest.mark.parametrize('scenario,agent,sizes', [
    ('large_grid', 'ma2c', [12, 9, 4]), ('large_grid', 'ia2c', [12, 9, 4]),
    ('small_grid', 'ma2c', [3, 2, 1]), ('small_grid', 'ia2c', [3, 2, 1]),
    ('real_net', 'ia2c', [2] * 4 + [1] * 20), ('real_net', 'ma2c', [2] + [1] * 26)])
def test_classes_of_the_built_in_scenarios(scenario, agent, sizes):
    cls, dims = _classes(scenario, agent)
    assert class_sizes(cls) == sizes
    for a, c in enumerate(cls):
        assert c <= a and cls[c] == c and dims[a] == dims[c]               # the id is the lowest member's index
        assert all(dims[b] != dims[a] for b in range(a) if cls[b] != c)    # and no earlier agent of the same shape was missed


def test_class_ids_are_lowest_member_indices():
    lay = Layout([(3, 1, 0, 2)] * 2 + [(1, 1, 0, 2)] + [(3, 1, 0, 2)], 4)
    assert share_classes(lay.n_wave_ls, lay.n_w_ls, lay.n_f_ls, lay.n_a_ls) == [0, 0, 2, 0]
    # equal observation width is not enough: every one of the four numbers counts
    assert share_classes([3, 2, 3, 3], [1, 2, 1, 1], [0, 0, 0, 1], [2, 2, 3, 2]) == [0, 1, 2, 3]


def test_distinct_agents_are_singletons():
    lay = Layout([(30, 6, 16, 5), (24, 6, 12, 5), (18, 6, 8, 5), (24, 6, 12, 4), (18, 5, 8, 5)], 52)
    assert share_classes(lay.n_wave_ls, lay.n_w_ls, lay.n_f_ls, lay.n_a_ls) == [0, 1, 2, 3, 4]


def test_config_key():
    defaults = {**A2C_DEFAULTS, **PPO_DEFAULTS, **SHARE_DEFAULTS}
    assert check_share_config(coerce_config({}, defaults)) == 0
    assert check_share_config(coerce_config({'share_params': '1'}, defaults)) == 1
    assert check_share_config(coerce_config({'SHARE_PARAMS': ' 0 '}, defaults)) == 0
    for bad in ('2', '-1', 2, 0.5, True, None):
        with pytest.raises(ValueError, match='share_params'):
            check_share_config(coerce_config({'share_params': bad}, defaults))


def test_share_mean_is_the_mean_and_leaves_singletons_alone():
    rng = np.random.RandomState(4)
    A, n = 9, 257
    g = (rng.standard_normal((A, n)) * 10.0 ** rng.randint(-6, 6, (A, n))).astype(np.float32)
    cls = [0, 1, 0, 3, 1, 0, 6, 1, 1]                                        # classes of 3 and 4, two singletons
    out = share_mean(g, cls)
    for c in (0, 1):
        members = [a for a, x in enumerate(cls) if x == c]
        ref = np.mean(g[members].astype(np.float64), 0)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(out[members[0]].astype(np.float64) - ref) <= ulp)
        for a in members[1:]:
            np.testing.assert_array_equal(out[a].view(np.uint32), out[members[0]].view(np.uint32))
    for a in (3, 6):
        np.testing.assert_array_equal(out[a].view(np.uint32), g[a].view(np.uint32))
    np.testing.assert_array_equal(share_mean(g, list(range(A))).view(np.uint32), g.view(np.uint32))
    # two members: the float64 sum is exact, so the result is the correctly rounded mean -- and 1e30 - 1e30 is 0, not nan
    pair = np.array([[1e30, -1e30, 1.0, 1e-45, 3.0], [1e30, 1e30, 2.0, 1e-45, 1e-40]], np.float32)
    got = share_mean(pair, [0, 0])[0]
    want = ((pair[0].astype(np.float64) + pair[1].astype(np.float64)) * 0.5).astype(np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[1] == 0 and got[0] == np.float32(1e30) and got[3] == np.float32(1e-45)
