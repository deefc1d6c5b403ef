"""Host-side checks of the opt-in multi-step returns of the Q-learners ([MODEL_CONFIG] return_steps; deeprl_signal_control_amd/iql.py
return_steps_config) and self-checks of their float64 oracle (tests/iql_ext_oracle.py, return_steps) -- no GPU."""
import configparser

import numpy as np
import pytest

from deeprl_signal_control_amd.agents import coerce_config
from deeprl_signal_control_amd.iql import IQL_DEFAULTS, QParamLayout, init_agent_params
from tests.iql_ext_oracle import ExtOracleIQL, nstep_window

GAMMA = 0.9


def test_return_steps_config_defaults_strings_and_bad_values():
    from deeprl_signal_control_amd.iql import MAX_RETURN_STEPS, return_steps_config
    assert IQL_DEFAULTS['return_steps'] == 1 and MAX_RETURN_STEPS == 32
    assert return_steps_config(coerce_config(None, IQL_DEFAULTS)) == 1
    for good in (1, 3, 32, 3.0, '5', ' 7 '):
        assert return_steps_config({'return_steps': good}) == int(float(good))
    cp = configparser.ConfigParser()
    cp.read_string('[MODEL_CONFIG]\nRETURN_STEPS = 3\ndueling = 1\n')
    assert return_steps_config(coerce_config(cp['MODEL_CONFIG'], IQL_DEFAULTS)) == 3
    for bad in (0, 33, -1, 2.5, '2.5', 'three', None, float('nan'), float('inf'), True):
        with pytest.raises(ValueError, match='return_steps'):
            return_steps_config({'return_steps': bad})


def _ring(cap, cum, done_slots, seed=0):
    """A hand-made ring after `cum` adds: reward of the t-th transition (t = 0, 1, ..) is float32(-(t + 1) / 8) -- exact in binary, so
    every partial sum below is exact in float64 whenever gamma's powers are -- stored at slot t % cap."""
    size = min(cap, cum)
    rews, dones, age = np.zeros(cap, np.float32), np.zeros(cap, bool), np.full(cap, -1)
    for t in range(cum):
        rews[t % cap], age[t % cap] = np.float32(-(t + 1) / 8.0), t
    for s in done_slots:
        dones[s] = True
    return rews, dones, age, size


def _brute(rews, dones, age, s, cum, n, gamma):
    """The same window by unrolling the ring into its chronological order first: transitions age[s], age[s] + 1, .. up to n of them, up
    to the first done, up to the newest (cum - 1)."""
    chron = {int(t): slot for slot, t in enumerate(age) if t >= 0}
    t, terms = int(age[s]), []
    while True:
        slot = chron[t]
        terms.append(float(rews[slot]))
        if dones[slot] or t == cum - 1 or len(terms) == n:
            break
        t += 1
    G = sum(gamma ** i * r for i, r in enumerate(terms))
    return chron[t], G, gamma ** len(terms), len(terms)


def _check(cap, cum, done_slots, s, n, want_j=None, want_k=None):
    rews, dones, age, size = _ring(cap, cum, done_slots)
    j, G, disc, k = nstep_window(rews, dones, s, size, cap, cum, n, GAMMA)
    bj, bG, bdisc, bk = _brute(rews, dones, age, s, cum, n, GAMMA)
    assert (j, k) == (bj, bk)
    assert G == pytest.approx(bG, rel=1e-13) and disc == pytest.approx(bdisc, rel=1e-13)
    if want_j is not None:
        assert (j, k) == (want_j, want_k)
    return j, G, disc, k


def test_window_on_an_unfilled_ring():
    # 6 of 10 slots filled: w = size - 1 = 5 ends every window, nothing wraps
    _check(10, 6, [], 0, 3, 2, 3)
    _check(10, 6, [], 4, 3, 5, 2)            # cut by the newest slot after two steps
    _check(10, 6, [], 5, 3, 5, 1)            # s = w
    for s in range(6):
        j, _, _, k = _check(10, 6, [2], s, 4)
        assert s <= j <= 5 and k == j - s + 1


def test_window_on_a_wrapped_ring_with_the_newest_slot_in_the_middle():
    # cap 8, 13 adds: w = 4, the oldest transition sits at slot 5
    _check(8, 13, [], 5, 3, 7, 3)
    _check(8, 13, [], 6, 3, 0, 3)            # crosses cap - 1 -> 0
    _check(8, 13, [], 7, 3, 1, 3)
    _check(8, 13, [], 7, 1, 7, 1)            # n = 1: the slot itself, whatever lies behind it
    _check(8, 13, [], 3, 3, 4, 2)            # cut by w
    _check(8, 13, [], 4, 3, 4, 1)            # s = w: never walks into the oldest transition at slot 5
    _check(8, 13, [], 5, 32, 4, 8)           # n = 32 > cap: the whole ring once, stops at w before it returns to s
    _check(8, 13, [], 0, 32, 4, 5)


def test_window_cut_by_done_at_its_first_middle_and_last_step():
    _check(8, 13, [6], 6, 3, 6, 1)           # first
    _check(8, 13, [7], 6, 3, 7, 2)           # middle
    _check(8, 13, [0], 6, 3, 0, 3)           # last (k = n and done): no bootstrap
    _check(8, 13, [0], 6, 32, 0, 3)
    _check(8, 13, [4], 3, 3, 4, 2)           # the newest slot is itself terminal
    j, G, disc, k = _check(8, 13, [7], 6, 3)
    rews = _ring(8, 13, [])[0]
    assert G == float(rews[6]) + GAMMA * float(rews[7]) and disc == GAMMA * GAMMA


def test_every_slot_and_horizon_against_the_unroll():
    rng = np.random.RandomState(3)
    for cap, cum in ((5, 3), (5, 5), (5, 9), (7, 30), (22, 29)):
        size = min(cap, cum)
        done_slots = [s for s in range(size) if rng.rand() < 0.2]
        for s in range(size):
            for n in (1, 2, 3, 5, 32):
                _check(cap, cum, done_slots, s, n)


def _pair(n, **kw):
    """ExtOracleIQL() and ExtOracleIQL(return_steps = n) over the same parameters and transitions: the smallest layout of tests/layouts.py."""
    from tests.layouts import IQL_LAYOUTS, iql_transitions
    spec = IQL_LAYOUTS['lr_tiny']
    lay = spec['layout']
    pl = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, spec['model_type'], spec['cfg']['num_fc'], spec['cfg']['num_h'])
    params = init_agent_params(pl, np.random.RandomState(5))
    E, cap = 2, 24
    common = dict(batch_size=20, buffer_size=cap, gamma=0.99, reward_norm=100.0, reward_clip=2.0, replay_seed=11, **kw)
    ext = ExtOracleIQL(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, E, **common)
    nst = ExtOracleIQL(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, E, return_steps=n, **common)
    for tr in iql_transitions(lay, E, cap, np.random.RandomState(9), 100.0):
        ext.add_transition(*tr)
        nst.add_transition(*tr)
    return ext, nst


@pytest.mark.parametrize('kw', [{}, dict(target_update=2, double_q=True, per=True)])
def test_one_step_oracle_is_the_extension_oracle_exactly(kw):
    ext, nst = _pair(1, **kw)
    for step in range(2):
        le, ne, ge = ext.minibatch_step(1e-2)
        ln, nn, gn = nst.minibatch_step(1e-2)
        np.testing.assert_array_equal(nst.last_idx, ext.last_idx)
        np.testing.assert_array_equal(ln, le)
        np.testing.assert_array_equal(nn, ne)
        for a in range(ext.A):
            for k in ge[a]:
                np.testing.assert_array_equal(gn[a][k], ge[a][k])
            for k, v in ext.qs[a].p.items():
                np.testing.assert_array_equal(nst.qs[a].p[k].numpy(), v.numpy())
            np.testing.assert_array_equal(nst.qs[a].last_y, ext.qs[a].last_y)
        np.testing.assert_array_equal(nst.prio, ext.prio)
        assert (nst.last_k == 1).all() and (nst.last_disc == 0.99).all()
        np.testing.assert_array_equal(nst.last_slot, nst.last_idx)


def test_three_step_oracle_differs_and_its_windows_follow_the_rule():
    ext, nst = _pair(3)
    le, _, _ = ext.minibatch_step(1e-2)
    ln, _, _ = nst.minibatch_step(1e-2)
    np.testing.assert_array_equal(nst.last_idx, ext.last_idx)
    assert not np.array_equal(ln, le)
    cat = nst.categories()
    assert all(c.any() for c in cat.values()), {k: int(v.sum()) for k, v in cat.items()}
    size, cum = nst.rings[0][0].size, nst.rings[0][0].cum_size
    for a in range(nst.A):
        for e in range(nst.E):
            buf = nst.rings[e][a].buffer
            for i, s in enumerate(nst.last_idx[e, a]):
                r = e * nst.B + i
                j, G, disc, k = nstep_window([t[2] for t in buf], [t[4] for t in buf], s, size, nst.cap, cum, 3, 0.99)
                assert (nst.last_slot[e, a, i], nst.last_G[a, r], nst.last_disc[a, r], nst.last_k[a, r]) == (j, G, disc, k)
                y = nst.qs[a].last_y[r]
                assert (y == G) == bool(buf[j][4])
