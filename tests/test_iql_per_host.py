"""Host-side checks of the opt-in prioritized replay of the Q-learners: the float64 restatement the GPU tests compare against
(tests/iql_ext_oracle.py), the configuration keys (`prioritized_replay`, `per_alpha`, `per_beta`, `per_eps`) and the beta schedule."""
import numpy as np
import pytest
import torch

from tests.iql_ext_oracle import ExtOracleIQL, ExtOracleQ, per_draw, per_priority, per_weights


def test_hand_computed_three_slot_ring():
    """q = [1, 0, 3]: C = [1, 1, 4], total 4, two strata of width 2.  Picks, weights and the write-back worked by hand."""
    q = np.array([1.0, 0.0, 3.0], np.float32)
    # stratum 0 = [0, 2): t = 2 u.  u = .25 -> t = .5 < C[0] -> slot 0;  u = .75 -> t = 1.5: C[0] = C[1] = 1 <= t < C[2] -> slot 2 (never slot 1)
    assert per_draw(q, 3, 2, lambda i: [0.25, 0.0][i]) == [0, 2]
    assert per_draw(q, 3, 2, lambda i: [0.75, 0.999][i]) == [2, 2]
    assert per_draw(q, 3, 2, lambda i: [0.5, 0.5][i]) == [2, 2]                 # t = 1 = C[0]: "C[k] > t" is strict
    assert per_draw(q, 3, 2, lambda i: [0.4999, 0.5][i]) == [0, 2]
    # the mass in the last filled slot; the slot behind `size` is never looked at
    assert per_draw(np.array([0.0, 0.0, 2.0, 9.0], np.float32), 3, 2, lambda i: 0.0) == [2, 2]
    # weights: (size q / total)^-beta = (3/4)^-beta and (9/4)^-beta, over the larger one
    np.testing.assert_allclose(per_weights(q, 3, [0, 2], 1.0), [1.0, 1.0 / 3.0], rtol=1e-15)
    np.testing.assert_allclose(per_weights(q, 3, [0, 2], 0.5), [1.0, np.sqrt(1.0 / 3.0)], rtol=1e-15)
    np.testing.assert_array_equal(per_weights(q, 3, [0, 2], 0.0), [1.0, 1.0])
    np.testing.assert_array_equal(per_weights(q, 3, [2, 2], 1.0), [1.0, 1.0])    # normalised by the ring's OWN picks
    np.testing.assert_array_equal(per_weights(np.ones(5, np.float32), 5, [0, 3, 3], 0.4), [1.0, 1.0, 1.0])      # equal priorities: base exactly 1
    # write-back: (|delta| + eps)^alpha as float32
    assert per_priority(0.24, 0.01, 0.5) == np.float32(0.5)
    assert per_priority(123.0, 0.01, 0.0) == np.float32(1.0)
    assert per_priority(0.0, 0.01, 1.0) == np.float32(0.01)


def test_strata_and_proportions():
    """Every pick lies in its stratum of the cumulative mass, and over many draws a slot is picked in proportion to its priority."""
    rng = np.random.RandomState(0)
    q = rng.rand(37).astype(np.float32)
    q[[3, 4, 20]] = 0
    C = np.cumsum(q.astype(np.float64))
    B, cnt = 5, np.zeros(37)
    for rep in range(4000):
        u = rng.rand(B)
        picks = per_draw(q, 37, B, lambda i: u[i])
        for i, k in enumerate(picks):
            assert q[k] > 0 and C[k] > i * C[-1] / B and (C[k - 1] if k else 0.0) <= (i + 1) * C[-1] / B
            cnt[k] += 1
    np.testing.assert_allclose(cnt / cnt.sum(), q / q.sum(), atol=0.004)


def _lr_params():
    return {'q_w': np.array([[1.0, 5.0, 2.0], [4.0, 0.0, 3.0]]), 'q_b': np.zeros(3)}


def test_weighted_loss_and_gradient_by_hand():
    """IQL-LR with one-hot observations (Q(s) is a row of q_w): loss = mean(w delta^2), dLoss/dq_w[s, a] = 2 w delta / n."""
    o = ExtOracleQ(_lr_params(), 2, 0, gamma=0.5, target_update=0)
    obs, nobs, acts, rs = np.eye(2), np.eye(2), [2, 0], [0.25, -1.0]
    o.weights = np.array([1.0, 0.25])
    loss, g = o.loss_and_grads(obs, acts, nobs, [False, True], rs)
    y = np.array([0.25 + 0.5 * 5.0, -1.0])                                     # max of row 0; done row: y = r
    d = np.array([2.0, 4.0]) - y
    np.testing.assert_array_equal(o.last_delta, d)
    assert loss == pytest.approx((o.weights * d ** 2).mean(), rel=1e-15)
    gw = np.zeros((2, 3)); gw[0, 2] = 1.0 * d[0]; gw[1, 0] = 0.25 * d[1]
    np.testing.assert_allclose(g['q_w'].numpy(), gw, rtol=1e-15)
    # weights of 1 are the target oracle's loss, exactly
    ref = ExtOracleQ(_lr_params(), 2, 0, gamma=0.5, target_update=3)
    o.weights = None
    l0, g0 = ref.loss_and_grads(obs, acts, nobs, [False, True], rs)
    l1, g1 = o.loss_and_grads(obs, acts, nobs, [False, True], rs)
    assert l0 == l1 and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_vector_oracle_rings_priorities_and_write_back():
    rng = np.random.RandomState(2)
    ps = [_lr_params(), _lr_params()]
    o = ExtOracleIQL(ps, [2, 2], [0, 0], [3, 3], 2, per=True, alpha=0.5, eps=0.01, batch_size=3, buffer_size=4, reward_norm=1.0, reward_clip=0.0, replay_seed=9)
    assert (o.qmax == 1).all() and (o.prio == 0).all()
    for t in range(6):                                                          # wraps: slots 0 and 1 are overwritten
        o.add_transition(rng.rand(2, 2, 2), rng.randint(0, 3, (2, 2)), -rng.rand(2, 2), rng.rand(2, 2, 2), rng.rand(2) < .2)
    assert (o.prio == 1).all()
    before = o.prio.copy()
    o.minibatch_step(1e-3, beta=0.4)
    np.testing.assert_array_equal(o.last_w, np.ones((2, 6)))                    # equal priorities: every weight exactly 1
    for e in range(2):
        for a in range(2):
            picks = o.last_idx[e, a]
            assert all(picks[i] <= picks[i + 1] for i in range(2))              # strata are ordered
            for s in range(4):
                hits = [i for i in range(3) if picks[i] == s]
                if hits:                                                        # the LAST pick of a slot drawn twice stays
                    assert o.prio[e, a, s] == per_priority(o.last_td[a, e * 3 + hits[-1]], 0.01, 0.5)
                else:
                    assert o.prio[e, a, s] == before[e, a, s]
            assert o.qmax[e, a] == max(1.0, o.prio[e, a].max())
    # a new transition enters at the ring's maximum, in every ring
    slot = o.rings[0][0].cum_size % 4
    o.add_transition(rng.rand(2, 2, 2), rng.randint(0, 3, (2, 2)), -rng.rand(2, 2), rng.rand(2, 2, 2), rng.rand(2) < .2)
    np.testing.assert_array_equal(o.prio[:, :, slot], o.qmax)
    # unequal priorities now: weights below 1 appear and each ring's maximum is exactly 1
    o.prio[:, :, 0] *= 7
    o.minibatch_step(1e-3, beta=1.0)
    w = o.last_w.reshape(2, 2, 3)
    assert (w.max(2) == 1).all() and w.min() < 1
    # a caller's draw: clamped, the weights from those slots' priorities
    o.minibatch_step(1e-3, beta=1.0, idx_given=np.array([[[0, 9, -1]] * 2] * 2))
    np.testing.assert_array_equal(o.last_idx, np.array([[[0, 3, 0]] * 2] * 2))


def test_config_keys():
    from deeprl_signal_control_amd.agents import coerce_config
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, per_config
    assert [IQL_DEFAULTS[k] for k in ('prioritized_replay', 'per_alpha', 'per_beta', 'per_eps')] == [0, 0.6, 0.4, 0.01]
    assert per_config(coerce_config({}, IQL_DEFAULTS)) == (0, 0.6, 0.4, 0.01)
    cfg = coerce_config({'PRIORITIZED_REPLAY': '1', 'per_alpha': '0.7', 'per_beta': '0.5', 'per_eps': '1e-3'}, IQL_DEFAULTS)   # configparser hands strings over
    assert per_config(cfg) == (1, 0.7, 0.5, 1e-3) and isinstance(cfg['prioritized_replay'], int)
    assert per_config(coerce_config({'prioritized_replay': '1', 'per_alpha': '0', 'per_beta': '1'}, IQL_DEFAULTS)) == (1, 0.0, 1.0, 0.01)
    for bad in ({'prioritized_replay': '2'}, {'per_alpha': '-0.1'}, {'per_beta': '1.5'}, {'per_beta': '-0.1'}, {'per_eps': '0'},
                {'per_eps': '-1'}, {'per_alpha': 'nan'}):
        with pytest.raises(ValueError):
            per_config(coerce_config(bad, IQL_DEFAULTS))


def test_beta_schedule():
    from deeprl_signal_control_amd.iql import per_beta_at
    assert per_beta_at(0.4, 0, 100) == 0.4
    assert per_beta_at(0.4, 50, 100) == pytest.approx(0.7, rel=1e-15)
    assert per_beta_at(0.4, 100, 100) == 1.0 and per_beta_at(0.4, 250, 100) == 1.0
    assert per_beta_at(1.0, 30, 100) == 1.0
    assert per_beta_at(0.4, 30, 0) == 0.4                                       # no horizon: it stays where it starts
    b = [per_beta_at(0.25, n, 1000) for n in range(0, 1001, 20)]
    assert all(x < y for x, y in zip(b, b[1:])) and b[-1] == 1.0


def test_sampler_block_index_without_division():
    """iql_per_sample_kernel finds the block of slot g as (g M) >> 20 with M = ceil(2^20 / K) instead of g / K: exact, and inside 32 bits,
    for every slot below TSC_IQL_PER_MAX_BUFFER = 4096 and every block length K <= 64 the bound admits."""
    g = np.arange(4096, dtype=np.uint64)
    for K in range(1, 65):
        M = ((1 << 20) + K - 1) // K
        assert int(g[-1]) * M < 2 ** 32
        np.testing.assert_array_equal((g * np.uint64(M)) >> np.uint64(20), g // np.uint64(K))
