"""Host-side checks of the opt-in target network / Double DQN of the Q-learners: the float64 restatement the GPU tests compare
against (tests/iql_ext_oracle.py) and the configuration keys (`target_update`, `double_q`)."""
import numpy as np
import pytest
import torch

from oracle.iql_oracle import OracleQ
from tests.iql_ext_oracle import ExtOracleIQL, ExtOracleQ


def _dqn_params(rng, nw=5, nt=3, fc=8, h=6, na=4):
    return {'fcw_w': rng.randn(nw, fc), 'fcw_b': rng.randn(fc) * .1, 'fct_w': rng.randn(nt, fc // 4), 'fct_b': rng.randn(fc // 4) * .1,
            'fc0_w': rng.randn(fc + fc // 4, h), 'fc0_b': rng.randn(h) * .1, 'q_w': rng.randn(h, na), 'q_b': rng.randn(na) * .1}


def _batch(rng, n=12, ns=8, na=4):
    return (rng.rand(n, ns) * 2, rng.randint(0, na, n), rng.rand(n, ns) * 2, rng.rand(n) < 0.3, -rng.rand(n) * 2)


@pytest.mark.parametrize('double_q', [False, True])
def test_target_equal_to_parameters_is_the_reference_loss(double_q):
    """theta- = theta: max_j Q(s')[j] = Q(s')[argmax_j Q(s')[j]], so both modes are OracleQ.loss_and_grads, exactly."""
    rng = np.random.RandomState(0)
    p = _dqn_params(rng)
    obs, acts, nobs, dones, rs = _batch(rng)
    ref = OracleQ(p, 5, 3)
    new = ExtOracleQ(p, 5, 3, target_update=3, double_q=double_q)
    l0, g0 = ref.loss_and_grads(obs, acts, nobs, dones, rs)
    l1, g1 = new.loss_and_grads(obs, acts, nobs, dones, rs)
    assert l0 == l1 and set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert (new.last_astar is not None) == double_q


def test_hand_computed_targets():
    """IQL-LR nets with one-hot observations, so that Q(s) is a row of q_w: 2 rows, 3 actions, worked by hand."""
    Wo = np.array([[1.0, 5.0, 2.0], [4.0, 0.0, 3.0]])           # online Q(s') of the two next states: argmax 1 and 0
    Wt = np.array([[7.0, 1.0, 2.0], [0.5, 6.0, 8.0]])           # target Q(s'):                          argmax 0 and 2
    b = np.zeros(3)
    obs = np.eye(2)                                             # Q(s) = Wo rows
    nobs, acts = np.eye(2), [2, 0]
    rs, gamma = [0.25, -1.0], 0.5
    for double_q, q1 in ((False, [7.0, 8.0]), (True, [1.0, 0.5])):
        o = ExtOracleQ({'q_w': Wo, 'q_b': b}, 2, 0, gamma=gamma, target_update=1, double_q=double_q)
        o.set_target({'q_w': Wt, 'q_b': b})
        loss, g = o.loss_and_grads(obs, acts, nobs, [False, False], rs)
        y = np.array([0.25 + 0.5 * q1[0], -1.0 + 0.5 * q1[1]])
        np.testing.assert_array_equal(o.last_y, y)
        if double_q:
            np.testing.assert_array_equal(o.last_astar, [1, 0])
            assert list(np.argmax(Wt, 1)) == [0, 2]             # the online pick is not the target net's own maximum
        d = np.array([Wo[0, 2], Wo[1, 0]]) - y                  # Q(s)[a] - y
        assert loss == pytest.approx((d ** 2).mean(), rel=1e-15)
        gw = np.zeros((2, 3)); gw[0, 2] = d[0]; gw[1, 0] = d[1]  # dLoss/dq_w = s^T (2 d / n) at the taken action; y carries no gradient
        np.testing.assert_allclose(g['q_w'].numpy(), gw, rtol=1e-15)
        # done rows: y = r, whatever the nets say
        o.loss_and_grads(obs, acts, nobs, [True, False], rs)
        np.testing.assert_array_equal(o.last_y, [0.25, y[1]])
    # a tie in the online values: the first maximum, like np.argmax
    o = ExtOracleQ({'q_w': np.array([[3.0, 3.0, 1.0], [0.0, 2.0, 2.0]]), 'q_b': b}, 2, 0, gamma=1.0, target_update=1, double_q=True)
    o.set_target({'q_w': Wt, 'q_b': b})
    o.loss_and_grads(obs, acts, nobs, [False, False], [0.0, 0.0])
    np.testing.assert_array_equal(o.last_astar, [0, 1])
    np.testing.assert_array_equal(o.last_y, [7.0, 6.0])


@pytest.mark.parametrize('N', [1, 2, 3])
def test_refresh_after_every_nth_adam_step_only(N):
    rng = np.random.RandomState(1)
    o = ExtOracleQ(_dqn_params(rng), 5, 3, target_update=N)
    eq = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    assert eq(o.target, o.p)
    frozen = {k: v.clone() for k, v in o.target.items()}
    for step in range(1, 3 * N + 2):
        o.backward(*_batch(rng), lr=1e-2)
        assert o.t == step
        if step % N == 0:
            assert eq(o.target, o.p)
            frozen = {k: v.clone() for k, v in o.target.items()}
        else:
            assert eq(o.target, frozen) and not eq(o.target, o.p)


def test_vector_oracle_uses_the_target_learners():
    rng = np.random.RandomState(2)
    ps = [_dqn_params(rng), _dqn_params(rng)]
    o = ExtOracleIQL(ps, [5, 5], [3, 3], [4, 4], 2, target_update=2, double_q=True, batch_size=3, buffer_size=8)
    assert all(isinstance(q, ExtOracleQ) and q.double_q and q.target_update == 2 for q in o.qs)
    for t in range(5):
        o.add_transition(rng.rand(2, 2, 8), rng.randint(0, 4, (2, 2)), -rng.rand(2, 2) * 3000, rng.rand(2, 2, 8), rng.rand(2) < .2)
    o.set_target_params([_dqn_params(rng), _dqn_params(rng)])
    t0 = o.target_params()
    o.minibatch_step(1e-3)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(t0, o.target_params()) for k in a)          # step 1: no refresh
    o.minibatch_step(1e-3)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(o.agent_params(), o.target_params()) for k in a)   # step 2: refreshed


def test_config_keys():
    from deeprl_signal_control_amd.agents import coerce_config
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, target_config
    assert IQL_DEFAULTS['target_update'] == 0 and IQL_DEFAULTS['double_q'] == 0
    assert target_config(coerce_config({}, IQL_DEFAULTS)) == (0, 0)
    cfg = coerce_config({'TARGET_UPDATE': '100', 'double_q': '1'}, IQL_DEFAULTS)           # a configparser section hands strings over
    assert cfg['target_update'] == 100 and isinstance(cfg['target_update'], int) and target_config(cfg) == (100, 1)
    assert target_config(coerce_config({'target_update': '5'}, IQL_DEFAULTS)) == (5, 0)
    with pytest.raises(ValueError, match='double_q'):
        target_config(coerce_config({'double_q': '1'}, IQL_DEFAULTS))
    with pytest.raises(ValueError):
        target_config(coerce_config({'target_update': '-1'}, IQL_DEFAULTS))
    with pytest.raises(ValueError):
        target_config(coerce_config({'target_update': '3', 'double_q': '2'}, IQL_DEFAULTS))
