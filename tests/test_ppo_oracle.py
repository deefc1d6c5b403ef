"""The float64 reference of the PPO update (tests/ppo_oracle.py PPOOracle) against OracleA2C and plain Python, and the config
surface of `algo = ppo` -- no GPU.  What the HIP path is held to lives in tests/test_ppo_gpu.py."""
import configparser

import numpy as np
import pytest

from deeprl_signal_control_amd.agents import A2C_DEFAULTS, PPO_DEFAULTS, check_algo_config, coerce_config
from deeprl_signal_control_amd.scenario import build_scenario
from oracle.nets_oracle import OracleA2C
from tests.ppo_oracle import K3_REWARD_NORM, K3_SMALL, PPOOracle, fill, k3_conditions, make_oracle


@pytest.mark.parametrize('agent,policy', [('ma2c', 'lstm'), ('ia2c', 'fc')])
def test_k1_lambda1_is_the_a2c_oracle(agent, policy):
    """K = 1, lambda = 1: the same gradients and, after two rollouts (the second one from the carried LSTM state and done), the
    same parameters as OracleA2C, to float64 round-off -- ratio = 1, so the surrogate's gradient is the A2C policy gradient."""
    scn = build_scenario('large_grid', agent)
    E, T = 6, 5
    o = make_oracle(scn, agent, policy, E, 3, gae_lambda=1.0)
    ref = OracleA2C(o.tower_params_f64(), o.nw, o.nt, o.nf, o.na, E, gamma=o.gamma, reward_norm=o.rnorm, reward_clip=o.rclip,
                    value_coef=o.vcoef, max_grad_norm=o.max_norm)
    o.reset(); ref.reset()
    r1, r2 = np.random.RandomState(4), np.random.RandomState(4)
    ob1 = d1 = ob2 = d2 = None
    for it in range(2):
        ob1, d1 = fill(scn, o, E, T, r1, o.rnorm, ob1, d1, done_at=(T - 1,) if it == 0 else ())
        ob2, d2 = fill(scn, ref, E, T, r2, o.rnorm, ob2, d2, done_at=(T - 1,) if it == 0 else ())
        _, Rb = ref.forward(ob2, np.zeros(E), 'v')
        Rb = Rb.astype(np.float32)
        g, st = o.compute_grads(Rb, 0.01, epoch=0)
        gr, str_ = ref.compute_grads(Rb, 0.01)
        np.testing.assert_array_equal(o.Rs, ref.Rs)
        np.testing.assert_array_equal(o.Advs, ref.Advs)
        assert o.clip_share.max() == 0 and np.abs(o.approx_kl).max() == 0
        for t in range(2 * scn.n_agent):
            for k in gr[t]:
                scale = max(float(gr[t][k].abs().max()), 1e-30)
                assert float((g[t][k] - gr[t][k]).abs().max()) <= 1e-12 * scale, (it, t, k)
        np.testing.assert_allclose(st[:, 1:], str_[:, 1:], rtol=1e-12)
        n1, n2 = o.apply_grads(g, 5e-4), ref.apply_grads(gr, 5e-4)
        np.testing.assert_allclose(n1, n2, rtol=1e-12)
        for p, q in zip(o.tower_params_f64(), ref.tower_params_f64()):
            for k in q:
                np.testing.assert_allclose(p[k], q[k], rtol=0, atol=1e-13)


def test_gae_against_a_plain_loop():
    """lambda = 1 is returns_advs; lambda < 1 equals a scalar Python loop over one (instance, agent) series at a time, with
    dones in the middle and at the end of the window."""
    rng = np.random.RandomState(0)
    T, E, A, gamma = 12, 5, 3, 0.99
    rs, vs = -rng.rand(T, E, A) * 2, rng.randn(T, E, A).astype(np.float32).astype(np.float64)
    R = rng.randn(E, A).astype(np.float32)
    dones = np.zeros((T + 1, E, A))
    dones[5, 1] = 1; dones[8, 2] = 1; dones[T, 3] = 1; dones[3, 4] = 1; dones[T, 4] = 1
    a, b = PPOOracle.gae(rs, vs, dones, R, gamma, 1.0), OracleA2C.returns_advs(rs, vs, dones, R, gamma)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    for lam in (0.9, 0.95, 0.5):
        Rs, Advs = PPOOracle.gae(rs, vs, dones, R, gamma, lam)
        assert Rs.dtype == np.float32 and Advs.dtype == np.float32
        for e in range(E):
            for ag in range(A):
                adv, want = 0.0, [0.0] * T
                for t in reversed(range(T)):
                    vn = float(R[e, ag]) if t == T - 1 else vs[t + 1, e, ag]
                    nd = 1.0 - dones[t + 1, e, ag]
                    delta = rs[t, e, ag] + gamma * vn * nd - vs[t, e, ag]
                    adv = delta + gamma * lam * nd * adv
                    want[t] = adv
                np.testing.assert_array_equal(Advs[:, e, ag], np.array(want).astype(np.float32))
                np.testing.assert_array_equal(Rs[:, e, ag], (np.array(want) + vs[:, e, ag]).astype(np.float32))
        # a terminal step cuts the window: what happens after it does not reach the steps before it
        rs2 = rs.copy(); rs2[6:, 1] -= 1.0
        assert np.array_equal(PPOOracle.gae(rs2, vs, dones, R, gamma, lam)[1][:5, 1], Advs[:5, 1])


@pytest.mark.parametrize('agent,policy,E,T,seed,rseed,lr', K3_SMALL)
def test_k3_cases_exercise_the_clip_on_the_oracle_alone(agent, policy, E, T, seed, rseed, lr):
    """The seeds and lr of the K = 3 GPU comparison, on the oracle alone (stored values: the oracle's own forward rounded to
    float32; on the GPU box they are the HIP forward's, 2e-5 away): clipped share at epochs 1 and 2 in [5 %, 50 %], ambiguous
    samples at most 0.5 %, epoch 0 unclipped with zero KL."""
    scn = build_scenario('large_grid', agent)
    o = make_oracle(scn, agent, policy, E, seed, cfg=dict(reward_norm=K3_REWARD_NORM))
    o.reset()
    obs, _ = fill(scn, o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM)
    _, Rb = o.forward(obs, np.zeros(E), 'v')
    for k in range(3):
        g, _ = o.compute_grads(Rb.astype(np.float32), 0.01, epoch=k, slack=False)
        clip, amb = k3_conditions(o, k)
        if k == 0:
            assert clip == 0 and np.abs(o.approx_kl).max() == 0
        else:
            assert o.approx_kl.mean() > 0
        print('%s %s epoch %d: clipped %.3f ambiguous %.4f kl %.4f' % (agent, policy, k, clip, amb, o.approx_kl.mean()))
        o.apply_grads(g, lr, end_of_rollout=k == 2)
    assert o.logp_old is None and len(o.buf['obs']) == 0


INI = """
[MODEL_CONFIG]
batch_size = 120
algo = %s
ppo_epochs = %s
ppo_clip = %s
gae_lambda = %s
"""


def _cfg(algo='ppo', epochs='4', clip='0.2', lam='0.95'):
    c = configparser.ConfigParser()
    c.read_string(INI % (algo, epochs, clip, lam))
    return coerce_config(c['MODEL_CONFIG'], {**A2C_DEFAULTS, **PPO_DEFAULTS})


def test_config_keys():
    """[MODEL_CONFIG] algo / ppo_epochs / ppo_clip / gae_lambda: typed like the other keys, absent keys mean A2C, anything else
    is rejected with the key's name."""
    assert check_algo_config(coerce_config({'batch_size': '120'}, {**A2C_DEFAULTS, **PPO_DEFAULTS})) == ('a2c', 4, 0.2, 0.95)
    assert check_algo_config(coerce_config(None, {**A2C_DEFAULTS, **PPO_DEFAULTS}))[0] == 'a2c'
    assert check_algo_config(_cfg()) == ('ppo', 4, 0.2, 0.95)
    assert check_algo_config(_cfg('PPO', '1', '0.1', '1.0')) == ('ppo', 1, 0.1, 1.0)
    assert check_algo_config(coerce_config({'ALGO': 'ppo', 'PPO_EPOCHS': 3}, {**A2C_DEFAULTS, **PPO_DEFAULTS}))[:2] == ('ppo', 3)
    for bad, key in ((dict(algo='trpo'), 'algo'), (dict(epochs='0'), 'ppo_epochs'), (dict(epochs='-2'), 'ppo_epochs'),
                     (dict(clip='0'), 'ppo_clip'), (dict(clip='-0.1'), 'ppo_clip'), (dict(lam='0'), 'gae_lambda'),
                     (dict(lam='1.01'), 'gae_lambda'), (dict(lam='-0.5'), 'gae_lambda')):
        with pytest.raises(ValueError, match=key):
            check_algo_config(_cfg(**bad))
    assert 'algo' not in A2C_DEFAULTS                       # the reference's key set stays what it was
