"""GPU parity of the HIP Q-learner (csrc/tsc_iql.hip through the C-ABI, host mirror deeprl_signal_control_amd/iql.py)
against the float64 oracle of the reference's IQL agents (oracle/iql_oracle.py: agents/models.py:264-376,
agents/policies.py:285-389, agents/utils.py:231-263).

Tolerances (fp32 kernels vs float64 oracle): Q values |d| <= 2e-5; gradients |d| <= 2e-5 * max|g| per tensor (hidden
units within 1e-6 of a ReLU kink excepted); replay contents and minibatch indices exact; after an Adam step the
parameter change agrees to 2e-6 wherever the gradient is well above that tolerance (Adam's first steps move every
weight by ~lr * sign(g), so an entry whose gradient is rounding noise may legitimately move the other way)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import iql_harness as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('scenario,agent,model_type,E', [('large_grid', 'iqld', 'dqn', 70), ('large_grid', 'iqll', 'lr', 33),
                                                         ('real_net', 'iqld', 'dqn', 40), ('real_net', 'iqll', 'lr', 5)])
def test_forward_and_epsilon_greedy(scenario, agent, model_type, E):
    scn, m, o = H.make(scenario, agent, model_type, E, seed=3)
    assert scn.n_f_ls == [0] * scn.n_agent and (scenario == 'real_net') == (max(scn.n_w_ls) == 0)
    H.forward_and_act(scn, m, o, E, np.random.RandomState(E))
    m.close()


# fused: '1' = the one-kernel DeepQPolicy learner (csrc/tsc_iql_fused.h, what bench.py --config q1 times), '0' = the grouped-GEMM
# path (TSC_IQL_FUSED=0; IQL-LR always takes it).  E = 1024 x batch 20 = the 20 480 rows per agent of the benchmarked batch,
# distinct transitions in every instance; E = 70 leaves the last 64-row chunk ragged (1400 = 21 x 64 + 56),
# E = 3 is a single partial chunk.
@pytest.mark.parametrize('scenario,agent,model_type,E,cap,fused', [
    ('large_grid', 'iqld', 'dqn', 6, 30, '1'), ('large_grid', 'iqld', 'dqn', 6, 30, '0'), ('large_grid', 'iqll', 'lr', 9, 1000, '0'),
    ('real_net', 'iqld', 'dqn', 4, 64, '1'), ('real_net', 'iqld', 'dqn', 4, 64, '0'), ('large_grid', 'iqld', 'dqn', 3, 25, '1'),
    ('large_grid', 'iqld', 'dqn', 70, 22, '1'), ('large_grid', 'iqld', 'dqn', 1024, 22, '1'), ('large_grid', 'iqld', 'dqn', 1024, 22, '0'),
    ('real_net', 'iqld', 'dqn', 512, 22, '1'), ('large_grid', 'iqll', 'lr', 1024, 22, '0'),         # IQL-LR at the benchmarked batch too
    ('small_grid', 'iqld', 'dqn', 7, 40, '1')])              # s_max 12, 2 - 3 actions, wait inputs in the first 16-feature group
def test_replay_minibatch_gradient_and_adam(scenario, agent, model_type, E, cap, fused, monkeypatch):
    """Fill the rings past their capacity, then three minibatch steps: replay indices (Floyd on the documented
    uniform) exact, TD loss / gradient / clip norm / Adam-updated parameters against the oracle."""
    monkeypatch.setenv('TSC_IQL_FUSED', fused)
    scn, m, o = H.make(scenario, agent, model_type, E, seed=5, buffer_size=cap)
    assert m.fused == (fused == '1')
    H.replay_vs_oracle(scn, m, o, E, cap, np.random.RandomState(cap + E))
    m.close()


def test_iql_trainer_and_reference_loop_at_E1():
    """VecTrainer drives the IQL agents (utils.py:142-193 value-based branch, :284-295): epsilon decays per control
    step, nothing is learned until the rings hold a batch, then 10 Adam steps per rollout; the E = 1 adaptor driven by
    the reference's own loop lands on the same parameters bit for bit (same kernels, same order)."""
    from deeprl_signal_control_amd.env import TrafficEnv, VecTrafficEnv
    from deeprl_signal_control_amd.iql import IQL, VecIQL
    from deeprl_signal_control_amd.scenario import build_large_grid
    from deeprl_signal_control_amd.trainer import VecTrainer
    scn = build_large_grid('iqld', episode_length_sec=300)                  # 60 control steps = 3 rollouts of 20
    cfg = dict(batch_size=20, buffer_size=1000, reward_norm=3000.0)
    venv = VecTrafficEnv(scn, 1, seed=12, seed_stride=1)
    vmod = VecIQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1, scn.s_max, 5, cfg, total_step=1000, seed=0, model_type='dqn')
    p0 = vmod.get_flat().copy()
    tr = VecTrainer(venv, vmod)
    for _ in range(6):
        tr.run_iteration()
    torch.cuda.synchronize()
    assert vmod.eps_scheduler.n == 120 and vmod.update_step == 60 and vmod.get_opt_state()[2] == 60
    assert np.abs(vmod.get_flat() - p0).max() > 0
    # the reference's loop (utils.py:255-308, value-based branch) on the E = 1 adaptor
    env = TrafficEnv(scn, seed=12)
    model = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, cfg, seed=0, model_type='dqn')
    for _ in range(2):
        ob = env.reset()
        model.reset()
        while True:
            for _ in range(model.n_step):
                action, policy = model.forward(ob, mode='explore')
                next_ob, reward, done, global_reward = env.step(action)
                model.add_transition(ob, action, reward, next_ob, done)
                if done:
                    break
                ob = next_ob
            model.backward(None, 0)
            if done:
                env.terminate()
                break
    np.testing.assert_array_equal(model.vec.get_flat(), vmod.get_flat())
    # evaluation path: greedy and stochastic action selection
    venv.train_mode = False
    mean, std = tr.perform(0, 'default')
    assert mean.shape == (1,) and mean[0] < 0
    for x in (venv, env):
        x.close()
    vmod.close(); model.vec.close()


def test_every_instance_draws_its_own_minibatch():
    """Identical rings in every instance: the replay uniforms are keyed by (instance, agent), so the instances still
    draw different minibatches (independent samples, as E independent reference learners would)."""
    from deeprl_signal_control_amd import _lib
    E = 4
    scn, full, _ = H.make('large_grid', 'iqld', 'dqn', E, seed=2, buffer_size=40)
    rng = np.random.RandomState(0)
    A = scn.n_agent
    obs = H.rand_obs(scn, 1, rng)
    for t in range(30):
        nobs = H.rand_obs(scn, 1, rng)
        act = rng.randint(0, 5, (1, A)).astype(np.int32)
        rew = -rng.rand(1, A) * 6000.0
        full.add_transition(torch.from_numpy(np.repeat(obs, E, 0)).cuda(), torch.from_numpy(np.repeat(act, E, 0)).cuda(),
                            torch.from_numpy(np.repeat(rew, E, 0)).cuda(), torch.from_numpy(np.repeat(nobs, E, 0)).cuda(),
                            torch.zeros(E, dtype=torch.uint8, device='cuda'))
        obs = nobs
    _lib.check(full._L.tsc_iql_compute_grads(full._h, 77, 0))
    idx = np.zeros((E, A, 20), np.int32)
    _lib.check(full._L.tsc_iql_debug_batch(full._h, idx.ctypes.data_as(C.c_void_p)))
    assert len({tuple(idx[e, 0]) for e in range(E)}) == E
    gf = full.grad_tensor().cpu().numpy()
    assert np.isfinite(gf).all() and np.abs(gf).max() > 0
    full.close()


def test_other_batch_sizes_take_the_generic_draw_and_the_same_kernels():
    """batch_size != 20 (the reference's value, which has its own register-resident Floyd draw): the generic sampler and the fused
    learner at 8 rows per instance -- indices exact, gradients against the oracle."""
    from deeprl_signal_control_amd import _lib
    scn, m, o = H.make('large_grid', 'iqld', 'dqn', 9, seed=4, buffer_size=16, batch_size=8)
    assert m.fused and m.n_step == 8
    A, B, E = scn.n_agent, 8, 9
    rng = np.random.RandomState(1)
    obs = H.rand_obs(scn, E, rng)
    for t in range(19):
        nobs = H.rand_obs(scn, E, rng)
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, A) * 3.0 * m.cfg['reward_norm']
        done = (rng.rand(E) < 0.1).astype(np.uint8)
        m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(),
                         torch.from_numpy(nobs).cuda(), torch.from_numpy(done).cuda())
        o.add_transition(obs, act, rew, nobs, done)
        obs = nobs
    _lib.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    idx = np.zeros((E, A, B), np.int32)
    _lib.check(m._L.tsc_iql_debug_batch(m._h, idx.ctypes.data_as(C.c_void_p)))
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    losses, norms, og = o.minibatch_step(1e-3)
    np.testing.assert_array_equal(idx, o.last_idx)
    assert all(len(set(idx[e, a])) == B and idx[e, a].max() < 16 for e in range(E) for a in range(A))
    for a in range(A):
        for k, ref in og[a].items():
            scale = max(np.abs(ref).max(), 1e-9)
            # 72 rows: a unit within 1e-6 of its ReLU kink is a ~ 1e-4 event per tensor; such a tensor would fail loudly, not silently
            assert np.abs(g[a][k] - ref).max() <= 5e-5 * scale, (a, k)
    m.close()
