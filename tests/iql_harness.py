"""Shared scaffolding of the Q-learner tests (tests/test_iql_*_gpu.py, the IQL part of tests/test_layouts_*.py, tests/test_cli_*_gpu.py) --
TEST INFRASTRUCTURE ONLY: case tables, model and oracle constructors, observation draws, the ring fill, ctypes accessors of the debug
surface of include/tsc.h, target arming, the gradient comparison, and the test bodies that more than one module runs.  One copy of each;
a test module keeps its tests and the helpers only it uses.

Tolerances are the project's (tests/test_iql_gpu.py): Q values, hence y = r + gamma Q and |delta|, |d| <= 2e-5; gradients |d| <= 2e-5 max|g|
per tensor, hidden units within 1e-6 of a ReLU kink excepted; loss and clip norm rtol 1e-4; replay contents, indices and a* exact."""
import ctypes as C

import numpy as np
import pytest
import torch

# scenario, agent, model_type, E, ring capacity, TSC_IQL_FUSED: the smallest shapes at which each path can go wrong -- E = 70 x batch 20 =
# 1400 rows = 21 x 64 + 56 (several row splits, a ragged last chunk), E = 3 one partial chunk, the grouped-GEMM path for IQL-DNN
# (TSC_IQL_FUSED=0) and IQL-LR, small_grid for the instantiation without a wait tile, real_net for heterogeneous action counts
CASES = [('large_grid', 'iqld', 'dqn', 70, 22, '1'), ('large_grid', 'iqld', 'dqn', 3, 25, '1'), ('large_grid', 'iqld', 'dqn', 6, 30, '0'),
         ('large_grid', 'iqll', 'lr', 9, 1000, '0'), ('small_grid', 'iqld', 'dqn', 7, 40, '1'), ('real_net', 'iqld', 'dqn', 4, 64, '1')]
GAP = 1e-4          # rows whose two best online values lie closer than this in float64 are re-drawn before they enter the rings
# the profile ids a minibatch step and an add can launch under (tsc_profile_read)
KERNELS = ('iql_sample', 'iql_per_sample', 'iql_nstep', 'iql_target', 'iql_grad', 'iql_reduce', 'iql_per_update', 'iql_per_add')

INI = """
[MODEL_CONFIG]
max_grad_norm = 40
gamma = 0.99
lr_init = 1e-4
lr_decay = constant
epsilon_init = 1.0
epsilon_min = 0.01
epsilon_decay = linear
epsilon_ratio = 0.5
num_fc = 128
num_h = 64
batch_size = 20
buffer_size = 1000
reward_norm = 100.0
reward_clip = 2.0
target_update = 5
double_q = 1

[TRAIN_CONFIG]
total_step = 120
test_interval = 60
log_interval = 60

[ENV_CONFIG]
clip_wave = 2.0
clip_wait = 2.0
control_interval_sec = 5
agent = iqld
coop_gamma = 0.9
data_path = ./small_grid/data/
episode_length_sec = 300
norm_wave = 5.0
norm_wait = 100.0
coef_wait = 0.2
num_extra_car_per_hour = 1000
objective = hybrid
scenario = small_grid
seed = 12
test_seeds = 10000,20000
yellow_interval_sec = 2
"""


def check(rc):
    from deeprl_signal_control_amd import _lib
    _lib.check(rc)


# ---- models and oracles ----------------------------------------------------------------------------------------------------------
def model(scenario, agent, model_type, E, seed=5, **cfg):
    """scenario: the name of a built-in scenario, or a layout object (tests/layouts.py: the attributes read below and nothing else)."""
    from deeprl_signal_control_amd.iql import VecIQL
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(scenario, agent) if isinstance(scenario, str) else scenario
    mc = dict(batch_size=20, buffer_size=1000, reward_norm=3000.0 if scenario == 'large_grid' else 1.0 if scenario == 'real_net' else 100.0)
    mc.update(cfg)
    a_max = int(scn.green_tab.shape[1]) if hasattr(scn, 'green_tab') else scn.a_max
    m = VecIQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, E, scn.s_max, a_max, mc, total_step=10000, seed=seed,
               model_type=model_type)
    return scn, m


def make(scenario, agent, model_type, E, seed=0, **cfg):
    """model() and the oracle of the reference's learner itself (oracle/iql_oracle.py), for the tests of the default configuration."""
    from oracle.iql_oracle import OracleIQL
    scn, m = model(scenario, agent, model_type, E, seed=seed, **cfg)
    o = OracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, E, batch_size=m.n_step,
                  buffer_size=int(m.cfg['buffer_size']), gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'],
                  reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'], replay_seed=m.replay_seed)
    return scn, m, o


def nontrivial(agents, rng):
    """Biases of both streams of a dueling head away from their zero initialisation (the weights are orthogonal draws already)."""
    for p in agents:
        p['q_b'] = (rng.randn(*p['q_b'].shape) * 0.3).astype(np.float32)
        p['v_b'] = (rng.randn(1) * 0.3 + 0.5).astype(np.float32)
    return agents


def duel_model(scenario, E, cap, seed=5, **cfg):
    scn, m = model(scenario, 'iqld', 'dqn', E, seed=seed, buffer_size=cap, dueling=1, **cfg)
    assert get_dueling(m) == 1 and m.layout.dueling
    m.set_agent_params(nontrivial(m.get_agent_params(), np.random.RandomState(seed + 100)))
    if m.target_update:
        m.sync_target()
    p = m.get_agent_params()
    assert all(np.abs(x['v_w']).max() > 0 and x['v_b'][0] != 0 and np.abs(x['q_b']).min() > 0 for x in p)
    return scn, m


def oracle_for(m, **over):
    """tests/iql_ext_oracle.py's oracle of the handle's own configuration: the options the model was made with (a one-step handle takes
    the stored tuples, return_steps = None), its parameters, batch, ring, reward scaling, clip and replay seed.  over: options to differ in."""
    from tests.iql_ext_oracle import ExtOracleIQL
    kw = dict(per=bool(m.prioritized_replay), alpha=m.per_alpha, eps=m.per_eps, target_update=m.target_update, double_q=bool(m.double_q),
              return_steps=m.return_steps if m.return_steps > 1 else None, batch_size=m.n_step, buffer_size=int(m.cfg['buffer_size']),
              gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'], reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'],
              replay_seed=m.replay_seed)
    kw.update(over)
    return ExtOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, **kw)


# ---- observations ----------------------------------------------------------------------------------------------------------------
def rand_obs(scn, E, rng):
    obs = np.zeros((E, scn.n_agent, scn.s_max), np.float32)
    for a, n in enumerate(scn.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


def kinks(o, obs_rows, a, thr=1e-6):
    """(layer-1 columns, any layer-2 unit) of agent a whose pre-activation is within thr of zero on the minibatch."""
    from oracle.iql_oracle import DT
    p = o.qs[a].p
    if 'fcw_w' not in p:
        return None, False
    S = torch.as_tensor(np.asarray(obs_rows), dtype=DT)
    nw = o.nw[a]
    z = [S[:, :nw] @ p['fcw_w'] + p['fcw_b']]
    if o.nt[a]:
        z.append(S[:, nw:] @ p['fct_w'] + p['fct_b'])
    z1 = torch.cat(z, 1)
    z2 = torch.relu(z1) @ p['fc0_w'] + p['fc0_b']
    return (z1.abs() < thr).any(0).numpy(), bool((z2.abs() < thr).any())


def rand_obs_off_the_kinks(scn, E, rng, o, thr=5e-6):
    """rand_obs, with every row re-drawn until no hidden unit of its agent's net (the oracle's CURRENT parameters) has a
    pre-activation within thr of zero: on such rows the float64 gradient is the gradient, not one of two subgradients, and a
    20 480-row minibatch (which meets ~ 4 such units per agent otherwise) can be compared tensor by tensor without exceptions."""
    from oracle.iql_oracle import DT
    obs = rand_obs(scn, E, rng)
    for a, n in enumerate(scn.n_s_ls):
        p, nw = o.qs[a].p, o.nw[a]
        if 'fcw_w' not in p:
            continue
        rows = np.arange(E)
        while rows.size:
            S = torch.as_tensor(obs[rows, a, :n].astype(np.float64), dtype=DT)
            z = [S[:, :nw] @ p['fcw_w'] + p['fcw_b']]
            if o.nt[a]:
                z.append(S[:, nw:] @ p['fct_w'] + p['fct_b'])
            z1 = torch.cat(z, 1)
            z2 = torch.relu(z1) @ p['fc0_w'] + p['fc0_b']
            bad = ((z1.abs() < thr).any(1) | (z2.abs() < thr).any(1)).numpy()
            rows = rows[bad]
            if rows.size:
                obs[rows, a, :n] = rng.rand(rows.size, n).astype(np.float32) * 2
    return obs


def gap_of(q):
    """The smallest top-two gap over the rows of q [rows, n_a] (inf for a single action)."""
    if q.shape[1] < 2:
        return np.inf
    top = np.sort(q, 1)
    return float((top[:, -1] - top[:, -2]).min())


def rand_obs_decided(scn, E, rng, o):
    """rand_obs with every row re-drawn until its agent's two best online values -- the combined ones of a dueling agent, ExtOracleQ.net --
    are at least GAP apart in float64: the greedy action and Double DQN's pick on such a row are the same in float32, so a* is compared
    on every row (the manner of rand_obs_off_the_kinks)."""
    from oracle.iql_oracle import DT
    obs = rand_obs(scn, E, rng)
    for a, n in enumerate(scn.n_s_ls):
        rows = np.arange(E)
        while rows.size:
            with torch.no_grad():
                q = o.qs[a].net(o.qs[a].p, torch.as_tensor(obs[rows, a, :n].astype(np.float64), dtype=DT)).numpy()
            if q.shape[1] < 2:
                break
            top = np.sort(q, 1)
            rows = rows[top[:, -1] - top[:, -2] < GAP]
            if rows.size:
                obs[rows, a, :n] = rng.rand(rows.size, n).astype(np.float32) * 2
    return obs


# ---- rings -----------------------------------------------------------------------------------------------------------------------
def fill(models, o, scn, E, cap, rng, draw_next=None, p_done=0.1, force_terminal=False):
    """test_replay_minibatch_gradient_and_adam's transitions into every model's rings (and the oracle's, unless None): past the capacity
    -- cap + 7 adds, so the newest slot w = 6 sits mid-ring -- except a ring of 100 slots or more, which takes 45: the size < cap branch.
    rng is consumed in one order whatever the options: the first observations, then per add the next observations, the actions agent by
    agent, the rewards, the done flags.  force_terminal: the fourth-newest transition is made terminal in every instance that would
    otherwise keep no terminal slot, so that EVERY ring has one to draw (no draw of rng is spent on it).
    -> (size, cum, rewards as stored [E][cap][A] float32, done [E][cap])."""
    A = scn.n_agent
    cfg = models[0].cfg
    n_add = cap + 7 if cap < 100 else 45
    draw = draw_next or (lambda: rand_obs(scn, E, rng))
    rews, dones = np.zeros((E, cap, A), np.float32), np.zeros((E, cap), bool)
    kept = np.ones(cap, bool)                      # slots that the adds after n_add - 4 do not overwrite
    for u in range(n_add - 3, n_add):
        kept[u % cap] = False
    obs = draw()
    for t in range(n_add):
        nobs = draw()
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, A) * 3.0 * cfg['reward_norm']
        done = (rng.rand(E) < p_done).astype(np.uint8)
        if force_terminal and t == n_add - 4:
            kept_t = kept.copy()
            kept_t[t % cap] = False
            done[~(dones & kept_t).any(1)] = 1
        for m in models:
            m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(),
                             torch.from_numpy(nobs).cuda(), torch.from_numpy(done).cuda())
        if o is not None:
            o.add_transition(obs, act, rew, nobs, done)
        r = rew / cfg['reward_norm'] if cfg['reward_norm'] else rew
        rews[:, t % cap] = (np.clip(r, -cfg['reward_clip'], cfg['reward_clip']) if cfg['reward_clip'] else r).astype(np.float32)
        dones[:, t % cap] = done.astype(bool)
        obs = nobs
    size = min(cap, n_add)
    assert not force_terminal or dones[:, :size].any(1).all()
    return size, n_add, rews, dones


def fill_one(m, scn, E, rng):
    """One more non-terminal transition into every ring of m."""
    obs, nobs = rand_obs(scn, E, rng), rand_obs(scn, E, rng)
    act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
    rew = -rng.rand(E, scn.n_agent) * m.cfg['reward_norm']
    m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(), torch.from_numpy(nobs).cuda(),
                     torch.zeros(E, dtype=torch.uint8, device='cuda'))


def draw_idx(rng, E, A, B, size):
    """A caller's draw [E][A][B] on the device: B distinct filled slots per ring."""
    return torch.from_numpy(np.stack([np.stack([rng.permutation(size)[:B] for _ in range(A)]) for _ in range(E)]).astype(np.int32)).cuda()


# ---- the handle's options and debug surface (include/tsc.h) ----------------------------------------------------------------------
def set_target(m, period, double_q):
    check(m._L.tsc_iql_set_target(m._h, period, double_q))


def set_per(m, enable, alpha=0.6, eps=0.01):
    check(m._L.tsc_iql_set_per(m._h, enable, alpha, eps))


def set_beta(m, beta):
    check(m._L.tsc_iql_set_per_beta(m._h, beta))


def set_dueling(m, enable):
    check(m._L.tsc_iql_set_dueling(m._h, enable))


def get_dueling(m):
    v = C.c_int32(-1)
    check(m._L.tsc_iql_get_dueling(m._h, C.byref(v)))
    return int(v.value)


def set_steps(m, n):
    check(m._L.tsc_iql_set_return_steps(m._h, n))


def get_steps(m):
    v = C.c_int32(-1)
    check(m._L.tsc_iql_get_return_steps(m._h, C.byref(v)))
    return int(v.value)


def targets(m):
    """-> (y, a*) [A][R] of the last step (tsc_iql_debug_targets)."""
    R = m.E * m.n_step
    y, astar = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.int32)
    check(m._L.tsc_iql_debug_targets(m._h, y.ctypes.data_as(C.c_void_p), astar.ctypes.data_as(C.c_void_p)))
    return y, astar


def per_debug(m):
    """-> (importance weights, |delta|) [A][R] of the last step (tsc_iql_debug_per)."""
    R = m.E * m.n_step
    w, td = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.float32)
    check(m._L.tsc_iql_debug_per(m._h, w.ctypes.data_as(C.c_void_p), td.ctypes.data_as(C.c_void_p)))
    return w, td


def nstep_debug(m):
    """-> (bootstrap slot [E][A][B], G, gamma^k, k [A][R]) of the last step (tsc_iql_debug_nstep)."""
    R = m.E * m.n_step
    slot = np.zeros((m.E, m.n_agent, m.n_step), np.int32)
    ret, disc, k = np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.float32), np.zeros((m.n_agent, R), np.int32)
    check(m._L.tsc_iql_debug_nstep(m._h, *[x.ctypes.data_as(C.c_void_p) for x in (slot, ret, disc, k)]))
    return slot, ret, disc, k


def batch(m):
    """-> the draw [E][A][B] of the last step (tsc_iql_debug_batch)."""
    idx = np.zeros((m.E, m.n_agent, m.n_step), np.int32)
    check(m._L.tsc_iql_debug_batch(m._h, idx.ctypes.data_as(C.c_void_p)))
    return idx


def grads_at(m, idx_dev, lr=1e-3):
    """One step on the caller's draw -> (flat gradient buffer, (loss, clip norm) [A][2]); applies Adam."""
    check(m._L.tsc_iql_compute_grads_at(m._h, C.c_void_p(idx_dev.data_ptr())))
    g = m.grad_tensor().cpu().numpy().copy()
    stats = np.zeros((m.n_agent, 2))
    check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(C.c_void_p)))
    return g, stats


def launches(name):
    """Launches counted under one profile id since the last reset."""
    from deeprl_signal_control_amd import _lib
    ms, cnt = C.c_double(), C.c_int64()
    _lib.check(_lib.lib().tsc_profile_read(_lib.profile_names().index(name), C.byref(ms), C.byref(cnt)))
    return int(cnt.value)


def reset_like(m, ref):
    """ref's parameters, zero Adam moments and step count, theta- = theta."""
    m.set_flat(ref.get_flat())
    z = np.zeros(m.n_param, np.float32)
    check(m._L.tsc_iql_set_opt_state(m._h, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0))
    if m.target_update:
        m.sync_target()


# ---- a target network that disagrees ---------------------------------------------------------------------------------------------
def disagreeing_target(m, o, seed=1234):
    """theta-: a second seeded initialisation, re-drawn per agent until its argmax differs from the online net's on a fifth of the
    next states in the agent's rings (an agent with two or three actions and a one-sided pair of nets would otherwise never
    exercise Double DQN); the test still asserts a disagreeing row among the SAMPLED ones."""
    from deeprl_signal_control_amd.iql import init_agent_params
    from oracle.iql_oracle import DT, q_net
    tp = init_agent_params(m.layout, np.random.RandomState(seed))
    for a, q in enumerate(o.qs):
        S1 = torch.as_tensor(np.asarray([t[3] for e in range(o.E) for t in o.rings[e][a].buffer]), dtype=DT)
        with torch.no_grad():
            on = q_net(q.p, S1, q.n_s, q.n_w).argmax(1)
            for trial in range(1, 40):
                cand = {k: torch.as_tensor(np.asarray(v), dtype=DT) for k, v in tp[a].items()}
                if (q_net(cand, S1, q.n_s, q.n_w).argmax(1) != on).double().mean() >= 0.2:
                    break
                tp[a] = init_agent_params(m.layout, np.random.RandomState(seed + trial))[a]
            else:
                pytest.fail('agent %d: no target initialisation disagrees with the online net' % a)
    return tp


def arm_disagreeing_target(m, o):
    """disagreeing_target into the handle and the oracle.  (On a dueling handle disagreeing_target compares the argmax of the advantage
    streams, which is the argmax of the combined values: V and the mean are common to a row's actions; so theta- keeps the advantage
    biases it was chosen with and only its value bias leaves zero.)"""
    tp = disagreeing_target(m, o)
    if 'v_b' in tp[0]:
        rng = np.random.RandomState(77)
        for p in tp:
            p['v_b'] = (rng.randn(1) * 0.3 - 0.4).astype(np.float32)
    m.set_target_flat(m.layout.pack(tp))
    o.set_target_params(m.layout.unpack(m.get_target_flat()))
    assert np.abs(m.get_target_flat() - m.get_flat()).max() > 0.01


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def compare_grads(m, o, g, og, idx, params_before, rows_before, what=''):
    """The gradient comparison of test_replay_minibatch_gradient_and_adam, every tensor of every agent (v_w / v_b of a dueling head
    included): |d| <= 2e-5 max|g| per tensor.  The kinks are those of the online net, at the parameters the gradient was taken at, on s, the
    SAMPLED slot's observation: first-layer columns on one are left out of fcw / fct, a second-layer unit on one leaves only the head's
    tensors to compare.  -> the agents that met a ReLU kink."""
    tol, kinked = 2e-5, set()
    for a in range(m.n_agent):
        q = o.qs[a]
        saved, q.p = q.p, params_before[a]
        cols, deep = kinks(o, [rows_before[a][e][s][0] for e in range(m.E) for s in idx[e, a]], a)
        q.p = saved
        if deep or (cols is not None and cols.any()):
            kinked.add(a)
        assert set(og[a]) == set(g[a]) and (not m.layout.dueling or ('v_w' in og[a] and 'v_b' in og[a]))
        for k, ref in og[a].items():
            if deep and k not in ('q_w', 'q_b', 'v_w', 'v_b'):
                continue
            got, scale = g[a][k], max(np.abs(ref).max(), 1e-9)
            err = np.abs(got - ref)
            if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                sel = cols[:m.layout.n_fc0] if k.startswith('fcw') else cols[m.layout.n_fc0:]
                err = err[..., ~sel] if err.ndim == 2 else err[~sel]
            assert err.size == 0 or err.max() <= tol * scale, '%s agent %d %s: %.2e' % (what, a, k, err.max() / scale)
    return kinked


def snapshot(o):
    """-> (params_before, rows_before) of compare_grads: the oracle's parameters and ring contents before its step."""
    return ([{k: v.clone() for k, v in q.p.items()} for q in o.qs],
            [[o.rings[e][a].buffer for e in range(o.E)] for a in range(o.A)])


def dead_columns_are_zero(m, flat_g):
    """columns n_a <= j < 7 of dWq and dbq of a dueling head: exactly 0."""
    lay = m.layout
    f = flat_g.reshape(lay.A, lay.stride)
    for a, na in enumerate(m.n_a_ls):
        Wq = f[a, lay.oWq:lay.obq].reshape(lay.H2, 8)
        assert (Wq[:, na:7] == 0).all() and (f[a, lay.obq + na:lay.obq + 7] == 0).all(), a
        assert np.abs(Wq[:, 7]).max() > 0 and f[a, lay.obq + 7] != 0 and np.abs(Wq[:, :na]).max() > 0


def check_targets(m, o, y, astar, gap_floor=GAP, ytol=None):
    """y and a* of every row of the last step against the oracle's; the test's own input conditions: no row with an undecided online
    argmax, and -- Double DQN -- a row on which the online pick is not the target's argmax, for every agent.  ytol(a): bound on |dy| per
    row, default the Q-value tolerance."""
    for a in range(m.n_agent):
        q = o.qs[a]
        dy = np.abs(y[a] - q.last_y)
        print('agent %d: max|dy| %.2e, smallest online gap %.2e' % (a, dy.max(), gap_of(q.last_q1_online)))
        assert gap_of(q.last_q1_online) >= gap_floor, 'agent %d: a sampled row with undecided online argmax remains' % a
        assert (dy <= (2e-5 if ytol is None else ytol(a))).all(), 'agent %d: y off by %.2e' % (a, dy.max())
        if m.double_q:
            np.testing.assert_array_equal(astar[a], q.last_astar)
            differ = q.last_astar != np.argmax(q.last_q1_target, 1)
            assert differ.any(), 'agent %d: the online argmax is the target argmax on every sampled row' % a
        else:
            assert (astar[a] == -1).all()


def check_weights(w, td, o, prio, size, idx, beta):
    """Importance weights and |delta| of the last step against the oracle's (tests/test_iql_per_gpu.py: float32 roundings of float64
    expressions of the device's own float32 priorities, rtol 1e-6; |delta| within the Q-value tolerance)."""
    from tests.iql_ext_oracle import per_weights
    E, A, B = idx.shape
    wr = w.reshape(A, E, B)
    assert (wr.max(2) == 1).all() and (w > 0).all() and w.min() < 0.5
    for e in range(E):
        for a in range(A):
            np.testing.assert_allclose(wr[a, e], per_weights(prio[e, a], size, idx[e, a], beta), rtol=1e-6, atol=0)
    np.testing.assert_allclose(w, o.last_w, rtol=1e-6, atol=0)
    print('max |d|delta|| %.2e' % np.abs(td - o.last_td).max())
    np.testing.assert_allclose(td, o.last_td, rtol=0, atol=2e-5)


def expected_after(before, qmax_before, idx, td, size, alpha, eps):
    """The priorities after the write-back of one step from the device's own |delta|: picks in order, the last pick of a slot stays."""
    E, A, B = idx.shape
    want, wmax = before.copy(), qmax_before.copy()
    hit = np.zeros(before.shape, bool)
    for e in range(E):
        for a in range(A):
            for i, s in enumerate(np.clip(idx[e, a], 0, size - 1)):
                v = np.float32((np.float64(td[a, e * B + i]) + eps) ** alpha)
                want[e, a, s], hit[e, a, s] = v, True
                wmax[e, a] = max(wmax[e, a], v)
    return want, wmax, hit


def check_write_back(m, before, qmax_before, idx, td, size):
    """The priorities of m after a step against expected_after: written slots rtol 1e-6, the others bit for bit."""
    after, qmax = m.get_priorities()
    want, wmax, hit = expected_after(before, qmax_before, idx, td, size, m.per_alpha, m.per_eps)
    np.testing.assert_allclose(after[hit], want[hit], rtol=1e-6, atol=0)
    np.testing.assert_array_equal(after[~hit], before[~hit])
    np.testing.assert_allclose(qmax, wmax, rtol=1e-6, atol=0)
    return hit


def random_priorities(m, size, rng):
    """Random priorities over four decades with a fifth of the filled slots at 0; ring (0, 0) keeps its whole mass in its last filled
    slot, ring (0, 1) in its first; the slots behind `size` hold a large value that must never be drawn."""
    prio, qmax = m.get_priorities()
    cap = prio.shape[2]
    q = (10.0 ** rng.uniform(-2, 2, prio.shape)).astype(np.float32)
    q[rng.rand(*prio.shape) < 0.2] = 0
    q[0, 0, :] = 0; q[0, 0, size - 1] = 3.5
    q[0, 1, :] = 0; q[0, 1, 0] = 0.25
    dead = q[:, :, :size].max(2) == 0
    q[dead, 0] = 1.0
    q[:, :, size:] = 1e6
    assert cap >= size
    m.set_priorities(q, np.maximum(qmax, q[:, :, :size].max(2)))
    got, _ = m.get_priorities()
    np.testing.assert_array_equal(got, q)
    return q


def positive_priorities(m, size, rng):
    """Random priorities over four decades on the filled slots, none of them 0: with a caller's draw a slot of priority 0 takes the ring's
    largest weight on the device, which the oracle's formula does not restate (no draw of the library's own can pick such a slot)."""
    prio, qmax = m.get_priorities()
    q = (10.0 ** rng.uniform(-2, 2, prio.shape)).astype(np.float32)
    q[:, :, size:] = 0
    m.set_priorities(q, np.maximum(qmax, q.max(2)))


def sync_oracle(m, o):
    """Hand the oracle the device's parameters and Adam moments: every step is then checked from the SAME state (entries whose gradient
    is rounding noise legitimately step the other way, and would otherwise compound)."""
    hm, hv, ht = m.get_opt_state()
    for a, (pp, mm, vv) in enumerate(zip(m.get_agent_params(), m.layout.unpack(hm), m.layout.unpack(hv))):
        for k in o.qs[a].p:
            o.qs[a].p[k] = torch.as_tensor(pp[k].astype(np.float64))
            o.qs[a].m[k] = torch.as_tensor(mm[k].astype(np.float64))
            o.qs[a].v[k] = torch.as_tensor(vv[k].astype(np.float64))
    return ht


# ---- test bodies that more than one module runs (the built-in scenarios and the synthetic layouts of tests/test_layouts_gpu.py) ----
def forward_and_act(scn, m, o, E, rng, steps=3, qtol=2e-5):
    """Q values, the greedy action and the epsilon-greedy action on the documented uniforms against the oracle.  qtol: bound on |dQ|,
    or a function of an agent's oracle values (layouts whose values leave the reference's range, tests/test_layouts_gpu.py)."""
    tol = qtol if callable(qtol) else (lambda oq: qtol)
    A = scn.n_agent
    for t in range(steps):
        obs = rand_obs(scn, E, rng)
        act, q = m.forward(torch.from_numpy(obs).cuda())                       # mode 'act': argmax
        act, q = act.cpu().numpy(), q.cpu().numpy()
        oq = o.forward(obs)
        for a in range(A):
            np.testing.assert_allclose(q[:, a, :scn.n_a_ls[a]], oq[a], atol=tol(oq[a]))
            assert np.all(q[:, a, scn.n_a_ls[a]:] == 0)
            np.testing.assert_array_equal(act[:, a], np.argmax(q[:, a, :scn.n_a_ls[a]], 1))
        explored(scn, m, obs, E)


def explored(scn, m, obs, E):
    """One mode='explore' forward: every action is the oracle's epsilon-greedy rule on the device's own Q values and the documented uniforms."""
    from oracle.iql_oracle import act_epsilon_greedy
    from oracle.nets_oracle import sample_uniform
    A = scn.n_agent
    eps_before = m.eps_scheduler.n
    act, q = m.forward(torch.from_numpy(obs).cuda(), mode='explore')
    eps = max(m.cfg['epsilon_min'], m.cfg['epsilon_init'] * (1 - (eps_before + 1) / (10000 * m.cfg['epsilon_ratio'])))
    act, q = act.cpu().numpy(), q.cpu().numpy()
    for e in range(E):
        for a in range(A):
            u0 = sample_uniform(m.sample_seed, m.act_step - 1, 2 * (e * A + a))
            u1 = sample_uniform(m.sample_seed, m.act_step - 1, 2 * (e * A + a) + 1)
            assert act[e, a] == act_epsilon_greedy(q[e, a, :scn.n_a_ls[a]], eps, u0, u1)


def replay_vs_oracle(scn, m, o, E, cap, rng, steps=None):
    """Fill the rings past their capacity, then minibatch steps (three, two at E >= 100, or `steps`): replay indices exact, TD loss /
    gradient / clip norm / Adam-updated parameters against the oracle."""
    A, B = scn.n_agent, m.n_step
    n_add = cap + (7 if E < 100 else 3) if cap < 100 else 45
    # big batches: observations off the ReLU kinks of the initial nets, so that the first step is compared without exceptions
    draw = (lambda: rand_obs_off_the_kinks(scn, E, rng, o)) if E >= 100 else (lambda: rand_obs(scn, E, rng))
    obs = draw()
    assert m.backward() is None                                              # fewer than a batch: no update (models.py:321-322)
    for t in range(n_add):
        nobs = draw()
        act = np.stack([rng.randint(0, n, E) for n in scn.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, A) * 3.0 * m.cfg['reward_norm']
        done = (rng.rand(E) < 0.1).astype(np.uint8)
        m.add_transition(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(),
                         torch.from_numpy(nobs).cuda(), torch.from_numpy(done).cuda())
        o.add_transition(obs, act, rew, nobs, done)
        obs = nobs
    assert m.replay_size() == (min(cap, n_add), n_add)
    lr = 1e-3
    for step in range((3 if E < 100 else 2) if steps is None else steps):
        before = m.get_flat().reshape(A, -1).copy()
        check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
        m.update_step += 1
        idx = batch(m)
        g = m.layout.unpack(m.grad_tensor().cpu().numpy())
        flat_g = m.grad_tensor().cpu().numpy().reshape(A, -1).copy()
        stats = np.zeros((A, 2))
        check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(C.c_void_p)))
        obefore = m.layout.pack(o.agent_params()).reshape(A, -1)
        params_before, rows_before = snapshot(o)
        losses, norms, og = o.minibatch_step(lr)
        np.testing.assert_array_equal(idx, o.last_idx)
        assert all(len(set(idx[e, a])) == B and idx[e, a].max() < min(cap, n_add) for e in range(E) for a in range(A))
        # agents with a hidden unit on a ReLU kink in this minibatch (enters Adam's moments)
        kinked = compare_grads(m, o, g, og, idx, params_before, rows_before, 'step %d' % step)
        if E >= 100 and step == 0:
            assert not kinked, 'agents %s: a row of the first minibatch sits on a ReLU kink' % sorted(kinked)
        np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
        # Adam: this step's parameter change.  Adam's first steps move a weight by ~lr * sign-like(m / sqrt(v)): entries
        # whose gradient is well above the gradient tolerance must move alike; entries whose gradient is itself
        # rounding noise may move either way, by at most ~lr
        after = m.get_flat().reshape(A, -1)
        oflat = m.layout.pack(o.agent_params()).reshape(A, -1)
        d_hip, d_orc = after - before, oflat - obefore
        real = np.abs(flat_g) > 1e-2 * np.abs(flat_g).max(1, keepdims=True)
        real[sorted(kinked)] = False
        assert step > 0 or real.any()
        if real.any():
            assert np.abs(d_hip - d_orc)[real].max() <= 2e-6, np.abs(d_hip - d_orc)[real].max()
        assert np.abs(d_hip).max() <= 1.01 * lr and np.abs(d_hip - d_orc).max() <= 2.02 * lr
        if step == 0:
            assert np.array_equal(after == before, flat_g == 0)                  # structural zeros never move
        assert sync_oracle(m, o) == step + 1 == o.qs[0].t


def duel_forward_vs_oracle(scn, m, o, E, rng):
    """forward_and_act on a dueling handle: the combined values, and the greedy action against the ORACLE's argmax too (rows decided by GAP)."""
    A = scn.n_agent
    for t in range(2):
        obs = rand_obs_decided(scn, E, rng, o)
        act, q = m.forward(torch.from_numpy(obs).cuda())
        act, q = act.cpu().numpy(), q.cpu().numpy()
        oq = o.forward(obs)
        worst = 0.0
        for a in range(A):
            na = scn.n_a_ls[a]
            worst = max(worst, np.abs(q[:, a, :na] - oq[a]).max())
            np.testing.assert_allclose(q[:, a, :na], oq[a], rtol=0, atol=2e-5)
            assert np.all(q[:, a, na:] == 0)
            np.testing.assert_array_equal(act[:, a], np.argmax(q[:, a, :na], 1))
            assert gap_of(oq[a]) >= GAP
            np.testing.assert_array_equal(act[:, a], np.argmax(oq[a], 1))
        print('max |dQ| %.2e' % worst)
        explored(scn, m, obs, E)


def targets_and_gradient_vs_oracle(scn, m, o, E, cap, rng):
    """One step of the library's own draw with theta- != theta where the handle has a target network: y and a* of every sampled row, loss,
    clip norm and every gradient tensor -> the flat gradient buffer of the step (the caller may look at single columns)."""
    A = scn.n_agent
    fill([m], o, scn, E, cap, rng, draw_next=lambda: rand_obs_decided(scn, E, rng, o))
    if m.target_update:
        arm_disagreeing_target(m, o)
    params_before, rows_before = snapshot(o)
    check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = batch(m)
    flat_g = m.grad_tensor().cpu().numpy().copy()
    g = m.layout.unpack(flat_g)
    y, astar = targets(m)                                         # (answers on a dueling handle without a target network too)
    stats = np.zeros((A, 2))
    check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3)
    np.testing.assert_array_equal(idx, o.last_idx)
    check_targets(m, o, y, astar)
    compare_grads(m, o, g, og, idx, params_before, rows_before)
    if m.layout.dueling:
        dead_columns_are_zero(m, flat_g)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
    return flat_g


def per_step_vs_oracle(scn, m, E, cap, rng, beta):
    """One prioritized-replay step of the library's own draw on random priorities: weights, |delta|, loss, clip norm, every gradient tensor."""
    o = oracle_for(m)
    A = scn.n_agent
    size = fill([m], o, scn, E, cap, rng, draw_next=lambda: rand_obs_decided(scn, E, rng, o))[0]
    if m.target_update:
        arm_disagreeing_target(m, o)
    q = random_priorities(m, size, rng)
    o.prio[:], o.qmax[:] = q, m.get_priorities()[1]
    set_beta(m, beta)
    params_before, rows_before = snapshot(o)
    check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
    m.update_step += 1
    idx = batch(m)
    g = m.layout.unpack(m.grad_tensor().cpu().numpy())
    w, td = per_debug(m)
    stats = np.zeros((A, 2))
    check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 1.0, stats.ctypes.data_as(C.c_void_p)))
    losses, norms, og = o.minibatch_step(1e-3, beta=beta, idx_given=idx)        # the device's draw (check 2 is test_draw's)
    check_weights(w, td, o, q, size, idx, beta)
    compare_grads(m, o, g, og, idx, params_before, rows_before)
    np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)
