"""Host-side conditions of tests/test_layouts_gpu.py, on the oracles alone (no GPU, no library): for every layout of tests/layouts.py
and the seeds of its table, the very inputs of the GPU module go through OracleA2C / OracleIQL and through their float32 restatement
(the same code in torch float32 on the CPU, layouts.f32_oracle_class), and

  * at most 4 hidden columns of a tower fall under the ReLU-kink exception of _grad_err / iql_harness.kinks in any round (and no second-layer
    unit of a Q-net sits on a kink: that would take every tensor below the head out of the comparison);
  * every action of every agent has an oracle probability in (1e-4, 1 - 1e-4) on some sample: no head is saturated, no gradient
    vacuous (a saturated softmax passes any kernel);
  * the second-round gradients of the float32 restatement, whose parameters carry the first update's float32 rounding exactly as the
    kernel's do, stay inside the 2e-4 allowance of the second round against float64 -- the allowance is wide enough for a correct
    float32 evaluation of these layouts, so a GPU failure there is the kernel's;
  * the float32 restatement's values stay inside the bound the GPU module uses for v and Q, 2e-5 max(1, max|oracle value|): layouts
    with up to 68 inputs in [0, 2) produce larger values than the reference's ranges do.

The seeds of tests/layouts.py were chosen so that this passes; the GPU module imports the same table."""
import functools

import numpy as np
import pytest
import torch

from tests import layouts as LY


def value_bound(ov):
    """The bound on |dv| / |dQ| of a layout: 2e-5 max(1, max|oracle value|) (tests/test_layouts_gpu.py uses the same function)."""
    return 2e-5 * max(1.0, float(np.abs(ov).max()))


@functools.lru_cache(maxsize=None)
def _towers(name, policy):
    """The weights VecA2C(seed=SEEDS[name]) starts from, of every agent (one stream of draws over all of them) -> (towers, n_f)."""
    from deeprl_signal_control_amd.agents import A2C_DEFAULTS, init_tower_params
    spec = LY.spec_of(name)
    lay, c = spec['layout'], dict(A2C_DEFAULTS, **spec['cfg'])
    ma = spec['agent'] == 'ma2c'
    n_f = lay.n_f_ls if ma else [0] * lay.n_agent
    n_fc = (c['num_fw'], c['num_fp'] if ma else 0, c['num_ft'] if max(lay.n_w_ls) > 0 else 0)
    return init_tower_params(lay.n_wave_ls, lay.n_w_ls, n_f, lay.n_a_ls, n_fc, 64, policy, np.random.RandomState(LY.seed_of(name))), n_f


def _a2c_pair(name, policy, E, sel=None, regime=None):
    """The float64 oracle and its float32 restatement on a layout's agents, or on the agents `sel` of it; regime: a value regime of
    tests/layouts.py REGIMES on the initial weights."""
    from deeprl_signal_control_amd.agents import A2C_DEFAULTS
    from oracle.nets_oracle import OracleA2C
    spec = LY.spec_of(name)
    lay, c = spec['layout'], dict(A2C_DEFAULTS, **spec['cfg'])
    towers, n_f = _towers(name, policy)
    if regime is not None:
        towers = LY.apply_regime(towers, regime, lay)
    kw = dict(gamma=c['gamma'], reward_norm=c['reward_norm'], reward_clip=c['reward_clip'], value_coef=c['value_coef'],
              max_grad_norm=c['max_grad_norm'])
    ids = list(range(lay.n_agent)) if sel is None else list(sel)
    args = ([towers[2 * a + k] for a in ids for k in (0, 1)],) + tuple([ls[a] for a in ids] for ls in (lay.n_wave_ls, lay.n_w_ls, n_f, lay.n_a_ls))
    o64 = OracleA2C(*args, E, **kw)
    o32 = LY.f32_oracle_class(OracleA2C)(*args, E, **kw)
    assert o32.p[0]['fcw_w'].dtype == torch.float32 and o64.p[0]['fcw_w'].dtype == torch.float64
    return lay, c, o64, o32


def _open_heads(lay, pis):
    """Every action of every agent: an oracle probability in (1e-4, 1 - 1e-4) on some sample of pis (list over steps of list[A])."""
    for a in range(len(pis[0])):                                         # (the agents the oracle holds: all, or a pick)
        p = np.concatenate([step[a] for step in pis], 0)
        ok = ((p > 1e-4) & (p < 1 - 1e-4)).any(0)
        assert ok.all(), 'agent %d: actions %s are saturated on every sample' % (a, np.nonzero(~ok)[0])


A2C_CASES = [(n, p) for n in LY.A2C_LAYOUTS for p in ('lstm', 'fc')]


@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_forward_conditions(name, policy):
    E = LY.A2C_FORWARD_E
    lay, c, o64, o32 = _a2c_pair(name, policy, E)
    steps, boot = LY.forward_inputs(lay, E, LY.A2C_FORWARD_STEPS, np.random.RandomState(LY.data_seed(name, E)))
    pis, worst, vmax = [], 0.0, 0.0
    for obs, done in steps:
        pi, v = o64.forward(obs, done, 'pv')
        pi32, v32 = o32.forward(obs, done, 'pv')
        pis.append(pi)
        assert np.abs(v32 - v).max() <= value_bound(v)
        assert max(np.abs(a - b).max() for a, b in zip(pi, pi32)) <= 2e-5
        worst, vmax = max(worst, np.abs(v32 - v).max()), max(vmax, np.abs(v).max())
    _, vb = o64.forward(boot, np.zeros(E), 'v')
    _, vb32 = o32.forward(boot, np.zeros(E), 'v')
    assert np.abs(vb32 - vb).max() <= value_bound(vb)
    print('%s %s: max|v| %.2f, float32 restatement |dv| %.1e (bound %.1e)' % (name, policy, vmax, worst, 2e-5 * max(1.0, vmax)))
    _open_heads(lay, pis)


def _update_conditions(name, policy, E, T, rounds=2, terminal=False, p_done=0.1, sel=None, max_kink=4, zero=()):
    """The oracle-only conditions of one update case of the GPU module, on its very rollouts -> worst float32-restatement error per round.
    zero: the tensors whose gradient must be exactly zero in this case (every other one must not be)."""
    from tests.test_model_gpu import _grad_err
    lay, c, o64, o32 = _a2c_pair(name, policy, E, sel)
    rng = np.random.RandomState(LY.data_seed(name, E, T))
    pis, worsts, kinks = [], [], 0
    for it in range(rounds):
        obs, done, p = LY.fill_host(lay, [o64, o32], E, T, rng, c['reward_norm'], p_done=p_done, terminal=terminal and it == 0, sel=sel)
        pis += p
        if sel is not None:
            obs = obs[:, sel]
        _, Rb = o64.forward(obs, np.zeros(E), 'v')
        o32.forward(obs, np.zeros(E), 'v')
        Rb = Rb.astype(np.float32)
        g64, _ = o64.compute_grads(Rb, 0.01)
        g32, _ = o32.compute_grads(Rb, 0.01)
        np.testing.assert_array_equal(o64.Rs, o32.Rs)
        worst = 0.0
        for t, kc in enumerate(o64.kink_cols):
            n_kink = sum(int(cols.sum()) for cols in kc.values())
            kinks = max(kinks, n_kink)
            assert n_kink <= max_kink, 'round %d tower %d: %d hidden columns on a ReLU kink' % (it, t, n_kink)
            for k, og in g64[t].items():
                if k in zero:
                    assert float(og.abs().max()) == 0 and float(g32[t][k].abs().max()) == 0, (it, t, k)
                    continue
                assert float(og.abs().max()) > 0, 'round %d tower %d %s: the oracle gradient is zero' % (it, t, k)
                err = _grad_err(o64, t, k, g32[t][k].double().numpy(), og.numpy())
                worst = max(worst, err)
                assert err <= (2e-5 if it == 0 else 2e-4), 'round %d tower %d %s: float32 restatement |dg| / max|g| = %.2e' % (it, t, k, err)
        print('%s %s E=%d T=%d round %d: float32 restatement worst |dg| / max|g| %.1e, at most %d kink columns' % (name, policy, E, T, it, worst, kinks))
        worsts.append(worst)
        o64.apply_grads(g64, 5e-4)
        o32.apply_grads(g32, 5e-4)
    _open_heads(lay, pis)
    return worsts


@pytest.mark.parametrize('E,T', LY.A2C_BATCHES)
@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_update_conditions(name, policy, E, T):
    _update_conditions(name, policy, E, T)


def _iql_pair(name, regime=None):
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, QParamLayout, init_agent_params
    from oracle.iql_oracle import OracleIQL
    spec = LY.IQL_LAYOUTS[name]
    lay, c = spec['layout'], dict(IQL_DEFAULTS, **spec['cfg'])
    ql = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, spec['model_type'], c['num_fc'], c['num_h'])
    params = init_agent_params(ql, np.random.RandomState(LY.SEEDS[name]))
    if regime is not None:                                                # a Q-learner regime of tests/layouts.py apply_iql_regime
        params = LY.apply_iql_regime(params, regime, name)
    kw = dict(batch_size=20, buffer_size=LY.IQL_CAP, gamma=c['gamma'], reward_norm=LY.IQL_REWARD_NORM, reward_clip=c['reward_clip'],
              max_grad_norm=c['max_grad_norm'], replay_seed=LY.SEEDS[name] ^ 0x5DEECE66D)
    o64 = OracleIQL(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, LY.IQL_E, **kw)
    o32 = LY.f32_oracle_class(OracleIQL)(params, lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, LY.IQL_E, **kw)
    return lay, o64, o32


@pytest.mark.parametrize('name', list(LY.IQL_LAYOUTS))
def test_iql_conditions(name):
    from tests.iql_harness import kinks
    lay, o64, o32 = _iql_pair(name)
    E, A = LY.IQL_E, lay.n_agent
    rng = np.random.RandomState(LY.data_seed(name, E))
    qmax, worst = 0.0, 0.0
    for t in range(3):                                                  # forward_and_act's observations
        obs = LY.rand_obs(lay, E, rng)
        for q, q32 in zip(o64.forward(obs), o32.forward(obs)):
            assert np.abs(q32 - q).max() <= value_bound(q)
            qmax, worst = max(qmax, np.abs(q).max()), max(worst, np.abs(q32 - q).max())
    print('%s: max|Q| %.2f, float32 restatement |dQ| %.1e (bound %.1e)' % (name, qmax, worst, 2e-5 * max(1.0, qmax)))
    rng = np.random.RandomState(LY.data_seed(name, E, LY.IQL_CAP))
    for tr in LY.iql_transitions(lay, E, LY.IQL_CAP, rng, LY.IQL_REWARD_NORM):
        o64.add_transition(*tr)
        o32.add_transition(*tr)
    for step in range(LY.IQL_STEPS):
        rows = [[o64.rings[e][a].buffer for e in range(E)] for a in range(A)]
        before = [{k: v.clone() for k, v in q.p.items()} for q in o64.qs]
        _, _, g64 = o64.minibatch_step(1e-3)
        _, _, g32 = o32.minibatch_step(1e-3)
        np.testing.assert_array_equal(o64.last_idx, o32.last_idx)
        n_deep = 0
        for a in range(A):
            saved, o64.qs[a].p = o64.qs[a].p, before[a]
            cols, deep = kinks(o64, [rows[a][e][s][0] for e in range(E) for s in o64.last_idx[e, a]], a)
            o64.qs[a].p = saved
            if A >= 100 and deep:
                # 130 agents x 100 sampled rows x 64 second-layer units = 832 000 pre-activations per step, of spread ~0.5: the
                # window of kinks(), |z| < 1e-6, holds one or two of them on average whatever the seed (ten seeds tried: none
                # without).  The harness then compares that agent's head tensors only (compare_grads); the condition here is that
                # this happens to at most 4 of the 130 agents per step (a Poisson count of mean 1.3 exceeds 4 once in a hundred
                # draws), so that all but a few replicas of the six agent shapes are compared in full.
                n_deep += 1
                assert n_deep <= 4, 'step %d: more than 4 agents with a second-layer unit on a ReLU kink' % step
            else:
                assert not deep, 'step %d agent %d: a second-layer unit on a ReLU kink' % (step, a)
            assert cols is None or cols.sum() <= 4, 'step %d agent %d: %d first-layer columns on a ReLU kink' % (step, a, cols.sum())
            for k, ref in g64[a].items():
                if deep and k not in ('q_w', 'q_b', 'v_w', 'v_b'):      # what compare_grads leaves out for such an agent, no more
                    continue
                err, scale = np.abs(g32[a][k] - ref), max(np.abs(ref).max(), 1e-9)
                assert np.abs(ref).max() > 0, (step, a, k)
                if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                    n0 = before[a]['fcw_b'].shape[0]
                    sel = cols[:n0] if k.startswith('fcw') else cols[n0:]
                    err = err[..., ~sel] if err.ndim == 2 else err[~sel]
                assert err.size == 0 or err.max() <= 2e-5 * scale, 'step %d agent %d %s: float32 restatement %.2e' % (step, a, k, err.max() / scale)
        for q64, q32 in zip(o64.qs, o32.qs):        # the next step starts from one state on both sides, as on the GPU
            for k in q64.p:
                q32.p[k], q32.m[k], q32.v[k] = q64.p[k].float(), q64.m[k].float(), q64.v[k].float()


def test_ppo_head8_conditions():
    """The K = 3 case of the GPU module on head8 (MA2C, LSTM): the clip branch is exercised and few samples sit on a clip bound
    (tests/ppo_oracle.py k3_conditions), on the oracle alone."""
    from tests.ppo_oracle import K3_REWARD_NORM, fill, k3_conditions, make_oracle
    spec = LY.A2C_LAYOUTS['head8']
    E, T, seed, rseed, lr = LY.PPO_HEAD8
    o = make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=dict(spec['cfg'], reward_norm=K3_REWARD_NORM), layout=spec['layout'])
    o.reset()
    obs, _ = fill(spec['layout'], o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM)
    _, Rb = o.forward(obs, np.zeros(E), 'v')
    for k in range(3):
        g, _ = o.compute_grads(Rb.astype(np.float32), 0.01, epoch=k, slack=False)
        clip, amb = k3_conditions(o, k)
        print('head8 epoch %d: clipped share %.3f, ambiguous %.4f' % (k, clip, amb))
        o.apply_grads(g, lr, end_of_rollout=(k == 2))


def test_layout_tables_are_consistent():
    for name, spec in LY.A2C_LAYOUTS.items():
        lay = spec['layout']
        assert 3 <= lay.n_agent <= 6 and lay.a_max <= 8 and spec['H'] % 4 == 0, name
        if spec['agent'] == 'ma2c':
            assert min(lay.n_f_ls) >= 1, name
        else:
            assert max(lay.n_f_ls) == 0, name
    assert LY.A2C_REFUSED['H'] % 4 != 0
    for name, spec in LY.IQL_LAYOUTS.items():
        lay = spec['layout']
        fits = max(lay.n_w_ls) == 0 or (max(lay.n_wave_ls) <= 32 and max(lay.n_w_ls) <= 16)
        want = spec['model_type'] == 'dqn' and spec['cfg'] == dict(num_fc=128, num_h=64) and lay.s_max <= 48 and fits
        assert spec['fused'] == want, name
    assert set(LY.SEEDS) == set(LY.A2C_LAYOUTS) | set(LY.IQL_LAYOUTS)


# ---- the agent-count, row-split and time axes ----------------------------------------------------------------------------------------
def test_schedule_restatements_agree_with_a_walk_of_the_loops():
    """dwxh_schedule / w1_schedule against the kernels' loops walked one sub-chunk at a time, for every R up to 400: the closed forms
    count what the loops run, every row of the split lies in exactly one sub-chunk, and no Plain sub-chunk reaches past the split --
    neither with its own rows nor with the A rows of sub-chunk c + 8 it stages (dwxh) or the successor chunk it fetches (dx1w1)."""
    for R in range(1, 401):
        c = full = 0
        while 16 * (c + 9) <= R:                                        # dwxh_kernel: for (; KC * (c + 9) <= R; c += 4)
            assert 16 * (c + 3 + 5 + 1) <= R                            # sub(Plain, c + 3) fetches the A rows of sub-chunk c + 8 unclamped
            c, full = c + 4, full + 1
        tail = 0
        while 16 * c < R:                                               # for (; KC * c < R; ++c)
            c, tail = c + 1, tail + 1
        assert (full, tail, R - 16 * (c - 1)) == LY.dwxh_schedule(R) and 16 * (c - 1) < R <= 16 * c
        row = plain = 0
        while row + 64 <= R:                                            # dx1w1_kernel2: for (; row + 2 * kW1Chunk <= n1; ...)
            row, plain = row + 32, plain + 1
        clamp = 0
        while row < R:
            row, clamp = row + 32, clamp + 1
        assert (plain, clamp, R - (row - 32)) == LY.w1_schedule(R) and row - 32 < R <= row and clamp in (1, 2)
    assert LY.dwxh_schedule(0) == LY.w1_schedule(0) == (0, 0, 0)


def test_rows_cover_the_schedules():
    """What the row sweep is for, stated by the restated loops: on the 65-agent layouts a split is the whole batch (s_upd = 1)."""
    assert all(LY.upd_splits(LY.A2C_COUNT_LAYOUTS[n]['layout'].n_agent) == 1 for n in ['many65'] + LY.ROW_WIDTHS)
    Rs = [E * T for E, T in LY.ROWS]
    assert max(Rs) <= 300 and len(set(Rs)) == len(Rs)
    dw, w1 = [LY.dwxh_schedule(R) for R in Rs], [LY.w1_schedule(R) for R in Rs]
    assert {min(f, 2) for f, _, _ in dw} == {0, 1, 2}
    assert {t for f, t, _ in dw if f >= 1} >= {5, 6, 7, 8, 9}           # every tail a full interval can leave behind
    assert {t for f, t, _ in dw if f == 0} >= {1, 2, 3, 4, 5, 6, 7, 8}
    assert {last for _, _, last in dw} >= {1, 2, 15, 16}
    assert {last for f, _, last in dw if f >= 1} >= {2, 15, 16} and any(last % 2 for f, _, last in dw if f >= 1)
    assert {min(p, 2) for p, _, _ in w1} == {0, 1, 2}
    after_plain = {last for p, _, last in w1 if p >= 1}
    assert 1 in after_plain and 16 in after_plain and 32 in after_plain
    assert any(1 < x < 16 for x in after_plain) and any(16 < x < 32 for x in after_plain)
    assert any(E % 16 for E, T in LY.ROWS if E * T in (130, 195, 255))   # ragged BPTT tiles too
    for sub in (LY.ROWS_REDUCED, LY.ROWS_FUSED, [LY.PPO_ROWS[:2]]):
        assert set(sub) <= set(LY.ROWS)
    red = [LY.dwxh_schedule(E * T) for E, T in LY.ROWS_REDUCED]
    assert {t for f, t, _ in red if f >= 1} >= {6, 8, 9} and any(f == 0 for f, _, _ in red) and {1, 2, 15} <= {last for _, _, last in red}
    for E, T in LY.ROWS_FUSED + [LY.PPO_ROWS[:2]]:                      # a full interval and a ragged tail
        f, t, last = LY.dwxh_schedule(E * T)
        assert f >= 1 and last < 16
    # many64: two splits, the boundary off the 16-row grid, a shorter last split, a full interval in each dwxh split
    assert LY.upd_splits(64) == 2 and LY.upd_splits(65) == 1
    for E, T in LY.ROWS_64:
        r_dw, r_w1 = LY.split_R(E * T, 2, LY.DWXH_Q), LY.split_R(E * T, 2, LY.W1_Q)
        assert sum(r_dw) == sum(r_w1) == E * T and r_dw[0] % 16 and r_dw[1] < r_dw[0] and r_w1[1] < r_w1[0]
        assert all(LY.dwxh_schedule(R)[0] >= 1 for R in r_dw)
    assert LY.split_R(297, 2, LY.DWXH_Q) == [150, 147] and LY.split_R(297, 2, LY.W1_Q) == [160, 137]


def test_agent_counts_sit_on_the_plan_edges():
    C_ = LY.A2C_COUNT_LAYOUTS
    A = {n: C_[n]['layout'].n_agent for n in C_}
    assert [LY.upd_splits(A[n]) for n in ('solo', 'many64', 'many65', 'many130')] == [128, 2, 1, 1] and 256 // (2 * A['many130']) == 0
    assert LY.fwd_splits(64, 32) == 1 and LY.fwd_splits(64, 33) == 2 and LY.fwd_splits(1, 37) == 2 and LY.fwd_splits(65, 1024) == 1
    # solo: at the batches of the GPU module nearly every one of the 128 splits is empty -- at least 100 of them in dx1w1 / fc_bwd
    # (32-row quantum) at both batches and in dwxh (2-row quantum) at N = 30; dwxh at N = 259 runs 65 splits of 4 rows and 63 empty ones
    empty = {(E * T, q): sum(1 for r in LY.split_R(E * T, 128, q) if r == 0) for E, T in LY.A2C_BATCHES for q in (LY.DWXH_Q, LY.W1_Q)}
    assert all(sum(LY.split_R(N, 128, q)) == N for N, q in empty)
    assert empty == {(30, 2): 113, (30, 32): 127, (259, 2): 63, (259, 32): 119}
    assert LY.head_slices(A['many130'], 10 ** 6) == 16 and LY.head_slices(1, 30) == 2 and LY.head_slices(65, 259) == 17
    # the workspace edge: s_upd 2 A dwxh_ws_floats(224) <= 48 Mi floats holds at 340 agents and fails at 341
    assert (A['ws_edge_340'], A['ws_edge_341']) == (340, 341) and C_['ws_edge_340']['H'] == C_['ws_edge_341']['H'] == 224
    assert LY.upd_splits(340) * 2 * 340 * LY.dwxh_ws_floats(224) <= 48 << 20 < LY.upd_splits(341) * 2 * 341 * LY.dwxh_ws_floats(224)
    for n, spec in C_.items():
        assert spec['route']['lstm'][1] == int(LY.dwxh_fits(A[n], spec['H'])), n
        assert LY.dwxh_fits(A[n], spec['H']) == (n != 'ws_edge_341')
        lay = spec['layout']
        assert all(lay.agents[i] != lay.agents[i + 1] for i in range(lay.n_agent - 1)), n      # neighbouring agents differ
        sel = LY.pick(lay.n_agent)
        assert sel[0] == 0 and sel[-1] == lay.n_agent - 1 and (lay.n_agent <= 128 or 128 in sel) and len(sel) == min(lay.n_agent, 4 + (lay.n_agent > 128))
    # the other widths' edges (INTEGRATION.md "Supported layouts"): the last agent count with dwxh and the first without
    assert [max(a for a in range(129, 600) if LY.dwxh_fits(a, H)) for H in (128, 160, 192, 224)] == [509, 436, 382, 340]


COUNT_CASES = LY.count_cases()


def _zero_tensors(policy, T, p_done):
    """dWh = h_prev^T dZ is exactly zero where every step's h_prev is masked: done after every step, and T = 1 (a window's only
    step follows the reset in the first round and the terminal step that ends the first round in the second)."""
    return ('lstm_wh',) if policy == 'lstm' and (T == 1 or p_done == 1.0) else ()


@pytest.mark.parametrize('group,name,policy,E,T,rounds,terminal,p_done', COUNT_CASES)
def test_count_update_conditions(group, name, policy, E, T, rounds, terminal, p_done):
    """The conditions of test_a2c_update_conditions on every case the three axes add, on the agents the GPU module's oracle
    evaluates.  The ReLU-kink cap of the new layouts is 8 columns of a tower (of 128 - 224); the older layouts keep 4."""
    _update_conditions(name, policy, E, T, rounds, terminal, p_done, sel=LY.pick_of(name),
                       max_kink=8 if name in LY.A2C_COUNT_LAYOUTS else 4, zero=_zero_tensors(policy, T, p_done))


@pytest.mark.parametrize('name,policy,E', [(n, p, E) for n in ('solo', 'many64', 'many65', 'many130') for p in ('lstm', 'fc')
                                           for E in ([LY.A2C_FORWARD_E, 33] if n == 'many64' else [LY.A2C_FORWARD_E])])
def test_count_forward_conditions(name, policy, E):
    sel = LY.pick_of(name)
    lay, c, o64, o32 = _a2c_pair(name, policy, E, sel)
    steps, boot = LY.forward_inputs(lay, E, LY.A2C_FORWARD_STEPS, np.random.RandomState(LY.data_seed(name, E)))
    pk = (lambda x: x) if sel is None else (lambda x: x[:, sel])
    pis = []
    for obs, done in steps:
        pi, v = o64.forward(pk(obs), done, 'pv')
        pi32, v32 = o32.forward(pk(obs), done, 'pv')
        pis.append(pi)
        assert np.abs(v32 - v).max() <= 2e-5 and max(np.abs(a - b).max() for a, b in zip(pi, pi32)) <= 2e-5
    _, vb = o64.forward(pk(boot), np.zeros(E), 'v')
    _, vb32 = o32.forward(pk(boot), np.zeros(E), 'v')
    assert np.abs(vb32 - vb).max() <= 2e-5
    _open_heads(lay, pis)


def test_ppo_rows_conditions():
    """The K = 2 case of the GPU module on many65 (picked agents): the clip branch is exercised at epoch 1 and few samples sit on a
    clip bound (tests/ppo_oracle.py k3_conditions), on the oracle alone."""
    from tests.ppo_oracle import K3_REWARD_NORM, fill, k3_conditions, make_oracle
    spec = LY.A2C_COUNT_LAYOUTS['many65']
    E, T, seed, rseed, lr = LY.PPO_ROWS
    sel = LY.pick_of('many65')
    o = make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=dict(spec['cfg'], reward_norm=K3_REWARD_NORM), layout=spec['layout'], sel=sel)
    o.reset()
    obs, _ = fill(spec['layout'], o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM, sel=sel)
    _, Rb = o.forward(obs[:, sel], np.zeros(E), 'v')
    for k in range(2):
        g, _ = o.compute_grads(Rb.astype(np.float32), 0.01, epoch=k, slack=False)
        clip, amb = k3_conditions(o, k)
        print('many65 epoch %d: clipped share %.3f, ambiguous %.4f' % (k, clip, amb))
        o.apply_grads(g, lr, end_of_rollout=(k == 1))


def test_count_tables_are_consistent():
    assert set(LY.COUNT_SEEDS) == set(LY.A2C_COUNT_LAYOUTS)
    assert not set(LY.A2C_LAYOUTS) & set(LY.A2C_COUNT_LAYOUTS)
    for name, spec in LY.A2C_COUNT_LAYOUTS.items():
        lay = spec['layout']
        assert lay.a_max <= 8 and spec['H'] in (128, 160, 192, 224) and lay.s_max <= 64, name
        assert (min(lay.n_f_ls) >= 1) if spec['agent'] == 'ma2c' else (max(lay.n_f_ls) == 0), name
    assert LY.IQL_LAYOUTS['q130_fused']['layout'].n_agent == LY.IQL_LAYOUTS['q130_grouped']['layout'].n_agent == 130
    assert len(COUNT_CASES) == len(set(COUNT_CASES))
