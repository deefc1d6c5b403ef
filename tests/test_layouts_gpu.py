"""GPU parity of both learners on the synthetic agent layouts of tests/layouts.py: every declared limit of the kernel choice
("Supported layouts") run on both of its sides, against the float64 oracles the learner suite uses.

Every case first asserts the ROUTE the handle took (tsc_model_plan / tsc_model_path / tsc_iql_path) against the value written in the
layout table -- a case that silently took another kernel than the one it is named after would check nothing -- then runs the body
of the existing parity test (tests/test_model_gpu.py, tests/test_iql_gpu.py, tests/test_iql_dueling_gpu.py, tests/test_iql_per_gpu.py,
tests/test_ppo_gpu.py: the helpers those tests are made of, which take a layout where they take a scenario name).

Batches: A2C (E, T) = (5, 6) and (37, 7), N = 30 and 259 rows, ragged in every row loop (the row-loop boundaries themselves are
tests/test_update_staging_gpu.py's); IQL E = 5 with ring capacity 30, 100 rows = one 64-row chunk and a partial one.

Tolerances are the ones the reused modules state: pi |d| <= 2e-5; gradients 2e-5 max|g| per tensor, 2e-4 in the second round;
ReLU-kink columns excepted as _grad_err / iql_harness.kinks do; parameters 3e-5.  v and Q: |d| <= 2e-5 on the layouts inside the reference's
input ranges; 2e-5 max(1, max|oracle value|) on the `wide` ones (up to 68 inputs in [0, 2): obs64, obs68, q_obs52, lr_wide), whose
values leave the reference's range.  tests/test_layouts_host.py measures the float32 restatement of the oracle against float64 on
these very inputs: |dv| <= 8.2e-7 (max|v| 2.35) and |dQ| <= 8.5e-7 (max|Q| 4.28) over all layouts, far inside either bound, and on
the gradients at most 1.7e-6 max|g| in the first round and 4.1e-6 in the second.  The seeds come from tests/layouts.py, where the
host module pins what they must satisfy."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import iql_harness as H
from tests import layouts as LY
from tests.test_layouts_host import value_bound

pytestmark = pytest.mark.gpu

A2C_CASES = [(n, p) for n in LY.A2C_LAYOUTS for p in ('lstm', 'fc')]
EDGES = [n for n in LY.A2C_LAYOUTS if n.startswith('edges')]


def _plan_of(spec, policy, E, G):
    """What tsc_model_plan must report for a layout: the table's route, s_upd ~ one workgroup per CU, s_fwd capped by the 32-instance tiles."""
    r = spec['route'][policy]
    s_upd, s_fwd = LY.upd_splits(G // 2), LY.fwd_splits(G // 2, E)
    if policy == 'lstm':
        return (r[0], r[1], r[2], 0, s_fwd, s_upd), (-1, -1)
    return (r[0], 0, 0, r[1], s_fwd, s_upd), ({LY.FC_MFMA: 2, LY.FC_THREAD: 1, LY.DENSE: 0}[r[0]], r[1])


def _a2c(name, policy, E, T, sel=None):
    from tests.test_model_gpu import _make
    spec = LY.spec_of(name)
    lay, m, o = _make(spec['agent'], E, T, seed=LY.seed_of(name), policy=policy, scenario=spec['layout'], sel=sel, **spec['cfg'])
    plan, fc_path = _plan_of(spec, policy, E, m.G)
    assert m.H == spec['H'] and m.plan == plan and m.fc_path == fc_path, \
        '%s %s: plan %r / fc_path %r, the layout table says %r / %r' % (name, policy, m.plan, m.fc_path, plan, fc_path)
    return spec, lay, m, o


@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_forward(name, policy):
    """pi, v and the non-advancing bootstrap value over 3 steps with random dones (the body of test_forward_matches_oracle) through
    forward_sample: padded actions exactly 0, rows of pi sum to 1, the action is np.random.choice on the kernel's own pi."""
    from tests.test_model_gpu import _forward_vs_oracle
    E = LY.A2C_FORWARD_E
    spec, lay, m, o = _a2c(name, policy, E, 4)
    _forward_vs_oracle(lay, m, o, E, np.random.RandomState(LY.data_seed(name, E)), steps=LY.A2C_FORWARD_STEPS, sample=True,
                       vtol=value_bound if spec['wide'] else 2e-5)
    m.close()


@pytest.mark.parametrize('use_cache', [True, False])
@pytest.mark.parametrize('E,T', LY.A2C_BATCHES)
@pytest.mark.parametrize('name,policy', A2C_CASES)
def test_a2c_update(name, policy, E, T, use_cache):
    """Two update rounds (the body of test_backward_matches_oracle): returns bit-exact, every gradient tensor, flat ==
    pack(unpack(flat)) -- the structural zeros of W1 exactly zero --, losses, norm, parameters after the step."""
    from tests.test_model_gpu import _backward_vs_oracle
    spec, lay, m, o = _a2c(name, policy, E, T)
    _backward_vs_oracle(lay, m, o, E, T, np.random.RandomState(LY.data_seed(name, E, T)), False, use_cache)
    m.close()


@pytest.mark.parametrize('policy', ['lstm', 'fc'])
@pytest.mark.parametrize('name', EDGES)
def test_a2c_fused_update_equals_grouped_gemms_on_block_edges_inside_a_tile(name, policy, monkeypatch):
    """The one-pass update kernels against the grouped GEMMs they replace (the body of test_fused_update_kernels_equal_grouped_gemms)
    with block edges inside a 32-column tile of krange and a 16-column unit of ftmask: same gradient, same zero pattern."""
    from tests.test_model_gpu import _fused_vs_grouped
    spec = LY.A2C_LAYOUTS[name]
    E, T = LY.A2C_BATCHES[1]
    fused, grouped = _fused_vs_grouped(spec['agent'], ('TSC_UNFUSED_DW', 'TSC_UNFUSED_DX'), policy, monkeypatch, E=E, T=T,
                                       scenario=spec['layout'], **spec['cfg'])
    assert fused[:4] == _plan_of(spec, policy, E, 2 * spec['layout'].n_agent)[0][:4] and fused[1:4] == ((1, 1, 0) if policy == 'lstm' else (0, 0, 1))
    assert grouped[0] == fused[0] and grouped[1:4] == (0, 0, 0)


def test_a2c_ppo_k3_on_the_full_head():
    """Three PPO epochs on head8 (MA2C, LSTM; n_a = 8, 7, 2, 5, 8) against tests/ppo_oracle.py: head_bwd_kernel<true> is an instantiation of
    its own of the 8-lane head mapping.  The case and what it must satisfy on the oracle alone: tests/layouts.py PPO_HEAD8,
    tests/test_layouts_host.py::test_ppo_head8_conditions."""
    from tests.test_ppo_gpu import _k3
    spec = LY.A2C_LAYOUTS['head8']
    E, T, seed, rseed, lr = LY.PPO_HEAD8
    _k3('ma2c', 'lstm', E, T, seed, rseed, lr, layout=spec['layout'], **spec['cfg'])


def test_a2c_refuses_a_hidden_width_that_is_no_multiple_of_4():
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import A2C_DEFAULTS, TscModelCfg, VecA2C, _setup_lib
    spec = LY.A2C_REFUSED
    lay, c = spec['layout'], dict(A2C_DEFAULTS, **spec['cfg'])
    L = _lib.lib()
    _setup_lib(L)
    ip = C.POINTER(C.c_int32)
    arrs = [np.ascontiguousarray(x, np.int32) for x in (lay.n_wave_ls, lay.n_w_ls, [0] * lay.n_agent, lay.n_a_ls)]
    for kind in (0, 1):
        mc = TscModelCfg(lay.n_agent, lay.s_max, lay.a_max, *[a.ctypes.data_as(ip) for a in arrs], c['num_fw'], c['num_ft'], 0, 64, 6,
                         c['gamma'], c['reward_norm'], c['reward_clip'], c['value_coef'], c['max_grad_norm'], c['rmsp_alpha'],
                         c['rmsp_epsilon'], kind)
        h = C.c_void_p()
        assert L.tsc_model_create(C.byref(mc), 5, 0, C.byref(h)) != 0
        assert h.value is None                                                  # no handle left behind
        assert 'hidden width must be a multiple of 4' in L.tsc_last_error().decode()
    with pytest.raises(RuntimeError, match='hidden width must be a multiple of 4'):
        VecA2C(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, lay.n_f_ls, 5, lay.s_max, lay.a_max, dict(batch_size=6, **spec['cfg']), seed=1, name='ia2c')


# ---- the agent-count, row-split and time axes (tests/layouts.py A2C_COUNT_LAYOUTS, ROWS, count_cases) -------------------------------
# From 64 agents on the float64 oracle evaluates LY.pick(A) -- the first, the last, two in between and index 128 -- as
# test_update_benchmarked_batch_E1024_T120 does; returns and advantages are compared for every agent.
COUNT = [n for n in ('solo', 'many64', 'many65', 'many130')]


def _cases(group, both_caches):
    return [c[1:] + (uc,) for c in LY.count_cases() if c[0] == group for uc in ((True, False) if both_caches else (True,))]


def _update_case(name, policy, E, T, rounds, terminal, p_done, use_cache, worst=None):
    from tests.test_model_gpu import _backward_vs_oracle
    sel = LY.pick_of(name)
    spec, lay, m, o = _a2c(name, policy, E, T, sel)
    flats = _backward_vs_oracle(lay, m, o, E, T, np.random.RandomState(LY.data_seed(name, E, T)), terminal, use_cache, sel=sel, p_done=p_done,
                                rounds=rounds, worst=worst)
    m.close()
    return flats


@pytest.mark.parametrize('name,policy,E', [(n, p, E) for n in COUNT for p in ('lstm', 'fc')
                                           for E in ([LY.A2C_FORWARD_E, 33] if n == 'many64' else [LY.A2C_FORWARD_E])])
def test_count_forward(name, policy, E):
    """test_a2c_forward on 1, 64, 65 and 130 agents; on many64 also at E = 33, the first batch with two forward workgroups per tower."""
    from tests.test_model_gpu import _forward_vs_oracle
    sel = LY.pick_of(name)
    spec, lay, m, o = _a2c(name, policy, E, 4, sel)
    _forward_vs_oracle(lay, m, o, E, np.random.RandomState(LY.data_seed(name, E)), steps=LY.A2C_FORWARD_STEPS, sample=True, sel=sel)
    m.close()


@pytest.mark.parametrize('name,policy,E,T,rounds,terminal,p_done,use_cache', _cases('count', True))
def test_count_update(name, policy, E, T, rounds, terminal, p_done, use_cache):
    """test_a2c_update where the agent count changes the launch: s_upd = 128 (solo: most splits empty), 2, 1, and 256 / G = 0."""
    _update_case(name, policy, E, T, rounds, terminal, p_done, use_cache)


@pytest.mark.parametrize('name,policy,E,T,rounds,terminal,p_done,use_cache', _cases('rows', False))
def test_row_sweep(name, policy, E, T, rounds, terminal, p_done, use_cache):
    """One update round per ROWS case through the activation cache: a split of R = E T rows (many64: two splits) walks a chosen
    number of full intervals and tail sub-chunks of dwxh_kernel and of plain and clamped chunks of dx1w1_kernel2 / fc_bwd_kernel.
    Gradients, structural zeros, flat == pack(unpack), losses, norm; then the same rollout on a fresh handle: the kernels are
    documented as deterministic, and a barrier mistake in the tail shows as a difference between two runs.
    (many65 LSTM at E = 1, T = 2 comes to 1.5e-5 of the 2e-5, every other case to about 1e-6: there dWh of a value tower is the one outer
    product h_0 (x) dz_1 with dz_1 ~ v_1 - R_1 = 0.0058, a cancelled difference that magnifies a 9e-8 rounding of v_1; CHANGELOG.md.)"""
    worst = {}
    first = _update_case(name, policy, E, T, rounds, terminal, p_done, use_cache, worst)
    second = _grads_only(name, policy, E, T, use_cache)
    np.testing.assert_array_equal(first[0], second)
    A = LY.spec_of(name)['layout'].n_agent
    S = LY.upd_splits(A)
    print('row sweep %s %s E=%d T=%d: dwxh %s, w1 %s, worst |dg| / max|g| %.1e at (tower, tensor, max|g|) %r' % (
        name, policy, E, T, [LY.dwxh_schedule(R) for R in LY.split_R(E * T, S, LY.DWXH_Q)],
        [LY.w1_schedule(R) for R in LY.split_R(E * T, S, LY.W1_Q)], worst[0], worst['where', 0]))


class _NoOracle:
    def forward(self, *a):
        return None

    def add_transition(self, *a):
        return None


def _grads_only(name, policy, E, T, use_cache):
    """The gradient buffer of the first update of a case's rollout on a fresh handle (no oracle)."""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import VecA2C
    from tests.test_model_gpu import _fill
    spec = LY.spec_of(name)
    lay = spec['layout']
    m = VecA2C(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, lay.n_f_ls, E, lay.s_max, lay.a_max, dict(batch_size=T, **spec['cfg']), device=0,
               seed=LY.seed_of(name), name=spec['agent'], policy=policy)
    m.reset()
    obs, _ = _fill(lay, m, _NoOracle(), E, T, np.random.RandomState(LY.data_seed(name, E, T)), use_cache=use_cache, sel=[])
    Rb = m.forward(torch.from_numpy(obs).cuda(), False, 'v').clone()
    _lib.check(m._L.tsc_model_compute_grads(m._h, C.c_void_p(Rb.data_ptr()), 0.01))
    flat = m.grad_tensor().cpu().numpy().reshape(m.G, m.stride).copy()
    m.close()
    return flat


@pytest.mark.parametrize('E,T', LY.ROWS_FUSED)
@pytest.mark.parametrize('policy', ['lstm', 'fc'])
def test_row_sweep_fused_update_equals_grouped_gemms(policy, E, T, monkeypatch):
    """The one-pass update kernels against the grouped GEMMs at splits with a full interval and a ragged tail (many65: R = E T)."""
    from tests.test_model_gpu import _fused_vs_grouped
    spec = LY.A2C_COUNT_LAYOUTS['many65']
    fused, grouped = _fused_vs_grouped(spec['agent'], ('TSC_UNFUSED_DW', 'TSC_UNFUSED_DX'), policy, monkeypatch, E=E, T=T,
                                       scenario=spec['layout'], sel=[0], **spec['cfg'])
    assert fused == _plan_of(spec, policy, E, 2 * spec['layout'].n_agent)[0] and fused[1:4] == ((1, 1, 0) if policy == 'lstm' else (0, 0, 1))
    assert grouped[0] == fused[0] and grouped[1:4] == (0, 0, 0) and grouped[4:] == fused[4:]


@pytest.mark.parametrize('name,policy,E,T,rounds,terminal,p_done,use_cache', _cases('time', True))
def test_time_axis_update(name, policy, E, T, rounds, terminal, p_done, use_cache):
    """T = 1 and T = 2: the edges of lstm_fwd_kernel<PF>'s next-step prefetch and of lstm_bwd2_kernel's previous-step one.  Two
    rounds, the first ending on a terminal step."""
    _update_case(name, policy, E, T, rounds, terminal, p_done, use_cache)


@pytest.mark.parametrize('name,policy,E,T,rounds,terminal,p_done,use_cache', _cases('done', True))
def test_done_patterns_update(name, policy, E, T, rounds, terminal, p_done, use_cache):
    """Done after every step (h_prev masked everywhere: dWh exactly zero) and never done after the reset, on head8, T = 7."""
    _update_case(name, policy, E, T, rounds, terminal, p_done, use_cache)


def test_ppo_k2_on_a_ragged_split():
    """Two PPO epochs on many65 at a ROWS case with a full interval and a ragged tail (R = 207) against tests/ppo_oracle.py on the picked
    agents, at the tolerances of test_k3_epochs_match_oracle: epoch 1 takes the re-forward path over the same split."""
    from tests.ppo_oracle import K3_REWARD_NORM, fill, k3_conditions
    from tests.test_ppo_gpu import _check_grads, _check_params, _dev, _make, _put_copy
    spec = LY.A2C_COUNT_LAYOUTS['many65']
    E, T, seed, rseed, lr = LY.PPO_ROWS
    sel = LY.pick_of('many65')
    lay, m, o = _make('ma2c', 'lstm', E, T, seed, sel=sel, layout=spec['layout'], algo='ppo', ppo_epochs=2, reward_norm=K3_REWARD_NORM,
                      lr_init=lr, **spec['cfg'])
    assert m.plan == _plan_of(spec, 'lstm', E, m.G)[0]
    obs, _ = fill(lay, o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM, put=_put_copy(m), sel=sel)
    Rb = m.forward(_dev(obs), False, 'v').clone()
    for k in range(2):
        ograds, ostats = o.compute_grads(Rb.cpu().numpy()[:, sel], 0.01, epoch=k)
        k3_conditions(o, k)
        m.compute_grads(Rb, k)
        worst = _check_grads(m, o, ograds, 2e-5 if k == 0 else 2e-4, sel=sel, slack=True, what='epoch %d' % k)
        stats = m.apply_grads(1.0, want_stats=True, epoch=k)
        onorm = o.apply_grads(ograds, lr, end_of_rollout=(k == 1))
        print('many65 PPO epoch %d: worst |dg| / max|g| %.1e' % (k, worst))
        np.testing.assert_allclose(stats[sel, 4], o.clip_share, rtol=2e-3, atol=o.amb_share.max() + 1e-12)
        np.testing.assert_allclose(stats[sel, 5], o.approx_kl, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[sel, 1:3], ostats[:, 1:], rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[sel, 3], onorm, rtol=2e-3)
        _check_params(m, o, sel=sel, what='epoch %d' % k)
    m.close()


@pytest.mark.parametrize('name', ['ws_edge_340', 'ws_edge_341'])
def test_workspace_edge(name):
    """340 agents at H = 224 are the last whose dwxh records fit the workspace (plan: dwxh = 1), 341 the first past it (dwxh = 0:
    the grouped GEMMs); the plan is asserted against the route of the layout table.  A handle of 680 towers takes seconds to create
    and fill, so the update round at E = 3, T = 2 against the oracle on the picked agents runs on 341 only: the side whose route
    no other test takes at H = 224."""
    if name == 'ws_edge_340':
        from deeprl_signal_control_amd.agents import VecA2C
        spec = LY.spec_of(name)
        lay, (E, T) = spec['layout'], LY.WS_EDGE_BATCH
        m = VecA2C(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, lay.n_f_ls, E, lay.s_max, lay.a_max, dict(batch_size=T, **spec['cfg']), device=0,
                   seed=None, name=spec['agent'], policy='lstm')
        assert m.plan == _plan_of(spec, 'lstm', E, m.G)[0] and m.plan[1] == 1
        m.close()
        return
    (case,) = [c for c in LY.count_cases() if c[0] == 'edge' and c[1] == name]
    worst = {}
    _update_case(*case[1:], True, worst)
    print('%s: dwxh = %d, worst |dg| / max|g| %.1e' % (name, LY.spec_of(name)['route']['lstm'][1], worst[0]))


# ---- IQL --------------------------------------------------------------------------------------------------------------------------
def _iql(name, monkeypatch, fused_knob=None):
    spec = LY.IQL_LAYOUTS[name]
    if fused_knob is not None:
        monkeypatch.setenv('TSC_IQL_FUSED', fused_knob)
    else:
        monkeypatch.delenv('TSC_IQL_FUSED', raising=False)
    lay, m, o = H.make(spec['layout'], 'iql', spec['model_type'], LY.IQL_E, seed=LY.SEEDS[name], buffer_size=LY.IQL_CAP,
                      reward_norm=LY.IQL_REWARD_NORM, **spec['cfg'])
    want = spec['fused'] and fused_knob != '0'
    assert m.fused == want, '%s: fused = %r, the layout table says %r' % (name, m.fused, want)
    return spec, lay, m, o


@pytest.mark.parametrize('name', list(LY.IQL_LAYOUTS))
def test_iql_forward_and_epsilon_greedy(name, monkeypatch):
    spec, lay, m, o = _iql(name, monkeypatch)
    H.forward_and_act(lay, m, o, LY.IQL_E, np.random.RandomState(LY.data_seed(name, LY.IQL_E)), qtol=value_bound if spec['wide'] else 2e-5)
    m.close()


@pytest.mark.parametrize('name', list(LY.IQL_LAYOUTS))
def test_iql_replay_gradient_and_adam(name, monkeypatch):
    """The body of test_replay_minibatch_gradient_and_adam with two minibatch steps."""
    spec, lay, m, o = _iql(name, monkeypatch)
    H.replay_vs_oracle(lay, m, o, LY.IQL_E, LY.IQL_CAP, np.random.RandomState(LY.data_seed(name, LY.IQL_E, LY.IQL_CAP)), steps=LY.IQL_STEPS)
    m.close()


def _duel(name, fused_knob, monkeypatch, **cfg):
    """The dueling head on the layout's agents with n_a <= 7 (column 7 of the head is V; tsc_iql_set_dueling refuses n_a = 8)."""
    spec = LY.IQL_LAYOUTS[name]
    lay = spec['layout'].only(lambda na: na <= 7)
    assert max(lay.n_a_ls) == 7 and lay.n_agent >= 4
    monkeypatch.setenv('TSC_IQL_FUSED', fused_knob)
    _, m = H.duel_model(lay, LY.IQL_E, LY.IQL_CAP, seed=LY.SEEDS[name], **spec['cfg'], **cfg)
    assert m.fused == (fused_knob == '1')
    return lay, m, H.oracle_for(m)


@pytest.mark.parametrize('fused_knob', ['1', '0'])
@pytest.mark.parametrize('name', ['q160_edge', 'q128_edge'])
def test_iql_dueling_forward(name, fused_knob, monkeypatch):
    lay, m, o = _duel(name, fused_knob, monkeypatch)
    H.duel_forward_vs_oracle(lay, m, o, LY.IQL_E, np.random.RandomState(LY.data_seed(name, LY.IQL_E)))
    m.close()


@pytest.mark.parametrize('target_update,double_q', [(0, 0), (100, 1)])
@pytest.mark.parametrize('fused_knob', ['1', '0'])
@pytest.mark.parametrize('name', ['q160_edge', 'q128_edge'])
def test_iql_dueling_targets_and_gradient(name, fused_knob, target_update, double_q, monkeypatch):
    """Targets and gradient of the dueling head at its last legal action count: the columns n_a <= j < 7 of dWq | dbq are exactly zero
    (dead_columns_are_zero), and at n_a = 7 that range is empty and column 7 carries dV right behind the seventh action's column."""
    lay, m, o = _duel(name, fused_knob, monkeypatch, target_update=target_update, double_q=double_q)
    rng = np.random.RandomState(LY.data_seed(name, LY.IQL_E, LY.IQL_CAP) + double_q + target_update)
    flat_g = H.targets_and_gradient_vs_oracle(lay, m, o, LY.IQL_E, LY.IQL_CAP, rng)
    ql, a7 = m.layout, lay.n_a_ls.index(7)
    head = flat_g.reshape(ql.A, ql.stride)[a7, ql.oWq:ql.obq].reshape(ql.H2, 8)
    assert (np.abs(head).max(0) > 0).all() and (flat_g.reshape(ql.A, ql.stride)[a7, ql.obq:ql.obq + 8] != 0).all()
    m.close()


def test_iql_prioritized_replay_step_at_the_fused_limit(monkeypatch):
    """One prioritized-replay step (target network + Double DQN, beta 0.4) on q160_edge against tests/iql_ext_oracle.py."""
    name = 'q160_edge'
    spec = LY.IQL_LAYOUTS[name]
    monkeypatch.delenv('TSC_IQL_FUSED', raising=False)
    lay, m = H.model(spec['layout'], 'iql', 'dqn', LY.IQL_E, seed=LY.SEEDS[name], buffer_size=LY.IQL_CAP, prioritized_replay=1,
                    target_update=100, double_q=1, **spec['cfg'])
    assert m.fused
    H.per_step_vs_oracle(lay, m, LY.IQL_E, LY.IQL_CAP, np.random.RandomState(LY.data_seed(name, LY.IQL_E, LY.IQL_CAP) + 1), 0.4)
    m.close()


def test_iql_refuses_hidden_widths_that_are_no_multiples_of_4():
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, TscIqlCfg, VecIQL, _setup_lib
    spec = LY.IQL_REFUSED
    lay, c = spec['layout'], dict(IQL_DEFAULTS, **spec['cfg'])
    L = _lib.lib()
    _setup_lib(L)
    ip = C.POINTER(C.c_int32)
    arrs = [np.ascontiguousarray(x, np.int32) for x in (lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls)]
    mc = TscIqlCfg(lay.n_agent, lay.s_max, lay.a_max, *[a.ctypes.data_as(ip) for a in arrs], 1, c['num_fc'], c['num_h'], 20, LY.IQL_CAP,
                   c['gamma'], LY.IQL_REWARD_NORM, c['reward_clip'], c['max_grad_norm'])
    h = C.c_void_p()
    assert L.tsc_iql_create(C.byref(mc), LY.IQL_E, 0, C.byref(h)) != 0
    assert h.value is None                                                      # no handle left behind
    assert 'hidden widths must be multiples of 4' in L.tsc_last_error().decode()
    with pytest.raises(RuntimeError, match='hidden widths must be multiples of 4'):
        VecIQL(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, LY.IQL_E, lay.s_max, lay.a_max, dict(batch_size=20, buffer_size=LY.IQL_CAP, **spec['cfg']),
               seed=1, model_type='dqn')
