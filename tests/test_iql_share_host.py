"""Parameter sharing for the Q-learners (INTEGRATION.md "Parameter sharing"; include/tsc.h tsc_iql_set_sharing), the host side: the
classes of the built-in scenarios and of the test layouts, the config key on VecIQL's config path, what a shared step IS -- the
reference's step on the class's pooled minibatch -- and the conditions the seeds of tests/test_iql_share_gpu.py must satisfy.  No GPU,
no library."""
import numpy as np
import pytest

from deeprl_signal_control_amd.agents import share_classes
from tests import layouts as LY
from tests.iql_share_oracle import (GRID_CASE, PARITY, PARITY_LR, PARITY_STEPS, PER_BETA, SHARE_LAYOUTS, case_data, case_params, class_mean, host_oracle,
                                    members_of, pooled_grads, preload_second_moments, spec_of)
from tests.test_share_host import class_sizes


def _iql_classes(lay):
    return share_classes(lay.n_wave_ls, lay.n_w_ls, [0] * lay.n_agent, lay.n_a_ls)


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scenario,sizes,shapes', [
    ('large_grid', [12, 9, 4], {(18, 6, 5), (24, 6, 5), (30, 6, 5)}),
    ('small_grid', [3, 2, 1], {(6, 2, 2), (7, 2, 2), (7, 3, 3)}),
    ('real_net', [2] * 4 + [1] * 20, None)])
@pytest.mark.parametrize('agent', ['iqld', 'iqll'])
def test_classes_of_the_built_in_scenarios(scenario, agent, sizes, shapes):
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(scenario, agent)
    n_wave = [s - w for s, w in zip(scn.n_s_ls, scn.n_w_ls)]
    dims = list(zip(n_wave, scn.n_w_ls, scn.n_a_ls))
    cls = share_classes(n_wave, scn.n_w_ls, [0] * scn.n_agent, scn.n_a_ls)
    assert scn.n_agent == sum(sizes) and class_sizes(cls) == sizes
    if shapes is not None:
        assert {tuple(int(x) for x in d) for d in dims} == shapes
    for a, c in enumerate(cls):
        assert c <= a and cls[c] == c and dims[a] == dims[c]               # the id is the lowest member's index
        assert all(dims[b] != dims[a] for b in range(a) if cls[b] != c)    # and no earlier agent of the same shape was missed


def test_classes_of_the_test_layouts():
    for name in ('q_small', 'q_h2'):
        assert _iql_classes(LY.IQL_LAYOUTS[name]['layout']) == [0, 1, 2, 1]
    for name, spec in SHARE_LAYOUTS.items():
        assert _iql_classes(spec['layout']) == spec['classes'], name
    assert class_sizes(SHARE_LAYOUTS['lr65']['classes']) == [33, 32]
    # the reduce's grid on q160x12: a stride of several workgroups of 256 four-float columns, the last one ragged
    from deeprl_signal_control_amd.iql import QParamLayout
    lay = SHARE_LAYOUTS['q160x12']['layout']
    ql = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, 'dqn', 128, 64)
    assert ql.stride % 4 == 0 and ql.stride // 4 > 2 * 256 and (ql.stride // 4) % 256 != 0
    lay = SHARE_LAYOUTS['lr4']['layout']
    assert QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, 'lr', 128, 64).stride == 40


# ---- config ----------------------------------------------------------------------------------------------------------------------------
def test_config_key_is_checked_on_the_models_config_path():
    """VecIQL reads share_params through agents.SHARE_DEFAULTS / check_share_config before it asks for a device: a bad value is refused
    with the key's name whether or not there is a GPU, for both model types and through the E = 1 adaptor."""
    from deeprl_signal_control_amd.iql import IQL, VecIQL
    lay = SHARE_LAYOUTS['lr4']['layout']
    for bad in ('2', '-1', 2, 0.5, True, None):
        for mt in ('dqn', 'lr'):
            with pytest.raises(ValueError, match='share_params'):
                VecIQL(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, 1, lay.s_max, lay.a_max, {'share_params': bad}, model_type=mt)
        with pytest.raises(ValueError, match='share_params'):
            IQL(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, 100, {'share_params': bad})
    with pytest.raises(ValueError, match='share_params'):
        VecIQL(lay.n_s_ls, lay.n_a_ls, lay.n_w_ls, 1, lay.s_max, lay.a_max, {'SHARE_PARAMS': ' 3 '})


# ---- the oracle's pieces ---------------------------------------------------------------------------------------------------------------
def test_class_mean_of_the_oracle():
    rng = np.random.RandomState(3)
    g = [{'w': rng.randn(3, 2), 'b': rng.randn(2)} for _ in range(5)]
    out = class_mean(g, [0, 1, 0, 3, 0])
    assert members_of([0, 1, 0, 3, 0]) == {0: [0, 2, 4]}
    for k in ('w', 'b'):
        want = (g[0][k] + g[2][k] + g[4][k]) * (1.0 / 3)
        for a in (0, 2, 4):
            np.testing.assert_array_equal(out[a][k], want)
        for a in (1, 3):
            np.testing.assert_array_equal(out[a][k], g[a][k])


def _fed(name, cfg, seed, E=LY.IQL_E, cap=LY.IQL_CAP, steps=PARITY_STEPS):
    o = host_oracle(name, cfg, seed, E, cap)
    trans, idx, prio = case_data(name, seed, E, cap, steps)
    for tr in trans:
        o.add_transition(*tr)
    if cfg.get('prioritized_replay'):
        o.prio[:] = prio
        o.qmax[:] = np.maximum(np.float32(1), prio.max(2))
    return o, idx


POOLED_OBSERVED, POOLED_BOUND = 9.8e-16, 9.8e-15


@pytest.mark.parametrize('name,seed', [('q160x12', 5), ('q_small', 6), ('lr4', 5)])
def test_shared_step_is_the_step_on_the_pooled_minibatch(name, seed):
    """At equal member parameters, the class mean of the members' mean-squared-error gradients (k minibatches of E B rows) is the gradient
    of ONE OracleQ on the k E B concatenated rows: mean_a mean_r l = mean over all rows.  In float64 the two differ by rounding only.
    Measured on the CPU over the three layouts, every class and tensor: max|d| / max|g| of the tensor at most 9.8e-16 (POOLED_OBSERVED: 9.74e-16 on
    q160x12, 8.39e-16 on q_small, 3.73e-16 on lr4); asserted at ten times that, 9.8e-15 (POOLED_BOUND).  The loss is the mean of the members' losses in the same sense."""
    o, idx = _fed(name, {}, seed)
    losses, _, _ = o.minibatch_step(0.0, idx_given=idx[0])               # lr 0: the parameters stay where the gradients were taken
    worst = 0.0
    for members in members_of(o.classes).values():
        loss, g = pooled_grads(o, members)
        assert abs(loss - np.mean([losses[a] for a in members])) <= 1e-14 * abs(loss)
        raw_differ = False
        for k, ref in g.items():
            mean = o.last_mean[members[0]][k]
            scale = np.abs(ref).max()
            assert scale > 0
            worst = max(worst, float(np.abs(mean - ref).max() / scale))
            raw_differ |= bool(np.abs(o.last_raw[members[0]][k] - ref).max() > 1e-3 * scale)
        assert raw_differ                                                 # (a member's own gradient is not the pooled one)
    print('%s: class mean vs pooled gradient, worst max|d| / max|g| %.2e (bound %.2e)' % (name, worst, POOLED_BOUND))
    assert worst <= POOLED_BOUND


# ---- the seeds of the GPU cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,cfg,seed', PARITY, ids=[n + ('_armed' if c else '') for n, c, _ in PARITY])
def test_parity_seeds_meet_their_conditions(name, cfg, seed):
    """The update-parity cases of tests/test_iql_share_gpu.py on the oracle alone, so that the GPU module needs no skips: in every step
    no sampled row puts a hidden unit of any agent within 1e-6 of a ReLU kink (tests/iql_harness.py::kinks; the class mean would carry one
    member's kink to all), every class norm stays below max_grad_norm, the members of a class hold different raw gradients and the same
    parameters after the step, and -- Double DQN -- every sampled row's online argmax is decided by iql_harness.GAP and some pick is not the
    frozen copy's argmax."""
    _conditions(name, cfg, seed, LY.IQL_E, LY.IQL_CAP, PARITY_STEPS, 0)


def test_grid_case_meets_its_conditions():
    """large_grid's 25 iqld agents at E = 3 (classes 12 + 9 + 4), one step: as above, except that 25 agents x 60 rows meet a first-layer
    kink now and then -- at most 4 first-layer columns per agent (the exception of iql_harness.compare_grads), no second-layer unit."""
    E, cap, seed = GRID_CASE
    assert class_sizes(spec_of('large_grid')['classes']) == [12, 9, 4]
    _conditions('large_grid', {}, seed, E, cap, 1, 4)


def _conditions(name, cfg, seed, E, cap, steps, max_cols):
    from tests.iql_harness import GAP, gap_of, kinks
    o, idx = _fed(name, cfg, seed, E, cap, steps)
    preload_second_moments(o)
    A = o.A
    for step in range(steps):
        rows = [[o.rings[e][a].buffer for e in range(E)] for a in range(A)]
        before = [{k: v.clone() for k, v in q.p.items()} for q in o.qs]
        losses, norms, raw = o.minibatch_step(PARITY_LR, beta=PER_BETA, idx_given=idx[step])
        np.testing.assert_array_equal(o.last_idx, idx[step])
        assert norms.max() < 0.9 * 40.0 and norms.min() > 0, norms
        for a in range(A):
            saved, o.qs[a].p = o.qs[a].p, before[a]
            cols, deep = kinks(o, [rows[a][e][s][0] for e in range(E) for s in idx[step][e, a]], a)
            o.qs[a].p = saved
            assert not deep and (cols is None or cols.sum() <= max_cols), 'step %d agent %d: a hidden unit on a ReLU kink' % (step, a)
        differ = False
        for members in members_of(o.classes).values():
            assert len({norms[a] for a in members}) == 1
            for a in members[1:]:
                assert any(np.abs(raw[a][k] - raw[members[0]][k]).max() > 0 for k in raw[a])
                for k in o.qs[a].p:
                    assert bool((o.qs[a].p[k] == o.qs[members[0]].p[k]).all()) and bool((o.qs[a].target[k] == o.qs[members[0]].target[k]).all())
        if cfg.get('double_q'):
            for q in o.qs:
                assert gap_of(q.last_q1_online) >= GAP
                differ |= bool((q.last_astar != np.argmax(q.last_q1_target, 1)).any())
            assert differ
        if cfg.get('return_steps'):
            assert (o.last_k > 1).any() and (o.last_k < cfg['return_steps']).any()      # full and cut windows
    print('%s %r: norms of the last step %s' % (name, cfg, np.round(norms, 3)))


def test_case_params_are_the_lowest_members_draws():
    """case_params restates VecIQL's initialisation rule: every agent is drawn in the unshared order, then takes its class's lowest
    member's draw -- so an agent alone in its class, and every lowest member, starts where an unshared model's does."""
    from deeprl_signal_control_amd.iql import QParamLayout, init_agent_params
    spec = SHARE_LAYOUTS['q_small']
    lay = spec['layout']
    ql = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, 'dqn', 64, 32)
    plain, shared = init_agent_params(ql, np.random.RandomState(6)), case_params('q_small', {}, 6)
    for a, c in enumerate(spec['classes']):
        for k in plain[a]:
            np.testing.assert_array_equal(shared[a][k], plain[c][k])
    assert any(np.abs(plain[3][k] - plain[1][k]).max() > 0 for k in plain[1])
