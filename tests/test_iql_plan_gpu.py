"""GPU test of the Q-learners' launch plan (csrc/tsc_iql.hip QPlan, the route at the top of iql_compute_grads): every route of every
path makes the launches it should, counted per profile id with tsc_profile_read as tests/test_iql_per_gpu.py::test_default_path_is_untouched
does.  A profile id does not tell two instantiations apart (max / Double DQN target, with / without weights, width 8 / 10, plain / dueling,
one-step / multi-step): that a route runs the RIGHT variant is what the numeric tests of tests/test_iql_target_gpu.py,
tests/test_iql_per_gpu.py, tests/test_iql_dueling_gpu.py and tests/test_iql_nstep_gpu.py pin.

Shapes: the smallest that reach every plan entry -- the fused path at both tile widths (large_grid with a wait part: width 10, E = 3 one
partial chunk; small_grid without: width 8) and the grouped-GEMM path for IQL-DNN (TSC_IQL_FUSED=0) and IQL-LR.

The expected counts are those of one tsc_iql_compute_grads + tsc_iql_apply_grads + tsc_iql_add_transition: the fused path brackets its
target (two-launch routes only: a target network, prioritized replay, the dueling head or multi-step returns), gradient and reduce
launches, the grouped path none of the three; the Floyd draw is iql_sample, the prioritized one iql_per_sample with iql_per_update behind
the gradient and iql_per_add behind the add; the window pre-pass iql_nstep runs once behind the draw whenever return_steps > 1, on both
paths, and never otherwise."""
import numpy as np
import pytest

from tests import iql_harness as H
from tests.iql_harness import KERNELS

pytestmark = pytest.mark.gpu

# scenario, agent, model_type, E, ring capacity, TSC_IQL_FUSED, fused path taken
HANDLES = [('large_grid', 'iqld', 'dqn', 3, 25, '1', True), ('small_grid', 'iqld', 'dqn', 7, 40, '1', True),
           ('large_grid', 'iqld', 'dqn', 6, 30, '0', False), ('large_grid', 'iqll', 'lr', 9, 30, '1', False)]
# (target period, double_q, prioritized replay, dueling, return_steps) -> launches of KERNELS (iql_sample, iql_per_sample, iql_nstep,
# iql_target, iql_grad, iql_reduce, iql_per_update, iql_per_add) on the fused path; the grouped path: the same with iql_target = iql_grad =
# iql_reduce = 0.  The dueling routes run on the IQL-DNN handles only (tsc_iql_set_dueling refuses IQL-LR).
ROUTES = [((0, 0, 0, 0, 1), [1, 0, 0, 0, 1, 1, 0, 0]),
          ((100, 0, 0, 0, 1), [1, 0, 0, 1, 1, 1, 0, 0]),
          ((100, 1, 0, 0, 1), [1, 0, 0, 1, 1, 1, 0, 0]),
          ((0, 0, 1, 0, 1), [0, 1, 0, 1, 1, 1, 1, 1]),
          ((100, 1, 1, 0, 1), [0, 1, 0, 1, 1, 1, 1, 1]),
          ((0, 0, 0, 1, 1), [1, 0, 0, 1, 1, 1, 0, 0]),
          ((100, 0, 0, 1, 1), [1, 0, 0, 1, 1, 1, 0, 0]),
          ((100, 1, 0, 1, 1), [1, 0, 0, 1, 1, 1, 0, 0]),
          ((100, 1, 1, 1, 1), [0, 1, 0, 1, 1, 1, 1, 1]),
          ((0, 0, 0, 0, 3), [1, 0, 1, 1, 1, 1, 0, 0]),
          ((100, 1, 0, 0, 3), [1, 0, 1, 1, 1, 1, 0, 0]),
          ((0, 0, 1, 0, 3), [0, 1, 1, 1, 1, 1, 1, 1]),
          ((0, 0, 0, 1, 3), [1, 0, 1, 1, 1, 1, 0, 0]),
          ((100, 1, 1, 1, 3), [0, 1, 1, 1, 1, 1, 1, 1])]


def _expected(counts, fused):
    return [c if fused or k not in ('iql_target', 'iql_grad', 'iql_reduce') else 0 for k, c in zip(KERNELS, counts)]


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,switch,fused', HANDLES)
def test_every_route_launches_the_kernels_of_its_plan(scenario, agent, model_type, E, cap, switch, fused, monkeypatch):
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', switch)
    scn, m = H.model(scenario, agent, model_type, E, buffer_size=cap)
    assert m.fused == fused
    rng = np.random.RandomState(E + cap)
    H.fill([m], None, scn, E, cap, rng)
    _lib.profile(enable=True)
    try:
        for route, counts in ROUTES + [ROUTES[0]]:          # ... and disarmed again: the unarmed route's launches
            period, double_q, per, duel, n = route
            if duel and model_type != 'dqn':
                continue
            H.set_target(m, period, double_q)
            H.set_per(m, per)
            if model_type == 'dqn':
                H.set_dueling(m, duel)
            H.set_steps(m, n)
            _lib.profile(reset=True)
            stats = m.minibatch_step(1e-3, want_stats=True)
            H.fill_one(m, scn, E, rng)
            got = [H.launches(k) for k in KERNELS]
            print(route, dict(zip(KERNELS, got)))
            assert got == _expected(counts, fused), route
            assert np.isfinite(stats).all() and (stats[:, 1] > 0).all()
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m.close()
