"""GPU test of the Q-learners' launch plan (csrc/tsc_iql.hip QPlan, the route at the top of iql_compute_grads): every route of every
path makes the launches it should, counted per profile id with tsc_profile_read as tests/test_iql_per_gpu.py::test_default_path_is_untouched
does.  A profile id does not tell two instantiations apart (max / Double DQN target, with / without weights, width 8 / 10): that a route
runs the RIGHT variant is what the numeric tests of tests/test_iql_target_gpu.py and tests/test_iql_per_gpu.py pin.

Shapes: the smallest that reach every plan entry -- the fused path at both tile widths (large_grid with a wait part: width 10, E = 3 one
partial chunk; small_grid without: width 8) and the grouped-GEMM path for IQL-DNN (TSC_IQL_FUSED=0) and IQL-LR.

The expected counts are those of one tsc_iql_compute_grads + tsc_iql_apply_grads + tsc_iql_add_transition as iql_compute_grads stood
before there was a plan: the fused path brackets its target (two-launch routes only), gradient and reduce launches, the grouped path none
of the three; the Floyd draw is iql_sample, the prioritized one iql_per_sample with iql_per_update behind the gradient and iql_per_add
behind the add."""
import numpy as np
import pytest

from tests.test_iql_per_gpu import _fill_one, _launches, _set_per
from tests.test_iql_target_gpu import _fill, _model, _set_target

pytestmark = pytest.mark.gpu

KERNELS = ('iql_sample', 'iql_per_sample', 'iql_target', 'iql_grad', 'iql_reduce', 'iql_per_update', 'iql_per_add')
# scenario, agent, model_type, E, ring capacity, TSC_IQL_FUSED, fused path taken
HANDLES = [('large_grid', 'iqld', 'dqn', 3, 25, '1', True), ('small_grid', 'iqld', 'dqn', 7, 40, '1', True),
           ('large_grid', 'iqld', 'dqn', 6, 30, '0', False), ('large_grid', 'iqll', 'lr', 9, 30, '1', False)]
# (target period, double_q, prioritized replay) -> launches of KERNELS on the fused path; the grouped path: the same with
# iql_target = iql_grad = iql_reduce = 0
ROUTES = [((0, 0, 0), [1, 0, 0, 1, 1, 0, 0]),
          ((100, 0, 0), [1, 0, 1, 1, 1, 0, 0]),
          ((100, 1, 0), [1, 0, 1, 1, 1, 0, 0]),
          ((0, 0, 1), [0, 1, 1, 1, 1, 1, 1]),
          ((100, 1, 1), [0, 1, 1, 1, 1, 1, 1])]


def _expected(counts, fused):
    return [c if fused or k not in ('iql_target', 'iql_grad', 'iql_reduce') else 0 for k, c in zip(KERNELS, counts)]


@pytest.mark.parametrize('scenario,agent,model_type,E,cap,switch,fused', HANDLES)
def test_every_route_launches_the_kernels_of_its_plan(scenario, agent, model_type, E, cap, switch, fused, monkeypatch):
    from deeprl_signal_control_amd import _lib
    monkeypatch.setenv('TSC_IQL_FUSED', switch)
    scn, m = _model(scenario, agent, model_type, E, buffer_size=cap)
    assert m.fused == fused
    rng = np.random.RandomState(E + cap)
    _fill([m], None, scn, E, cap, rng)
    _lib.profile(enable=True)
    try:
        for (period, double_q, per), counts in ROUTES + [ROUTES[0]]:          # ... and disarmed again: the unarmed route's launches
            _set_target(m, period, double_q)
            _set_per(m, per)
            _lib.profile(reset=True)
            stats = m.minibatch_step(1e-3, want_stats=True)
            _fill_one(m, scn, E, rng)
            got = [_launches(k) for k in KERNELS]
            print((period, double_q, per), dict(zip(KERNELS, got)))
            assert got == _expected(counts, fused), (period, double_q, per)
            assert np.isfinite(stats).all() and (stats[:, 1] > 0).all()
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    m.close()
