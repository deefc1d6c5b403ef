"""Which step_kernel instantiation a handle launches (tsc_env_step_plan, VecTrafficEnv.step_plan) for every state that enters the
choice: the expectations are the rules of INTEGRATION.md section 5 written out as literals (row = (MAXT, HELP, REC, KF, SPEC),
threads per workgroup), on large_grid with four instances and once on Monaco.  Every case ends with a reset and two steps: the
planned launch succeeds.  What the kernels compute is pinned elsewhere (test_env_gpu, test_krauss_gpu, test_trace_gpu,
test_lane_data_gpu); this file pins which one runs."""
import pytest
import torch

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net

pytestmark = pytest.mark.gpu

E = 4
LDS_MAX = 160 * 1024
IDM_DEFAULT = (1024, 1, 0, 1, 1)           # four instances on an empty device: 1024 threads each, large_grid's dimensions compiled in
KNOBS = ('TSC_ENV_SPEC', 'TSC_ENV_KF', 'TSC_ENV_THREADS', 'TSC_ENV_HELP')


@pytest.fixture(scope='module')
def scns():
    return {'idm': build_large_grid('ma2c'), 'krauss': build_large_grid('ma2c', car_following='krauss', krauss_sigma=0.5)}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _env(scn, **kw):
    from deeprl_signal_control_amd.env import VecTrafficEnv
    return VecTrafficEnv(scn, E, seed=5, **kw)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(env, row, threads=None):
    p = env.step_plan()
    print('step_plan', p)
    assert p['row'] == row
    if threads is not None:
        assert p['threads'] == threads
    assert p['threads'] <= p['row'][0]
    assert 0 < p['lds_bytes'] <= LDS_MAX
    return p


def _step2(env):
    act = torch.zeros(E, env.A, dtype=torch.int32, device='cuda')
    for _ in range(2):
        obs, _, _, _ = env.step(act)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all())


def _runs(env):
    env.reset()
    _step2(env)


def _resident(env, n):
    _lib.check(env._L.tsc_env_set_resident_instances(env._h, int(n)))


def test_fresh_handle(scns):
    env = _env(scns['idm'])
    _plan(env, IDM_DEFAULT, 1024)
    _runs(env)
    _plan(env, IDM_DEFAULT, 1024)
    env.close()


@pytest.mark.parametrize('cus_times,row', [(1, (512, 1, 0, 2, 1)), (2, (256, 1, 0, 2, 1))])
def test_resident_instances(scns, cus_times, row):
    env = _env(scns['idm'])
    _resident(env, cus_times * _cus() + 1)
    _plan(env, row, row[0])
    _runs(env)
    env.close()
    env = _env(scns['idm'], resident=cus_times * _cus() + 1)
    _plan(env, row, row[0])
    env.close()


def test_recording_and_trace(scns):
    env = _env(scns['idm'])
    env.set_record(True)
    _plan(env, (1024, 0, 1, 4, 0), 1024)
    env.set_trace([0, 2], row_cap=1 << 12)
    _plan(env, (1024, 0, 1, 4, -2), 1024)          # at once, no reset in between
    _runs(env)
    env.set_trace([])
    _plan(env, (1024, 0, 1, 4, 0), 1024)
    _step2(env)
    env.set_record(False)
    _plan(env, IDM_DEFAULT, 1024)
    env.close()


def test_recording_alone_runs(scns):
    env = _env(scns['idm'])
    env.set_record(True)
    _plan(env, (1024, 0, 1, 4, 0), 1024)
    _runs(env)
    env.close()


def test_lane_data_from_the_reset_on(scns):
    env = _env(scns['idm'])
    env.set_record(True)
    env.set_lane_data(60)
    _plan(env, (1024, 0, 1, 4, 0), 1024)           # armed, not live
    _runs(env)
    _plan(env, (1024, 0, 1, 4, -4), 1024)
    env.set_lane_data(0)
    _plan(env, (1024, 0, 1, 4, 0), 1024)
    _step2(env)
    env.close()


def test_krauss_from_the_reset_on(scns):
    env = _env(scns['krauss'])                     # (the constructor has called tsc_env_set_car_following)
    _plan(env, IDM_DEFAULT, 1024)
    _runs(env)
    p = _plan(env, (256, 1, 0, 1, -1), 256)
    for n in (1, _cus() + 1, 2 * _cus() + 1):      # Krauss ignores the device's load
        _resident(env, n)
        assert env.step_plan() == p
    _step2(env)
    env.close()


def test_krauss_recording_and_trace(scns):
    env = _env(scns['krauss'])
    env.set_record(True)
    env.set_trace([1], row_cap=1 << 12)
    _runs(env)
    _plan(env, (256, 0, 1, 1, -3), 256)
    env.set_trace([])
    _plan(env, (256, 0, 1, 1, -1), 256)
    _step2(env)
    env.close()


def test_krauss_lane_data(scns):
    env = _env(scns['krauss'])
    env.set_record(True)
    env.set_lane_data(60)
    _plan(env, (1024, 0, 1, 4, 0), 1024)           # neither Krauss nor the lane data before the reset
    _runs(env)
    _plan(env, (256, 0, 1, 1, -5), 256)
    env.close()


@pytest.mark.parametrize('model,knobs,row,threads', [
    ('idm', dict(TSC_ENV_SPEC='0'), (256, 1, 0, 1, 0), 256),
    ('idm', dict(TSC_ENV_SPEC='0', TSC_ENV_KF='2'), (256, 1, 0, 2, 0), 256),
    ('idm', dict(TSC_ENV_SPEC='0', TSC_ENV_KF='4'), (256, 1, 0, 4, 0), 256),
    ('idm', dict(TSC_ENV_SPEC='0', TSC_ENV_THREADS='512'), (1024, 1, 0, 4, 0), 512),
    ('idm', dict(TSC_ENV_SPEC='0', TSC_ENV_THREADS='512', TSC_ENV_KF='1'), (1024, 1, 0, 4, 0), 512),
    ('idm', dict(TSC_ENV_THREADS='320'), (1024, 1, 0, 4, 0), 320),
    ('idm', dict(TSC_ENV_KF='4'), (256, 1, 0, 4, 0), 256),
    ('idm', dict(TSC_ENV_HELP='0'), (256, 0, 0, 4, 0), 128),
    ('krauss', dict(TSC_ENV_KF='2'), (256, 1, 0, 2, -1), 256),
    ('krauss', dict(TSC_ENV_THREADS='1024', TSC_ENV_KF='2'), (1024, 1, 0, 1, -1), 1024),
    ('krauss', dict(TSC_ENV_HELP='0'), (256, 0, 0, 1, -1), 128),
], ids=lambda v: '-'.join('%s=%s' % (k[8:], x) for k, x in v.items()) if isinstance(v, dict) else None)
def test_knobs(scns, model, knobs, row, threads, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    env = _env(scns[model])
    if model == 'idm':
        _plan(env, row, threads)
    _runs(env)
    _plan(env, row, threads)
    env.close()


def test_monaco_gets_its_own_dimensions():
    env = _env(build_real_net('ma2c'))
    _plan(env, (1024, 1, 0, 1, 2), 1024)
    _runs(env)
    env.close()


def test_single_env_adaptor(scns):
    from deeprl_signal_control_amd.env import TrafficEnv
    env = TrafficEnv(scns['idm'], seed=12)
    assert env.step_plan() == env.vec.step_plan() and env.step_plan()['row'] == IDM_DEFAULT
    env.close()
