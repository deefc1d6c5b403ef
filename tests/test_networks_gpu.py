"""step_kernel / reset_kernel (csrc/tsc_env.hip) against the CPU oracle on the synthetic networks of tests/networks.py: every declared
limit of tsc_env_create from the inside -- the wide runtime-dimension kernel, the table-copy fallback, the stride loops of the
prologue, four feeders, link 62, control intervals 8 / 3 and 1 / 0, several vehicles a second from one stream, feeder bytes up to 253,
more than 128 agents under np.sum's order -- and from the outside only where the host refuses (nothing past a limit is ever launched).

Nothing here has a tolerance: the simulator's contract is bit equality with the oracle.  tests/test_networks_host.py states, on the
oracle alone, that each of these runs reaches the limit it is named for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import env_harness as H
from tests import networks as nw
from tests.env_harness import oracle_krauss

pytestmark = pytest.mark.gpu


def _compare(name, monkeypatch, plan=None, env=None, scn=None, train_mode=True, record=False):
    """The one comparison of this module (env_harness.compare_with_oracle) over the registry entry `name`.
    plan: what step_plan() must report after the first reset (row + threads); env: TSC_ENV_* variables on top of the entry's own;
    scn: a variant of the entry's scenario (Krauss: inside oracle_krauss)."""
    net = nw.NETWORKS[name]
    return H.compare_with_oracle(net.scenario() if scn is None else scn, net, monkeypatch, plan=plan, env=env, train_mode=train_mode,
                                 record=record)


@pytest.mark.parametrize('name', list(nw.NETWORKS))
def test_network_vs_oracle_with_the_librarys_own_plan(name, monkeypatch):
    """Every network of the registry under the plan the library chooses for it, which is the one written next to it."""
    _compare(name, monkeypatch, plan=nw.NETWORKS[name].plan)


def test_grid_x2_at_512_threads(monkeypatch):
    """The copy_words fallback with another stride: the 4-wide flat phase of the wide runtime-dimension kernel at 512 threads."""
    _compare('grid_x2', monkeypatch, plan=(1024, 1, 0, 4, 0, 512), env={'TSC_ENV_THREADS': '512'})


def test_isolated_130_ma2c_shaping_with_neighbours(monkeypatch):
    """More than 128 agents as MA2C: the neighbour-discounted rewards and the fingerprints of 130 agents."""
    _compare('isolated_130', monkeypatch, plan=nw.NETWORKS['isolated_130'].plan, scn=nw.isolated(130, agent='ma2c', objective='hybrid'))


def test_isolated_130_test_mode_returns_local_rewards(monkeypatch):
    """train_mode = 0: the local rewards of 130 agents (and np.sum of them as the global reward)."""
    _compare('isolated_130', monkeypatch, train_mode=False)


@pytest.mark.parametrize('name,plan', [('grid_x4', (1024, 1, 0, 1, -1, 384)), ('merge4_zipper', (256, 1, 0, 1, -1, 256)),
                                       ('merge4_yield', (256, 1, 0, 1, -1, 256))])
def test_krauss_on_the_wide_kernel_and_the_four_way_merge(name, plan, monkeypatch):
    import copy
    scn = copy.copy(nw.NETWORKS[name].scenario())
    scn.car_following, scn.krauss_sigma = 'krauss', 0.5
    with oracle_krauss(0.5):
        _compare(name, monkeypatch, plan=plan, scn=scn)


@pytest.mark.parametrize('name,plan', [('grid_x2', (256, 0, 1, 4, 0, 256)), ('ctrl8', (256, 0, 1, 4, 0, 256))])
def test_recording_rows_and_trip_log(name, plan, monkeypatch):
    """The recording walk: per-second rows (ctrl8 is the only run that fills all eight of a launch), control rows and the trip log
    against the oracle's, the way tests/test_eval_outputs.py and tests/test_krauss_gpu.py compare them."""
    tot = _compare(name, monkeypatch, plan=plan, record=True)
    assert min(x['arrived'] for x in tot) > 100


def _create(scn, monkeypatch=None):
    """tsc_env_create on a scenario Scenario.check_limits would stop first (the binding calls it): -> (rc, error text)."""
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.scenario import Scenario
    if monkeypatch is not None:
        monkeypatch.setattr(Scenario, 'check_limits', lambda self: self)
    L = _lib.lib()
    sc, keep = _lib.scenario_struct(scn)
    h = C.c_void_p()
    rc = L.tsc_env_create(C.byref(sc), 2, 0, C.byref(h))
    text = L.tsc_last_error().decode() if rc else ''
    if rc == 0:
        L.tsc_env_destroy(h)
    return rc, text


@pytest.mark.parametrize('what', list(nw.REFUSED))
def test_refusals_name_the_limit_and_leave_the_library_usable(what, monkeypatch):
    """One step past every limit: tsc_env_create returns non-zero with the limit in tsc_last_error (host checks: nothing is
    launched), Scenario.check_limits refuses the same scenario (tests/test_networks_host.py), and a good scenario is created and
    stepped afterwards."""
    import re
    from deeprl_signal_control_amd.env import VecTrafficEnv
    make, host_text, lib_text = nw.REFUSED[what]
    scn = make()
    if host_text is not None:
        with pytest.raises(ValueError, match=host_text):
            scn.check_limits()
        with pytest.raises(ValueError, match=host_text):
            VecTrafficEnv(scn, 2)
    rc, text = _create(scn, monkeypatch)
    assert rc != 0 and re.search(lib_text, text), (rc, text)
    monkeypatch.undo()
    good = nw.NETWORKS['merge4_zipper'].scenario()
    dev = VecTrafficEnv(good, 2, seed=1)
    dev.reset()
    _, _, _, g = dev.step(torch.zeros(2, good.n_agent, dtype=torch.int32, device='cuda'))
    assert np.isfinite(g.cpu().numpy()).all()
    dev.close()
