"""Parameter sharing through the command line: `train` of ma2c on small_grid with share_params = 1 in the INI needs nothing else -- it
runs, its checkpoint carries the class list (3 + 2 + 1) and parameters that are bit-identical inside every class, and `evaluate` rebuilds
the shared model from the config copied into the agent's data/ directory and loads the checkpoint."""
import os

import numpy as np
import pytest

from tests.test_cli_gpu import INI

pytestmark = pytest.mark.gpu


def test_train_then_evaluate_with_shared_parameters(tmp_path):
    from deeprl_signal_control_amd import main as cli
    ini = INI % {'agent': 'ma2c'}
    for old, new in (('[MODEL_CONFIG]\n', '[MODEL_CONFIG]\nshare_params = 1\n'), ('reward_norm = 2000.0\n', 'reward_norm = 100.0\n'),
                     ('data_path = ./large_grid/data/\n', 'data_path = ./small_grid/data/\n'),
                     ('peak_flow1 = 1100\npeak_flow2 = 925\ninit_density = 0\n', 'num_extra_car_per_hour = 1000\n'),
                     ('scenario = large_grid\n', 'scenario = small_grid\n')):
        assert old in ini
        ini = ini.replace(old, new)
    cfg = tmp_path / 'config_ma2c.ini'
    cfg.write_text(ini)
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/ma2c', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', '4'])
    assert len(rows) > 0
    ck = base + '/ma2c/model/checkpoint-120.npz'
    assert os.path.exists(ck)
    z = np.load(ck)
    share = [int(x) for x in z['share']]
    assert len(share) == 6 and sorted((share.count(c) for c in set(share)), reverse=True) == [3, 2, 1]
    assert all(share[c] == c and c <= a for a, c in enumerate(share))
    p, ms = z['params'].reshape(6, -1), z['ms'].reshape(6, -1)
    for a, c in enumerate(share):
        np.testing.assert_array_equal(p[a].view(np.uint32), p[c].view(np.uint32))
        np.testing.assert_array_equal(ms[a].view(np.uint32), ms[c].view(np.uint32))
    assert (ms != 1).any()                                  # six updates ran
    with open(base + '/ma2c/log/%s' % sorted(os.listdir(base + '/ma2c/log'))[0]) as f:
        assert 'parameter sharing, 6 agents in 3 classes of 3 + 2 + 1 members' in f.read()
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'ma2c', '--evaluation-seeds', '10000'])
    mean, std = out['ma2c']
    assert mean.shape == (1,) and mean[0] < 0
