"""The full 3DQN through the command line: `train` of iqld on small_grid with dueling = 1, double_q = 1, target_update = 10 and
prioritized_replay = 1 in the INI needs nothing else -- it runs, its checkpoint carries the dueling flag (and theta-, and the beta
counter), `evaluate` loads it."""
import os

import numpy as np
import pytest

from tests.iql_harness import INI

pytestmark = pytest.mark.gpu


def test_train_then_evaluate_with_the_dueling_head(tmp_path):
    from deeprl_signal_control_amd import main as cli
    ini = INI.replace('target_update = 5\n', 'target_update = 10\nprioritized_replay = 1\ndueling = 1\n')
    assert all(line in ini for line in ('dueling = 1', 'double_q = 1', 'target_update = 10', 'prioritized_replay = 1', 'agent = iqld',
                                        'scenario = small_grid'))
    cfg = tmp_path / 'config_iqld.ini'
    cfg.write_text(ini)
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/iqld', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', '4'])
    assert len(rows) > 0
    ck = base + '/iqld/model/checkpoint-120.npz'
    assert os.path.exists(ck)
    z = np.load(ck)
    assert 'dueling' in z.files and int(z['dueling']) == 1
    assert 'target' in z.files and z['target'].shape == z['params'].shape and 'per_n' in z.files
    assert int(z['counters'][0]) > 0
    # the value stream was trained: column 7 of every agent's head bias has left its zero initialisation
    lay = [int(x) for x in z['layout']]
    A, stride, obq = lay[0], lay[1], lay[9]
    assert (z['params'].reshape(A, stride)[:, obq + 7] != 0).all()
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'iqld', '--evaluation-seeds', '10000'])
    mean, std = out['iqld']
    assert mean.shape == (1,) and mean[0] < 0
