"""Multi-step returns through the command line: `train` of iqld on small_grid with return_steps = 3 in the INI needs nothing else -- it
runs its updates and writes a checkpoint with exactly the keys it would have without the option (the parameters mean the same under
every horizon), and a model whose config has no such key loads that checkpoint."""
import os

import numpy as np
import pytest

from tests.iql_harness import INI

pytestmark = pytest.mark.gpu


def test_train_with_return_steps_then_load_without(tmp_path):
    from deeprl_signal_control_amd import main as cli
    from tests.iql_harness import model
    ini = INI.replace('target_update = 5\n', 'target_update = 5\nreturn_steps = 3\n')
    assert all(line in ini for line in ('return_steps = 3', 'double_q = 1', 'agent = iqld', 'scenario = small_grid'))
    cfg = tmp_path / 'config_iqld.ini'
    cfg.write_text(ini)
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/iqld', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', '4'])
    assert len(rows) > 0
    ck = base + '/iqld/model/checkpoint-120.npz'
    assert os.path.exists(ck)
    z = np.load(ck)
    assert sorted(z.files) == ['adam_m', 'adam_v', 'counters', 'format', 'layout', 'params', 'target']      # no key of its own
    assert int(z['counters'][0]) >= 2 and int(z['counters'][2]) >= 2                                      # Adam steps, minibatch draws
    # a model without the key (and one with another horizon) loads the file; `evaluate` runs on it
    for kw in ({}, dict(return_steps=5)):
        _, m = model('small_grid', 'iqld', 'dqn', 2, seed=9, target_update=5, double_q=1, **kw)
        assert m.return_steps == kw.get('return_steps', 1)
        assert m.load(base + '/iqld/model')
        np.testing.assert_array_equal(m.get_flat(), z['params'])
        np.testing.assert_array_equal(m.get_target_flat(), z['target'])
        m.close()
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'iqld', '--evaluation-seeds', '10000'])
    mean, std = out['iqld']
    assert mean.shape == (1,) and mean[0] < 0
