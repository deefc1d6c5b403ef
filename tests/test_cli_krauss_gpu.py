"""[ENV_CONFIG] car_following = krauss through the command line: `train` builds its env with the Krauss model, and `evaluate`
rebuilds the env from the config copied into the agent's data/ directory, so an agent trained under Krauss is evaluated under
Krauss."""
import os

import numpy as np
import pytest

from tests.test_cli_gpu import INI

pytestmark = pytest.mark.gpu


def test_train_then_evaluate_under_krauss(tmp_path, monkeypatch):
    from deeprl_signal_control_amd import env as env_mod
    from deeprl_signal_control_amd import main as cli
    seen = []
    close = env_mod.VecTrafficEnv.close

    def recording_close(self):                      # the model each env ran with, read before its handle goes
        if getattr(self, '_h', None) is not None:
            seen.append((self.E, self.car_following()))
        close(self)
    monkeypatch.setattr(env_mod.VecTrafficEnv, 'close', recording_close)
    ini = (INI % {'agent': 'ma2c'}).replace('[ENV_CONFIG]\n', '[ENV_CONFIG]\ncar_following = krauss\nkrauss_sigma = 0.5\n')
    cfg = tmp_path / 'config_ma2c.ini'
    cfg.write_text(ini)
    base = str(tmp_path / 'exp')
    cli.main(['--base-dir', base + '/ma2c', 'train', '--config-dir', str(cfg), '--envs', '4'])
    assert os.path.exists(base + '/ma2c/model/checkpoint-120.npz')
    assert (4, ('krauss', 0.5)) in seen
    seen.clear()
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'ma2c', '--evaluation-seeds', '10000,20000'])
    mean, _ = out['ma2c']
    assert mean.shape == (2,) and np.isfinite(mean).all() and (mean < 0).all()
    assert seen == [(2, ('krauss', 0.5))]                    # the evaluation env reports Krauss
    log = open(os.path.join(base, 'eva_log', os.listdir(os.path.join(base, 'eva_log'))[0])).read()
    assert 'car following krauss (sigma 0.5)' in log
