"""`objective = pressure` through the command line: `train` learns on the pressure reward, `evaluate` writes it into the control
table, and the max-pressure controller evaluates from the same config."""
import os
import shutil

import numpy as np
import pytest

from tests.test_cli_gpu import INI

pytestmark = pytest.mark.gpu
E_TRAIN, T = 4, 60                     # instances; control steps of the 300 s episode


def test_train_then_evaluate_on_pressure(tmp_path):
    import configparser

    import pandas as pd
    import torch
    from deeprl_signal_control_amd import main as cli
    from deeprl_signal_control_amd.env import VecTrafficEnv, scenario_from_config
    from deeprl_signal_control_amd.trainer import pressure_reward
    ini = (INI % {'agent': 'ma2c'}).replace('objective = hybrid', 'objective = pressure').replace('total_step = 120', 'total_step = 60')
    assert 'objective = pressure' in ini and 'total_step = 60' in ini          # the config's only change (and one episode of it)
    cfg = tmp_path / 'config_ma2c.ini'
    cfg.write_text(ini)
    base = str(tmp_path / 'exp')
    rows = cli.main(['--base-dir', base + '/ma2c', 'train', '--config-dir', str(cfg), '--test-mode', 'no_test', '--envs', str(E_TRAIN)])
    assert os.path.exists(base + '/ma2c/model/checkpoint-60.npz')
    df = pd.read_csv(base + '/ma2c/data/train_reward.csv', index_col=0)
    train_rows = df[df.test_id == -1]
    assert len(train_rows) == len(rows) == 1 and list(train_rows.step) == [60]
    # avg_reward is the mean over T control steps and E instances of g = -sum |P|, before any reward_norm: a non-positive integer / (T E)
    total = float(train_rows.avg_reward.iloc[0]) * T * E_TRAIN
    assert total < 0 and abs(total - round(total)) < 1e-6 * abs(total), total
    # evaluate the trained agent and the max-pressure controller from the same config
    os.makedirs(base + '/maxpressure/data')
    shutil.copy(str(cfg), base + '/maxpressure/data/')
    seeds = [10000, 20000]
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'ma2c,maxpressure', '--evaluation-seeds', ','.join(map(str, seeds))])
    control = {}
    for name in ('ma2c', 'maxpressure'):
        mean, _ = out[name]
        assert mean.shape == (2,) and (mean < 0).all()
        control[name] = pd.read_csv(base + '/eva_data/large_grid_%s_control.csv' % name, index_col=0)
        assert len(control[name]) == 2 * T and sorted(control[name].episode.unique()) == [1, 2]
        assert len(pd.read_csv(base + '/eva_data/large_grid_%s_traffic.csv' % name, index_col=0)) == 2 * 300
    assert (control['maxpressure'].action != control['ma2c'].action).any()
    # the ma2c control table's reward is the sum of the local pressure rewards of the state its own actions lead to
    config = configparser.ConfigParser()
    config.read(str(cfg))
    scn, seed, _ = scenario_from_config(config['ENV_CONFIG'])
    env = VecTrafficEnv(scn, 2, seed=seed, test_seeds=seeds)
    env.train_mode = False
    env.reset(test_ind=np.arange(2))
    c = control['ma2c']
    per_episode = [c[c.episode == e + 1].sort_values('step') for e in range(2)]
    for t in range(T):
        act = np.array([[int(x) for x in per_episode[e].action.iloc[t].split(',')] for e in range(2)], np.int32)
        env.step(torch.from_numpy(act).cuda())
        for e in range(2):
            local, g, _ = pressure_reward(scn, env.get_state(e), 'count', train_mode=False)
            assert float(per_episode[e].reward.iloc[t]) == float(local.sum()) == g, (t, e)
    assert c.reward.min() < 0
    env.close()
