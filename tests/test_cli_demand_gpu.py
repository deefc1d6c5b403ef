"""Per-instance demand through the command line: `train` with [ENV_CONFIG] demand_scales / demand_jitter is reproducible and leaves
a run without the keys what it was; `evaluate --demand-scales` runs seeds x scales as one batched episode and marks every table."""
import os
import shutil

import numpy as np
import pytest

from tests.test_cli_gpu import INI

pytestmark = pytest.mark.gpu

DEMAND_KEYS = 'demand_scales = 0.6,0.8,1.0,1.2\ndemand_jitter = 0.15\n'


def _train(tmp_path, tag, ini):
    from deeprl_signal_control_amd import main as cli
    cfg = tmp_path / ('config_%s.ini' % tag)
    cfg.write_text(ini)
    base = str(tmp_path / tag)
    cli.main(['--base-dir', base, 'train', '--config-dir', str(cfg), '--envs', '8'])
    csv = open(base + '/data/train_reward.csv').read()
    ck = np.load(base + '/model/checkpoint-120.npz')
    logs = ''.join(open(os.path.join(base, 'log', f)).read() for f in sorted(os.listdir(base + '/log')))
    return csv, {k: ck[k] for k in ck.files}, logs


def test_train_with_sampled_demand(tmp_path):
    ini = INI % {'agent': 'ma2c'}
    with_keys = ini + DEMAND_KEYS
    a = _train(tmp_path, 'a', with_keys)
    b = _train(tmp_path, 'b', with_keys)
    p = _train(tmp_path, 'p', ini)
    q = _train(tmp_path, 'q', ini)
    assert a[0] == b[0] and p[0] == q[0]                           # same seed, same files
    for x, y in ((a, b), (p, q)):
        assert sorted(x[1]) == sorted(y[1])
        for k in x[1]:
            np.testing.assert_array_equal(x[1][k], y[1][k], err_msg=k)
    assert a[0] != p[0]                                            # the demand was different
    assert a[0].splitlines()[0] == p[0].splitlines()[0] == ',agent,avg_reward,std_reward,step,test_id'
    assert 'per-instance demand, scales 0.6,0.8,1,1.2, jitter 0.15' in a[2] and 'mean demand scale' in a[2]
    assert 'demand' not in p[2]                                    # without the keys nothing is built, nothing is logged
    # without the keys no sampler is built, so train() constructs the handle exactly as before
    import configparser
    from deeprl_signal_control_amd.env import demand_from_config, scenario_from_config
    c = configparser.ConfigParser()
    c.read_string(ini)
    scn, _, _ = scenario_from_config(c['ENV_CONFIG'])
    assert demand_from_config(c['ENV_CONFIG'], scn) is None


def test_evaluate_demand_scales(tmp_path):
    import pandas as pd
    from deeprl_signal_control_amd import main as cli
    cfg = tmp_path / 'config_greedy.ini'
    cfg.write_text(INI % {'agent': 'greedy'})

    def run(tag, *flags):
        base = str(tmp_path / tag)
        os.makedirs(base + '/greedy/data')
        shutil.copy(str(cfg), base + '/greedy/data/')
        out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'greedy', '--evaluation-seeds', '10000,20000',
                        '--trajectories', '1', '--lane-data', '300'] + list(flags))
        tabs = {k: pd.read_csv(base + '/eva_data/large_grid_greedy_%s.csv' % k, index_col=0)
                for k in ('control', 'traffic', 'trip', 'fcd', 'lanedata')}
        raw = {k: open(base + '/eva_data/large_grid_greedy_%s.csv' % k).read() for k in tabs}
        return out['greedy'], tabs, raw
    (mean, _), tabs, _ = run('scaled', '--demand-scales', '0.8,1.2')
    assert mean.shape == (4,)
    for k, df in tabs.items():
        assert 'demand_scale' in df.columns, k
        want = {1: 0.8, 2: 0.8, 3: 1.2, 4: 1.2} if k != 'fcd' else {1: 0.8, 3: 1.2}        # (--trajectories 1: the first seed of each scale)
        got = {int(ep): set(g.demand_scale) for ep, g in df.groupby('episode')}
        assert got == {ep: {s} for ep, s in want.items()}, k
    t = tabs['traffic']
    dep = t.groupby('episode').number_departed_car.sum()
    assert dep[3] > 1.3 * dep[1] and dep[4] > 1.3 * dep[2]          # 1.2 / 0.8 = 1.5 times the vehicles
    # scale 1.0 alone: the flag-less tables plus the column; and the flag-less files are the plain ones (no such column)
    _, one, _ = run('one', '--demand-scales', '1.0')
    (mean0, _), plain, raw0 = run('plain')
    _, plain2, raw1 = run('plain2')
    assert raw0 == raw1
    for k in plain:
        assert 'demand_scale' not in plain[k].columns, k
        assert set(one[k].demand_scale) == {1.0}, k
        pd.testing.assert_frame_equal(one[k].drop(columns='demand_scale'), plain[k], check_exact=True)
