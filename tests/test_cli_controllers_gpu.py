"""`evaluate --agents greedy,maxpressure,fixedtime`: the controllers without a learner through the command line.  Every table is
named and labelled with the controller's own name; DIR/<name>/data/*.ini supplies the config."""
import os

import pytest

pytestmark = pytest.mark.gpu

INI = """
[MODEL_CONFIG]
policy = greedy

[ENV_CONFIG]
clip_wave = 2.0
clip_wait = 2.0
control_interval_sec = 5
agent = greedy
coop_gamma = 0.9
episode_length_sec = 3600
norm_wave = 5.0
norm_wait = 100.0
coef_wait = 0.2
peak_flow1 = 1100
peak_flow2 = 925
init_density = 0
objective = hybrid
scenario = large_grid
seed = 12
test_seeds = 10000,20000
yellow_interval_sec = 2
pressure_measure = count
pressure_min_green = 2
fixed_time_steps = 6
"""


def test_evaluate_controllers(tmp_path):
    import pandas as pd
    from deeprl_signal_control_amd import main as cli
    base = str(tmp_path)
    names = ('greedy', 'maxpressure', 'fixedtime')
    for name in names:
        os.makedirs(base + '/%s/data' % name)
        with open(base + '/%s/data/config.ini' % name, 'w') as fh:
            fh.write(INI)
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', ','.join(names), '--evaluation-seeds', '10000,20000',
                    '--lane-data', '300'])
    control = {}
    for name in names:
        mean, _ = out[name]
        assert mean.shape == (2,) and (mean < 0).all()
        c = pd.read_csv(base + '/eva_data/large_grid_%s_control.csv' % name, index_col=0)
        assert len(c) == 2 * 720 and sorted(c.episode.unique()) == [1, 2]          # 720 control rows per seed
        t = pd.read_csv(base + '/eva_data/large_grid_%s_traffic.csv' % name, index_col=0)
        assert len(t) == 2 * 3600
        tr = pd.read_csv(base + '/eva_data/large_grid_%s_trip.csv' % name, index_col=0)
        assert len(tr) > 100 and set(tr.episode.unique()) == {1, 2}
        ld = pd.read_csv(base + '/eva_data/large_grid_%s_lanedata.csv' % name, index_col=0)
        assert len(ld) % (2 * 12) == 0 and len(ld) > 0 and sorted(ld.episode.unique()) == [1, 2]      # 12 intervals of 300 s per seed
        control[name] = c
    assert (control['maxpressure'].action != control['greedy'].action).any()
    # the fixed-time cycle: 6 control steps per phase, five phases at every intersection
    first = control['fixedtime'][control['fixedtime'].episode == 1].action.tolist()
    assert first[:13] == [','.join(['%d' % ((t // 6) % 5)] * 25) for t in range(13)]
    assert all(f.split('_')[2] in names for f in os.listdir(base + '/eva_data'))   # nothing is written under another name
