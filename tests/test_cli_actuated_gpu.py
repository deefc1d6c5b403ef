"""`evaluate --agents actuated,sotl,fixedtime`: the actuated and SOTL controllers through the command line.  Every table is named and
labelled with the controller's own name; DIR/<name>/data/*.ini supplies the config."""
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
episode_length_sec = 1200
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
fixed_time_steps = 6
actuated_min_green = 2
actuated_max_green = 8
actuated_gap_sec = 3.0
sotl_min_green = 2
sotl_theta = 20
sotl_mu = 2
sotl_omega = 25.0
"""


def runs(actions):
    """Lengths of the runs of equal values, the last (cut by the episode's end) left out."""
    out, n = [], 1
    for x, y in zip(actions, actions[1:]):
        if x == y:
            n += 1
        else:
            out.append(n)
            n = 1
    return out


def test_evaluate_actuated_and_sotl(tmp_path):
    import pandas as pd
    from deeprl_signal_control_amd import main as cli
    base = str(tmp_path)
    names = ('actuated', 'sotl', 'fixedtime')
    for name in names:
        os.makedirs(base + '/%s/data' % name)
        with open(base + '/%s/data/config.ini' % name, 'w') as fh:
            fh.write(INI)
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', ','.join(names), '--evaluation-seeds', '10000,20000'])
    control = {}
    for name in names:
        mean, _ = out[name]
        assert mean.shape == (2,) and (mean < 0).all()
        c = pd.read_csv(base + '/eva_data/large_grid_%s_control.csv' % name, index_col=0)
        assert len(c) == 2 * 240 and sorted(c.episode.unique()) == [1, 2]          # 240 control rows per seed
        t = pd.read_csv(base + '/eva_data/large_grid_%s_traffic.csv' % name, index_col=0)
        assert len(t) == 2 * 1200
        tr = pd.read_csv(base + '/eva_data/large_grid_%s_trip.csv' % name, index_col=0)
        assert len(tr) > 100 and set(tr.episode.unique()) == {1, 2}
        control[name] = c
    assert sorted({f.split('_')[2] for f in os.listdir(base + '/eva_data')}) == sorted(names)      # nothing under another name
    for name in ('actuated', 'sotl'):
        assert (control[name].action != control['fixedtime'].action).any()
        n_runs = 0
        # every agent's phase runs last at least min_green = 2 control steps -- but for the run the episode begins with: reset() frees
        # the first decision (cur = 0, age = min_green), so phase 0 may be kept for one step and left at the second
        for ep in (1, 2):
            rows = [[int(x) for x in s.split(',')] for s in control[name][control[name].episode == ep].action]
            for a in range(25):
                r = runs([row[a] for row in rows])[1:]
                assert all(n >= 2 for n in r), (name, ep, a, r)     # (junctions the traffic has not reached keep phase 0: no run)
                n_runs += len(r)
        assert n_runs > 25 * 2 * 5                          # and the phases do change
    assert (control['actuated'].action != control['sotl'].action).any()
