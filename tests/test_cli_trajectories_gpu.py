"""evaluate --trajectories N: the greedy baseline on large_grid writes eva_data/large_grid_greedy_fcd.csv for the first N seeds, whose
rows per second match that episode's traffic table; without the flag no fcd file appears."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from tests.test_cli_gpu import INI

pytestmark = pytest.mark.gpu


def _evaluate(tmp_path, extra):
    from deeprl_signal_control_amd import main as cli
    cfg = tmp_path / 'config_greedy.ini'
    cfg.write_text(INI % {'agent': 'greedy'})
    base = str(tmp_path / 'exp')
    os.makedirs(base + '/greedy/data')
    shutil.copy(str(cfg), base + '/greedy/data/')
    out = cli.main(['--base-dir', base, 'evaluate', '--agents', 'greedy', '--evaluation-seeds', '10000,20000'] + extra)
    assert out['greedy'][0].shape == (2,)
    return base + '/eva_data/'


def test_evaluate_trajectories(tmp_path):
    eva = _evaluate(tmp_path, ['--trajectories', '1'])
    fcd = pd.read_csv(eva + 'large_grid_greedy_fcd.csv', index_col=0)
    assert list(fcd.columns) == ['episode', 'time_sec', 'id', 'lane', 'pos', 'speed']
    assert set(fcd['episode']) == {1}
    traffic = pd.read_csv(eva + 'large_grid_greedy_traffic.csv', index_col=0)
    ep1 = traffic[traffic['episode'] == 1]
    per_sec = fcd.groupby('time_sec').size().reindex(ep1['time_sec'], fill_value=0).to_numpy()
    np.testing.assert_array_equal(per_sec, ep1['number_total_car'].to_numpy())
    assert fcd['id'].str.match(r'^f_\d+\.\d+$').all()
    assert (fcd['pos'] >= 0).all() and (fcd['pos'] <= 200.0 + 1e-3).all() and (fcd['speed'] >= 0).all()
    trips = pd.read_csv(eva + 'large_grid_greedy_trip.csv', index_col=0)
    assert set(trips[trips['episode'] == 1]['id']) <= set(fcd['id'])


def test_evaluate_without_trajectories(tmp_path):
    eva = _evaluate(tmp_path, [])
    assert os.path.exists(eva + 'large_grid_greedy_traffic.csv')
    assert not os.path.exists(eva + 'large_grid_greedy_fcd.csv')
