"""bench.py's plain run (no --full) on the device: it times exactly --steps iterations, its line carries the headline fields
and nothing that needs further passes, and --dump-outputs writes what the last timed iteration computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_iteration(tmp_path):
    out = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--envs', '64',
           '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d
    assert d['steps'] == 2 and d['warmup'] == 1 and d['dtype'] == 'f32' and d['higher_is_better'] is True
    # value = agents x instances x simulated seconds of the timed steps / their wall time
    assert abs(d['value'] - 25 * 64 * 120 * 5 / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    assert not {'roofline', 'kernels', 'cpu_baseline'} & set(d) and set(d['extra']) == {'ranks'}
    a = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert set(a) == {'params', 'grad', 'obs', 'action', 'value', 'reward', 'done'}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a['obs'].shape[:2] == (64, 25) and a['action'].shape == (120, 64, 25) and a['done'].shape == (120, 64)
    assert (a['action'] == np.round(a['action'])).all() and 0 <= a['action'].min() and a['action'].max() < 5
    assert set(np.unique(a['done'])) <= {0.0, 1.0} and np.abs(a['params']).max() > 0
