#!/usr/bin/env python
"""Cost of the Krauss car following (tsc_env_set_car_following) on the env kernel: sim-only greedy large_grid episodes at E = 1024
for IDM on the specialised kernel, IDM on the runtime-dimension kernel (TSC_ENV_SPEC=0) and Krauss with sigma = 0 / 0.5 (runtime
dimensions).  Each setting runs in a child process of its own, once timed with CUDA events around whole episodes and once under
`rocprofv3 --kernel-trace --stats` for the kernel time.  V-bar = mean live vehicles per instance over the timed episodes: dawdling
adds traffic, so step times compare only at equal V-bar, and sigma = 0 isolates the cost of the serial word.

    python tools/bench_krauss.py [--out profiles/krauss_bench.json] [--episodes 3] [--no-rocprof]
    python tools/bench_krauss.py run SETTING E EPISODES        (one child: prints one JSON line)"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {'idm_spec': ({}, 'idm', 0.0), 'idm_spec0': ({'TSC_ENV_SPEC': '0'}, 'idm', 0.0),
            'krauss_sigma0': ({}, 'krauss', 0.0), 'krauss_sigma0.5': ({}, 'krauss', 0.5)}


def child(setting, E, episodes):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_large_grid
    _, model, sigma = SETTINGS[setting]
    kw = dict(car_following=model, krauss_sigma=sigma) if model != 'idm' else {}
    scn = build_large_grid('greedy', **kw)
    env = VecTrafficEnv(scn, E, seed=12)
    T = int(env.T)
    res = []
    for ep in range(episodes + 1):                              # episode 0 warms up
        env.reset()
        env.live_vehicle_mean(1, reset=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(T):
            env.step(env.greedy_actions())
        b.record()
        torch.cuda.synchronize()
        if ep:
            res.append((a.elapsed_time(b) * 1e3 / T, env.live_vehicle_mean(T)))
    us = float(np.median([r[0] for r in res]))
    out = dict(setting=setting, model=env.car_following()[0], sigma=env.car_following()[1], E=E,
               us_per_control_step=us, env_steps_per_s=25 * E * scn.control_interval_sec / (us * 1e-6),
               mean_live_vehicles=float(np.mean([r[1] for r in res])), episodes=episodes, control_steps_per_episode=T)
    env.close()
    print(json.dumps(out))


def kernel_stats(d):
    rows = {}
    for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        import csv
        for r in csv.DictReader(open(f)):
            rows[r['Name']] = dict(calls=int(r['Calls']), total_ns=float(r['TotalDurationNs']), avg_ns=float(r['AverageNs']))
    return rows


def main():
    args = sys.argv[1:]
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'krauss_bench.json')
    episodes = int(args[args.index('--episodes') + 1]) if '--episodes' in args else 3
    E = 1024
    results = {}
    for name, (env_over, _, _) in SETTINGS.items():
        env = dict(os.environ, **env_over)
        cmd = [sys.executable, os.path.abspath(__file__), 'run', name, str(E), str(episodes)]
        p = subprocess.run(['timeout', '-k', '10', '300'] + cmd, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit('%s failed (%d):\n%s' % (name, p.returncode, p.stderr[-3000:]))
        r = json.loads(p.stdout.strip().splitlines()[-1])
        if '--no-rocprof' not in args:
            d = tempfile.mkdtemp(prefix='krauss_prof_')
            try:
                p = subprocess.run(['timeout', '-k', '10', '400', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv',
                                    '-d', d, '-o', name, '--'] + cmd[:-1] + ['1'], env=env, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.exit('%s under rocprofv3 failed (%d):\n%s' % (name, p.returncode, p.stderr[-3000:]))
                st = kernel_stats(d)
            finally:
                shutil.rmtree(d, ignore_errors=True)
            step = {k: v for k, v in st.items() if 'step_kernel' in k}
            r['rocprof_step_kernels'] = step
            calls = sum(v['calls'] for v in step.values())
            r['rocprof_step_kernel_avg_us'] = sum(v['total_ns'] for v in step.values()) / max(calls, 1) / 1e3
            r['rocprof_greedy_kernel_avg_us'] = next((v['avg_ns'] / 1e3 for k, v in st.items() if 'greedy_kernel' in k), None)
        results[name] = r
        print(json.dumps(r), flush=True)
    json.dump(dict(scenario='large_grid', controller='greedy', E=E, note=__doc__.split('\n\n')[0], results=results), open(out, 'w'), indent=1)
    print('wrote', out)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
