#!/usr/bin/env python
"""Cost of the lane data (tsc_env_lane_data) on the recording step kernel: greedy large_grid at E = 1024 and greedy Monaco at E = 512,
recording on, the same seeds everywhere, the step kernel's time from `rocprofv3 --kernel-trace --stats` (one child process per run,
nothing else traced).  Three settings, alternated within every repetition: the PARENT tree's recording kernel (a checkout of the
commit before the lane data, its library built; lane data does not exist there), this tree's recording kernel with lane data off, and
this tree with lane data on at a 300-s period.

    python tools/bench_lanedata.py --parent DIR [--out profiles/lanedata_bench.json] [--reps 3] [--steps 240]
    python tools/bench_lanedata.py run ROOT SCENARIO E STEPS PERIOD        (one child)"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (('large_grid', 1024), ('real_net', 512))


def child(root, scenario, E, steps, period):
    sys.path.insert(0, root)
    import numpy as np
    from deeprl_signal_control_amd import scenario as sc
    from deeprl_signal_control_amd.env import VecTrafficEnv
    scn = (sc.build_large_grid if scenario == 'large_grid' else sc.build_real_net)('greedy')
    env = VecTrafficEnv(scn, E, seed=12)
    env.set_record(True)
    if period:
        env.set_lane_data(period)
    env.is_record = False              # the device keeps recording; the host skips reading the per-second tables after each step
    env.reset()
    for _ in range(steps):
        env.step(env.greedy_actions())
    live = env.live_vehicle_mean(steps)
    env.close()
    print(json.dumps(dict(mean_live_vehicles=float(np.mean(live)))))


def kernel_stats(d):
    rows = {}
    for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[r['Name']] = dict(calls=int(r['Calls']), total_ns=float(r['TotalDurationNs']), avg_ns=float(r['AverageNs']))
    return rows


def one(root, scenario, E, steps, period, tag):
    cmd = [sys.executable, os.path.abspath(__file__), 'run', root, scenario, str(E), str(steps), str(period)]
    d = tempfile.mkdtemp(prefix='lanedata_prof_')
    try:
        p = subprocess.run(['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv',
                            '-d', d, '-o', tag, '--'] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit('%s under rocprofv3 failed (%d):\n%s' % (tag, p.returncode, p.stderr[-3000:]))
        st = kernel_stats(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    step = {k: v for k, v in st.items() if 'step_kernel' in k}
    calls = sum(v['calls'] for v in step.values())
    r = json.loads(p.stdout.strip().splitlines()[-1])
    r.update(step_kernel_avg_us=sum(v['total_ns'] for v in step.values()) / max(calls, 1) / 1e3, step_kernel_calls=calls,
             step_kernels=sorted(step))
    return r


def main():
    args = sys.argv[1:]
    if '--parent' not in args:
        sys.exit(__doc__)
    parent = os.path.abspath(args[args.index('--parent') + 1])
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'lanedata_bench.json')
    reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 3
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else 240
    settings = (('parent', parent, 0), ('off', ROOT, 0), ('on300', ROOT, 300))
    results = {}
    for scenario, E in CASES:
        runs = {name: [] for name, _, _ in settings}
        for rep in range(reps):
            for name, root, period in settings:
                r = one(root, scenario, E, steps, period, '%s_%s_%d' % (scenario, name, rep))
                runs[name].append(r)
                print(scenario, E, name, rep, json.dumps(r), flush=True)
        us = {name: [r['step_kernel_avg_us'] for r in rs] for name, rs in runs.items()}
        med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
        results[scenario] = dict(E=E, control_steps=steps, step_kernel_avg_us=us, median_us=med,
                                 ratio_on300_to_parent=med['on300'] / med['parent'], ratio_off_to_parent=med['off'] / med['parent'],
                                 mean_live_vehicles={name: [r['mean_live_vehicles'] for r in rs] for name, rs in runs.items()},
                                 step_kernels={name: rs[0]['step_kernels'] for name, rs in runs.items()})
        print(scenario, json.dumps(results[scenario]['median_us']), flush=True)
    json.dump(dict(controller='greedy', ceiling=1.10, note=__doc__.split('\n\n')[0], results=results), open(out, 'w'), indent=1)
    print('wrote', out)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        main()
