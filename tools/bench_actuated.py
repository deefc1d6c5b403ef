#!/usr/bin/env python
"""Measurements of the actuated and SOTL controllers.

    python tools/bench_actuated.py kernel [--parent-root DIR] [--rounds 5] [--json profiles/actuated_bench.json]
    python tools/bench_actuated.py eval [--json profiles/actuated_eval.json]

kernel: actuated_kernel under both rules and pressure_kernel (count) alone (tsc_profile_select on their ids), on one handle of
large_grid at E = 1024 and one of Monaco at E = 512, each on the state after 120 greedy-controlled control steps.  Every round starts
a fresh process per library, arms each controller in turn (the order rotates from round to round), warms it up and times 100 calls.
--parent-root names a checkout of the parent commit with its library built: its pressure_kernel, measured the same way in processes
that alternate with this library's, is the yardstick -- the new kernel walks the incoming lanes only and adds one LDS atomic per
vehicle.  Reported: the median over the rounds per arm, the parent's spread ((max - min) / median over its rounds) and each arm's
ratio to the parent's median.
eval: `evaluate` for greedy, fixedtime, maxpressure, actuated and sotl with their default keys, on large_grid (evaluation seeds
10000, 20000) and Monaco (10000, 20000, 30000): mean step reward, arrived vehicles (rows of the trip table) and teleports (trips the
teleport surrogate truncated).  Context, not a ranking: the vehicle dynamics are not pinned against SUMO and no default is tuned."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (('large_grid', 1024), ('real_net', 512))
ARMS = ('pressure', 'actuated', 'sotl')
TRAFFIC_STEPS, WARM_UP, TIMED = 120, 20, 100


def child(args):
    """One process, one library: the handle, the traffic, then every arm once -> one JSON line {arm: microseconds per call}."""
    sys.path.insert(0, args.package_root or ROOT)
    import torch
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(args.scenario, 'greedy')
    E = args.envs
    env = VecTrafficEnv(scn, E, seed=12)
    obs = env.reset()
    act = torch.zeros(E, scn.n_agent, dtype=torch.int32, device='cuda')
    for _ in range(TRAFFIC_STEPS):
        obs = env.step(env.greedy_actions(obs, out=act))[0]
    call = {'pressure': lambda: env.max_pressure_actions(out=act, measure='count'),
            'actuated': lambda: env.actuated_actions(out=act), 'sotl': lambda: env.sotl_actions(out=act)}
    out = dict(live_vehicles=env.mean_live_vehicles())
    for arm in args.arms.split(','):
        for _ in range(WARM_UP):                                   # (the first call arms the tables)
            call[arm]()
        _lib.profile_select(['pressure' if arm == 'pressure' else 'actuated'])
        _lib.profile(enable=True, reset=True)
        for _ in range(TIMED):
            call[arm]()
        p = _lib.profile()
        _lib.profile(enable=False)
        ms, n = p['pressure' if arm == 'pressure' else 'actuated']
        out[arm] = 1e3 * ms / n
    _lib.profile_select(None)
    env.close()
    print('RESULT ' + json.dumps(out), flush=True)


def run_child(scenario, envs, arms, package_root=None):
    cmd = [sys.executable, os.path.abspath(__file__), 'child', '--scenario', scenario, '--envs', str(envs), '--arms', ','.join(arms)]
    if package_root:
        cmd += ['--package-root', os.path.abspath(package_root)]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    return json.loads([ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1][7:])


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def kernel(args):
    out = dict(traffic_steps=TRAFFIC_STEPS, warm_up_calls=WARM_UP, timed_calls=TIMED, rounds=args.rounds, unit='microseconds per call',
               parent_library=bool(args.parent_root))
    for scenario, envs in CASES:
        runs = {arm: [] for arm in ARMS}
        parent, live = [], None
        for k in range(args.rounds):
            order = ['new', 'parent'] if k % 2 == 0 else ['parent', 'new']
            for which in order:
                if which == 'new':
                    res = run_child(scenario, envs, ARMS[k % 3:] + ARMS[:k % 3])
                    live = res['live_vehicles']
                    for arm in ARMS:
                        runs[arm].append(res[arm])
                elif args.parent_root:
                    parent.append(run_child(scenario, envs, ['pressure'], args.parent_root)['pressure'])
            print(scenario, 'round', k, {a: round(v[-1], 2) for a, v in runs.items()}, 'parent', parent[-1:], flush=True)
        yard = parent if parent else runs['pressure']
        res = dict(envs=envs, live_vehicles=live, yardstick='pressure_kernel of the parent commit' if parent else 'pressure_kernel of this library',
                   yardstick_us=yard, yardstick_median_us=median(yard), yardstick_spread=(max(yard) - min(yard)) / median(yard))
        for arm in ARMS:
            res[arm] = dict(us=runs[arm], median_us=median(runs[arm]), ratio_to_yardstick=median(runs[arm]) / median(yard))
        out[scenario] = res
    return out


def evaluate(args):
    import pandas as pd
    sys.path.insert(0, ROOT)
    from bench_controllers import ENV_INI
    from deeprl_signal_control_amd import main as cli
    out = dict(note='default keys, nothing tuned; vehicle dynamics not pinned against SUMO')
    for scenario in ('large_grid', 'real_net'):
        seeds = ENV_INI[scenario]['test_seeds']
        rows = []
        for name in ('greedy', 'fixedtime', 'maxpressure', 'actuated', 'sotl'):
            with tempfile.TemporaryDirectory() as base:
                os.makedirs(base + '/%s/data' % name)
                keys = dict(ENV_INI[scenario], agent='greedy')
                with open(base + '/%s/data/config.ini' % name, 'w') as fh:
                    fh.write('[MODEL_CONFIG]\npolicy = greedy\n\n[ENV_CONFIG]\n' + ''.join('%s = %s\n' % kv for kv in keys.items()))
                cli.main(['--base-dir', base, 'evaluate', '--agents', name, '--evaluation-seeds', seeds])
                pre = base + '/eva_data/%s_%s_' % (scenario, name)
                control, trip = (pd.read_csv(pre + k + '.csv', index_col=0) for k in ('control', 'trip'))
                cut = len(pd.read_csv(pre + 'trip_truncated.csv', index_col=0)) if os.path.exists(pre + 'trip_truncated.csv') else 0
                rows.append(dict(controller=name, mean_step_reward=float(control.reward.mean()), arrived=int(len(trip)), teleports=int(cut)))
                print(json.dumps(rows[-1]), flush=True)
        out[scenario] = dict(seeds=[int(s) for s in seeds.split(',')], rows=rows)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['kernel', 'eval', 'child'])
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--scenario', default='large_grid', help='(child)')
    ap.add_argument('--envs', type=int, default=1024, help='(child)')
    ap.add_argument('--arms', default=','.join(ARMS), help='(child)')
    ap.add_argument('--package-root', default=None, help='(child)')
    args = ap.parse_args()
    if args.what == 'child':
        child(args)
    else:
        res = kernel(args) if args.what == 'kernel' else evaluate(args)
        print(json.dumps(res, indent=1))
        if args.json:
            with open(args.json, 'w') as fh:
                json.dump(res, fh, indent=1)
                fh.write('\n')
