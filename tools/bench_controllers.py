#!/usr/bin/env python
"""Measurements of the baseline controllers (greedy, max-pressure, fixed-time).

    python tools/bench_controllers.py kernel [--envs 1024] [--json profiles/controllers_bench.json]
    python tools/bench_controllers.py eval [--seeds 10] [--scenarios large_grid,real_net] [--json profiles/controllers_eval.json]

kernel: pressure_kernel alone (tsc_profile_select on its id) at E instances of large_grid, on the state after 200 greedy-controlled
control steps, as microseconds and as a share of the HBM peak on its algorithmic bytes -- the records and counts of the walked
lanes read once plus the action write (vehicles on the walked lanes from 64 evenly spaced instances) -- next to step_kernel's
time over the last 50 of those steps, and the sim-only loop with each controller in front of every step.
eval: `evaluate` over the evaluation seeds for greedy, max-pressure (count / queue, min_green 1 / 3) and fixed-time: mean step
reward, average queue and mean trip time, the trips the teleport surrogate truncated counted apart."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK = 8.0e12          # B/s (MI355X spec)
ENV_INI = {
    'large_grid': dict(clip_wave=2.0, clip_wait=2.0, control_interval_sec=5, coop_gamma=0.9, episode_length_sec=3600, norm_wave=5.0,
                       norm_wait=100.0, coef_wait=0.2, peak_flow1=1100, peak_flow2=925, init_density=0, objective='hybrid',
                       scenario='large_grid', seed=12, test_seeds='10000,20000', yellow_interval_sec=2),
    'real_net': dict(clip_wave=2.0, clip_wait=2.0, control_interval_sec=5, coop_gamma=0.75, episode_length_sec=3600, norm_wave=5.0,
                     norm_wait=30.0, coef_wait=0, flow_rate=325, objective='queue', scenario='real_net', seed=42,
                     test_seeds='10000,20000,30000', yellow_interval_sec=2)}


def kernel(args):
    import torch
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_large_grid
    scn = build_large_grid('greedy')
    E = args.envs
    env = VecTrafficEnv(scn, E, seed=12)
    obs = env.reset()
    act = torch.zeros(E, scn.n_agent, dtype=torch.int32, device='cuda')
    for _ in range(150):
        obs = env.step(env.greedy_actions(obs, out=act))[0]
    _lib.profile_select(['env_step'])
    _lib.profile(enable=True, reset=True)
    for _ in range(50):
        obs = env.step(env.greedy_actions(obs, out=act))[0]
    p = _lib.profile()
    step_us = 1e3 * p['env_step'][0] / p['env_step'][1]
    out = dict(envs=E, scenario='large_grid', live_vehicles=env.mean_live_vehicles(), step_kernel_us=step_us)
    tabs = scn.pressure_tables()
    walked = np.mean([env.get_state(int(e))['n'][tabs['walk']].sum() for e in np.linspace(0, E - 1, 64).astype(int)])
    bytes_ = E * (16.0 * walked + 4 * len(tabs['walk']) + 4 * scn.n_agent)
    for measure in ('count', 'queue'):
        env.max_pressure_actions(out=act, measure=measure)         # arm
        _lib.profile_select(['pressure'])
        _lib.profile(enable=True, reset=True)
        for _ in range(50):
            env.max_pressure_actions(out=act, measure=measure)
        p = _lib.profile()
        us = 1e3 * p['pressure'][0] / p['pressure'][1]
        out['pressure_kernel_%s' % measure] = dict(us=us, share_of_step_kernel=us / step_us, algorithmic_bytes=bytes_,
                                                   walked_vehicles_per_instance=float(walked),
                                                   hbm_share=bytes_ / (us * 1e-6) / HBM_PEAK)
    _lib.profile(enable=False)
    _lib.profile_select(None)
    loop = {}
    for ctl in ('greedy', 'maxpressure', 'fixedtime'):             # sim-only loop, controller + step, from the same state on
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(200):
            if ctl == 'greedy':
                env.greedy_actions(obs, out=act)
            elif ctl == 'maxpressure':
                env.max_pressure_actions(out=act, measure='count')
            else:
                env.fixed_time_actions(6, out=act)
            obs = env.step(act)[0]
        torch.cuda.synchronize()
        loop[ctl] = 1e6 * (time.perf_counter() - t0) / 200
    out['loop_us_per_control_step'] = loop
    env.close()
    return out


def evaluate(args):
    import pandas as pd
    from deeprl_signal_control_amd import main as cli
    seeds = [10000 * (i + 1) for i in range(args.seeds)]
    variants = [('greedy', {})] + [('maxpressure', dict(pressure_measure=m, pressure_min_green=g)) for m in ('count', 'queue') for g in (1, 3)] \
        + [('fixedtime', dict(fixed_time_steps=6))]
    out = {}
    for scenario in args.scenarios.split(','):
        rows = []
        for name, extra in variants:
            with tempfile.TemporaryDirectory() as base:
                os.makedirs(base + '/%s/data' % name)
                keys = dict(ENV_INI[scenario], agent='greedy', **extra)
                with open(base + '/%s/data/config.ini' % name, 'w') as fh:
                    fh.write('[MODEL_CONFIG]\npolicy = greedy\n\n[ENV_CONFIG]\n' + ''.join('%s = %s\n' % kv for kv in keys.items()))
                cli.main(['--base-dir', base, 'evaluate', '--agents', name, '--evaluation-seeds', ','.join(map(str, seeds))])
                pre = base + '/eva_data/%s_%s_' % (scenario, name)
                control, traffic, trip = (pd.read_csv(pre + k + '.csv', index_col=0) for k in ('control', 'traffic', 'trip'))
                cut = pd.read_csv(pre + 'trip_truncated.csv', index_col=0) if os.path.exists(pre + 'trip_truncated.csv') else None
                rows.append(dict(controller=name, **extra, mean_step_reward=float(control.reward.mean()),
                                 avg_queue=float(traffic.avg_queue.mean()), trips=int(len(trip)),
                                 mean_trip_time_sec=float(trip.duration_sec.mean()),
                                 truncated_trips=0 if cut is None else int(len(cut)),
                                 truncated_mean_time_in_network_sec=None if cut is None else float(cut.duration_sec.mean())))
                print(json.dumps(rows[-1]), flush=True)
        out[scenario] = dict(seeds=seeds, rows=rows)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['kernel', 'eval'])
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--seeds', type=int, default=10)
    ap.add_argument('--scenarios', default='large_grid,real_net')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    res = kernel(args) if args.what == 'kernel' else evaluate(args)
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
