#!/usr/bin/env python
"""Measurements of the pressure reward (objective = pressure).

    python tools/bench_pressure_reward.py [--envs 1024] [--json OUT]

pressure_reward_kernel alone (tsc_profile_select on its id) at E instances of large_grid, armed, after 200 greedy-controlled control
steps: microseconds, share of step_kernel's time (measured the same way over the same kind of steps) and share of the HBM peak on its
algorithmic bytes -- 16 B per live vehicle on the walked lanes (from 64 evenly spaced instances), the walked lanes' counts, and
A * 8 + 8 B written per instance; both measures.  The control step with and without the reward is tools/bench_env.py
[--reward-pressure count]."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK = 8.0e12          # B/s (MI355X spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import torch
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_large_grid
    E = args.envs
    out = dict(envs=E, scenario='large_grid', warm_up_steps=200, timed_steps=50)
    for measure in ('count', 'queue'):
        scn = build_large_grid('ma2c', objective='pressure', pressure_measure=measure)
        tabs = scn.pressure_tables()
        env = VecTrafficEnv(scn, E, seed=12)
        obs = env.reset()
        act = torch.zeros(E, scn.n_agent, dtype=torch.int32, device='cuda')
        for _ in range(200):
            obs = env.step(env.greedy_actions(obs, out=act))[0]
        res = {}
        for name in ('env_step', 'pressure_reward'):               # one id bracketed at a time
            _lib.profile_select([name])
            _lib.profile(enable=True, reset=True)
            for _ in range(50):
                obs = env.step(env.greedy_actions(obs, out=act))[0]
            p = _lib.profile()
            _lib.profile(enable=False)
            res[name] = 1e3 * p[name][0] / p[name][1]
        _lib.profile_select(None)
        walked = float(np.mean([env.get_state(int(e))['n'][tabs['walk']].sum() for e in np.linspace(0, E - 1, 64).astype(int)]))
        bytes_ = E * (16.0 * walked + 4 * len(tabs['walk']) + 8 * scn.n_agent + 8)
        us = res['pressure_reward']
        out[measure] = dict(pressure_reward_kernel_us=us, step_kernel_us=res['env_step'], share_of_step_kernel=us / res['env_step'],
                            walked_vehicles_per_instance=walked, live_vehicles=env.mean_live_vehicles(), algorithmic_bytes=bytes_,
                            hbm_share=bytes_ / (us * 1e-6) / HBM_PEAK)
        env.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
