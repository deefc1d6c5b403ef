#!/usr/bin/env python
"""Sim-only cost of per-instance demand (tsc_env_set_demand) with tools/bench_env.py's protocol: large_grid, E instances, 300 control
steps of random actions to t = 1500 s, then `steps` timed ones.
    python tools/bench_demand.py [E] [steps] [nominal|demand]
nominal: a handle that never calls set_demand.  demand: every instance runs the scenario's own column through its per-instance table
(the same traffic, so the same vehicles); also demand_kernel's time per reset (HIP events, tsc_profile_read) and the prologue's
shader-clock cycles (tsc_env_debug_clock).  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from deeprl_signal_control_amd import _lib
from deeprl_signal_control_amd.env import VecTrafficEnv
from deeprl_signal_control_amd.scenario import build_large_grid

E = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
mode = sys.argv[3] if len(sys.argv) > 3 else 'demand'
scn = build_large_grid('ma2c')
env = VecTrafficEnv(scn, E, seed=12)
out = dict(mode=mode, E=E, steps=steps)
if mode == 'demand':
    nominal = np.tile(scn.flows[:, 2].astype(np.int32), (E, 1))
    env.set_demand(nominal)
    env.reset()                              # (first launch: code object load)
    _lib.profile_select(['demand'])
    _lib.profile(enable=True, reset=True)
    for _ in range(5):                       # (a reset rebuilds the tables only after a set_demand)
        env.set_demand(nominal)
        env.reset()
    ms, cnt = _lib.profile()['demand']
    _lib.profile(enable=False)
    _lib.profile_select(None)
    out.update(demand_kernel_us_per_reset=1e3 * ms / cnt, demand_kernel_launches=cnt,
               table_bytes=int(E * scn.n_stream * ((scn.episode_length_sec + 64 + 3) // 4 * 4)))
    env.seeds[:] = np.arange(12, 12 + E)     # the timed episode runs the seeds of a fresh handle
env.reset()
g = torch.Generator(device='cuda'); g.manual_seed(0)
acts = [torch.randint(0, 5, (E, 25), generator=g, device='cuda', dtype=torch.int32) for _ in range(16)]
for phase, n in (('warmup', 300), ('timed', steps)):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(n):
        env.step(acts[i % 16])
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    out['%s_us_per_step' % phase] = 1e6 * dt / n
out['live_vehicles_per_env'] = env.mean_live_vehicles()
st = (C.c_int64 * 64)()
_lib.check(env._L.tsc_env_debug_clock(env._h, 1, None))
pro = []
for i in range(8):
    env.step(acts[i]); torch.cuda.synchronize()
    _lib.check(env._L.tsc_env_debug_clock(env._h, 1, st))
    pro.append(int(st[1] - st[0]))
out['prologue_cycles_workgroup0'] = pro
print(json.dumps(out))
env.close()
