#!/usr/bin/env python
"""Times an IQL learner's launches in isolation (large_grid, E = 1024 by default): the minibatch gradient
(tsc_iql_compute_grads: sample + fused gradient + reduce) and the acting forward, with HIP events on the launch stream.

    python tools/bench_iql.py [--envs 1024] [--reps 50] [--scenario large_grid] [--model-type dqn|lr] [--target-update N [--double-q]] [--per]
                              [--dueling] [--return-steps N] [--share-params]

--model-type lr times IQL-LR, which always runs the grouped-GEMM path (gather, GEMMs, iql_td_kernel).  IQL-DNN runs the fused kernels at
the widths they are built for; TSC_IQL_FUSED=0 in the environment selects the grouped path for it too ("fused" in the output line says
which path ran).

--target-update N arms the target network (two launches per gradient: the TD targets from the frozen copy, then the gradient with one
row set).  --per arms prioritized replay (the proportional sampler in place of the Floyd draw, the
two-launch gradient with importance weights, the priority write-back and, on add_transition, the fill at the ring's maximum; the rings are
filled to their capacity then, the sampler's full read).  --dueling arms the dueling head (always the two-launch gradient, its own
instantiations of the act, target and gradient kernels).  --return-steps N arms multi-step returns (the window pre-pass iql_nstep behind the
draw, always the two-launch gradient, the target kernel's instantiations with the rows' return and discount).  --share-params arms
parameter sharing (share_reduce_kernel in front of the norm, inside the iql_adam scope: compare that id of --split with and without).  --split adds the per-kernel split of the minibatch step ("kernel_us": iql_target / iql_grad / ..., each measured in a
pass of its own with only its launches bracketed: 5 x reps more minibatch steps).  --stamps reads the gradient kernel's workgroups
and, on an armed handle, the target kernel's as well ("target_wg_us").
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--scenario', default='large_grid')
    ap.add_argument('--model-type', choices=('dqn', 'lr'), default='dqn', help='IQL-DNN or IQL-LR (lr: always the grouped-GEMM path)')
    ap.add_argument('--target-update', type=int, default=0, help='[MODEL_CONFIG] target_update: refresh the target network every N Adam steps (0: none)')
    ap.add_argument('--double-q', action='store_true', help='[MODEL_CONFIG] double_q = 1 (needs --target-update)')
    ap.add_argument('--per', action='store_true', help='[MODEL_CONFIG] prioritized_replay = 1')
    ap.add_argument('--dueling', action='store_true', help='[MODEL_CONFIG] dueling = 1')
    ap.add_argument('--return-steps', type=int, default=1, help='[MODEL_CONFIG] return_steps (multi-step returns; 1: the one-step target)')
    ap.add_argument('--share-params', action='store_true', help='[MODEL_CONFIG] share_params = 1 (one Q-network per class of like-shaped agents)')
    ap.add_argument('--split', action='store_true', help='per-kernel split of the minibatch step (one more pass of --reps steps per kernel)')
    ap.add_argument('--stamps', action='store_true', help='phase stamps of workgroup 0 and the start / end of every workgroup (tsc_iql_debug_clock)')
    args = ap.parse_args()
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.iql import VecIQL
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(args.scenario, 'iqld' if args.model_type == 'dqn' else 'iqll')
    E, A = args.envs, scn.n_agent
    m = VecIQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, E, scn.s_max, int(scn.green_tab.shape[1]),
               dict(batch_size=20, buffer_size=1000, reward_norm=3000.0, target_update=args.target_update, double_q=int(args.double_q),
                    prioritized_replay=int(args.per), dueling=int(args.dueling), return_steps=args.return_steps,
                    share_params=int(args.share_params)),
               total_step=10 ** 6, seed=0, model_type=args.model_type)
    g = torch.Generator(device='cuda'); g.manual_seed(0)
    mask = torch.zeros(A, scn.s_max, device='cuda')
    for a, n in enumerate(scn.n_s_ls):
        mask[a, :n] = 1
    obs = torch.rand(E, A, scn.s_max, generator=g, device='cuda') * 2 * mask
    for t in range(1000 if args.per else 40):
        nobs = torch.rand(E, A, scn.s_max, generator=g, device='cuda') * 2 * mask
        act = (torch.rand(E, A, generator=g, device='cuda') * torch.as_tensor(scn.n_a_ls, device='cuda')).to(torch.int32)
        rew = -torch.rand(E, A, generator=g, device='cuda', dtype=torch.float64) * 6000.0
        done = (torch.rand(E, generator=g, device='cuda') < 0.05).to(torch.uint8)
        m.add_transition(obs, act, rew, nobs, done)
        obs = nobs

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        for _ in range(reps):
            fn()
        b_.record()
        torch.cuda.synchronize()
        return a_.elapsed_time(b_) / reps * 1e3

    step = [0]

    def grads():
        _lib.check(m._L.tsc_iql_compute_grads(m._h, 7, step[0]))
        step[0] += 1
    out = {'model_type': args.model_type, 'fused': m.fused, 'E': E, 'target_update': m.target_update, 'double_q': m.double_q, 'prioritized_replay': m.prioritized_replay, 'dueling': m.dueling, 'return_steps': m.return_steps,
           'share_params': int(m.share is not None), 'share_sizes': m.share_sizes(),
           'replay_size': m.replay_size()[0], 'compute_grads_us': timed(grads, args.reps),
           'forward_us': timed(lambda: m.forward(obs, mode='explore'), args.reps),
           'minibatch_step_us': timed(lambda: m.minibatch_step(1e-4), args.reps)}
    # where a minibatch step's time goes: one kernel id at a time (an event pair inflates the launch behind it, include/tsc.h)
    kern = {}
    two_launch = bool((m.target_update or m.prioritized_replay or m.dueling or m.return_steps > 1) and m.fused)
    sample = ['iql_per_sample', 'iql_per_update', 'iql_per_add'] if m.prioritized_replay else ['iql_sample']
    for name in (['iql_nstep'] * (m.return_steps > 1) + ['iql_target'] * two_launch + ['iql_grad', 'iql_reduce'] + sample + ['iql_adam']) * args.split:
        _lib.profile_select([name])
        _lib.profile(enable=True)
        _lib.profile(reset=True)
        for _ in range(args.reps):
            if name == 'iql_per_add':
                m.add_transition(obs, act, rew, nobs, done)
            else:
                m.minibatch_step(1e-4)
        ms, cnt = _lib.profile().get(name, (0.0, 0))
        _lib.profile(enable=False)
        if cnt:
            kern[name] = ms / cnt * 1e3
    _lib.profile_select(None)
    _lib.profile(reset=True)
    if args.split:
        out['kernel_us'] = kern
        if 'iql_per_sample' in kern:       # the sampler's roofline: every ring's filled slots read once, over the measured time
            out['per_sample_bytes'] = 4 * E * A * m.replay_size()[0]
            out['per_sample_GBps'] = out['per_sample_bytes'] / kern['iql_per_sample'] * 1e-3
    if args.stamps and m.fused:
        import ctypes as C
        n = 64 + 2 * 4096
        buf = np.zeros(n, np.int64)
        _lib.check(m._L.tsc_iql_debug_clock(m._h, 1, None, 0))
        for _ in range(3):
            grads()
        _lib.check(m._L.tsc_iql_debug_clock(m._h, 1, buf.ctypes.data_as(C.c_void_p), n))
        st = buf[:64].reshape(4, 16)[:, :11]
        names = ['nets', 'td+stage', 'dX1', 'bar1', 'B', 'bar2', 'C', 'bar3', 'D', 'bar4']
        out['phase_cycles_per_wave'] = {nm: [int(st[w, k + 1] - st[w, k]) for w in range(4)] for k, nm in enumerate(names)}
        out['chunk_cycles'] = [int(st[w, 10] - st[w, 0]) for w in range(4)]
        fine = buf[:64].reshape(4, 16)
        if fine[0, 11]:
            out['nets_fine'] = {'L1': [int(fine[w, 11] - fine[w, 0]) for w in range(4)], 'relu1': [int(fine[w, 12] - fine[w, 11]) for w in range(4)], 'L2': [int(fine[w, 13] - fine[w, 12]) for w in range(4)], 'relu2': [int(fine[w, 14] - fine[w, 13]) for w in range(4)], 'Q': [int(fine[w, 1] - fine[w, 14]) for w in range(4)]}
        def wg_stats(wg):
            t0 = wg[:, 0].min()
            return {'first_start': 0.0, 'last_start': float((wg[:, 0].max() - t0) / 100.0), 'min_dur': float((wg[:, 1] - wg[:, 0]).min() / 100.0),
                    'median_dur': float(np.median(wg[:, 1] - wg[:, 0]) / 100.0), 'max_dur': float((wg[:, 1] - wg[:, 0]).max() / 100.0),
                    'span': float((wg[:, 1].max() - t0) / 100.0)}
        # [64 + 2 b]: the gradient kernel's workgroups; behind them, on an armed handle, the target kernel's (include/tsc.h): an unarmed
        # handle leaves that half zero, so the number of workgroups is the number of stamped pairs, halved when armed
        wg = buf[64:].reshape(-1, 2)
        wg = wg[wg[:, 0] > 0]
        W = len(wg) // 2 if two_launch else len(wg)
        out['workgroups'] = int(W)
        out['wg_us'] = wg_stats(wg[:W])
        if two_launch:
            out['target_wg_us'] = wg_stats(wg[W:])
    gsum = float(m.grad_tensor().double().abs().sum().item())
    out['grad_abs_sum'] = gsum
    print(json.dumps(out))
    m.close()


if __name__ == '__main__':
    main()
