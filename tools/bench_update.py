#!/usr/bin/env python
"""Time the A2C update's kernels alone (no simulator): fill one rollout of the benchmark shape through the fused forward
(random observations, E env instances, T = n_step), then run compute_grads `--reps` times with HIP-event timing on.
    python tools/bench_update.py [--envs 1024] [--agent ma2c] [--policy lstm] [--reps 3] [--algo ppo [--ppo-epochs 2] [--json]] [--share-params]
--algo ppo times `--ppo-epochs` epochs per rollout and also prints the wall time (stream-synchronised, profiling off) of an epoch-0
update and of a later epoch (re-forward + update); --algo a2c prints the wall time of its one update the same way.
Environment knobs of the library (TSC_DW_SPLIT, TSC_DX_SPLIT, TSC_UNFUSED_DW, TSC_UNFUSED_DX) select kernel variants
for A/B runs; --json reports the choice (dw_split, dx_split).  --share-params arms parameter sharing ([MODEL_CONFIG] share_params = 1): the class-mean
reduce runs inside the grad_norm scope, so that line's difference to an unarmed run is its cost.  The dwxh stamps are dwxh_kernel's (TSC_DW_SPLIT=0): dwxh_split_kernel carries
none; the dx1w1 stamps are taken by whichever of dx1w1_split_kernel / dx1w1_kernel2 runs.
--stamps (a library built with TSC_BUILD_DEFS=-DTSC_UPD_STAMPS=1): shader-clock stamps of workgroup 0, waves 0 and 4 (the two
wavefronts of one SIMD), in one step of dwxh_kernel (16 rows: sub-chunk 11, the last of its 64-row interval) and of dx1w1_kernel2
(32 rows: chunk 5) -- step start, first MFMA, last MFMA, staging done, barrier passed -- printed as cycles per segment, each
labelled with what that wave does in it (waves 0..3 stage before their MFMAs, waves 4..7 after).  Valid where the stamped step
lies in an unclamped interval: splits of at least 272 rows (the benchmark shape: 24 576)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--agent', default='ma2c')
    ap.add_argument('--scenario', default='large_grid')
    ap.add_argument('--policy', default='lstm', choices=['lstm', 'fc'], help='fc = FcACPolicy (the benchmark runs it with --agent ia2c)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--algo', default='a2c', choices=['a2c', 'ppo'])
    ap.add_argument('--ppo-epochs', type=int, default=2)
    ap.add_argument('--share-params', action='store_true', help='[MODEL_CONFIG] share_params = 1: agents of equal shape share one set of weights')
    ap.add_argument('--stamps', action='store_true', help='per-step cycle split of dwxh / dx1w1 (needs a -DTSC_UPD_STAMPS=1 build)')
    ap.add_argument('--json', action='store_true', help='one JSON line with the wall times (ms) of the updates, per epoch index, and the kernel times at full precision')
    args = ap.parse_args()
    from deeprl_signal_control_amd import _lib
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario(args.scenario, args.agent)
    T = 120 if args.scenario == 'large_grid' else 40
    m = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, args.envs, scn.s_max, int(scn.green_tab.shape[1]),
               dict(batch_size=T, **(dict(algo='ppo', ppo_epochs=args.ppo_epochs) if args.algo == 'ppo' else {}),
                    **(dict(share_params=1) if args.share_params else {})), device=0, seed=0,
               name=args.agent, policy=args.policy)
    sl = m.rollout_slots()
    g = torch.Generator(device='cuda'); g.manual_seed(0)
    out = {}
    for rep in range(args.reps + 1):
        m.reset()
        sl['obs'].copy_(torch.rand(sl['obs'].shape, generator=g, device='cuda') * 2)
        sl['done'].zero_(); sl['done'][0].fill_(1)
        sl['reward'].copy_(-torch.rand(sl['reward'].shape, generator=g, device='cuda', dtype=torch.float64) * 4000)
        m.cur_t = 0
        for t in range(T):
            m.forward_sample(sl['obs'][t], sl['done'][t], v_out=sl['value'][t], action_out=sl['action'][t])
            m.commit_transition()
        R = m.forward(sl['obs'][T], False, 'v')
        torch.cuda.synchronize()
        if rep == 1:
            _lib.profile(enable=1, reset=True)
        if args.stamps and rep == args.reps:
            _lib.check(m._L.tsc_model_debug_clock(m._h, 1, None, 0))
        m.backward(R)
    torch.cuda.synchronize()
    if args.stamps:
        import ctypes as C
        st = np.zeros(32, np.int64)
        _lib.check(m._L.tsc_model_debug_clock(m._h, 1, st.ctypes.data_as(C.c_void_p), 32))
        # What lies between two stamps differs by wave: in dwxh waves 0..3 stage (LDS writes, row requests) BEFORE their MFMAs and
        # waves 4..7 after; in dx1w1 waves 0..3 request the next chunk before their tiles, waves 4..7 between them (inside the MFMA
        # segment), and both write LDS after the last MFMA.
        seg_names = {('dwxh', 0): ('dZ requests + staging', 'MFMA block', 'operand moves', 'barrier'),
                     ('dwxh', 1): ('dZ requests', 'MFMA block', 'staging + operand moves', 'barrier'),
                     ('dx1w1', 0): ('next chunk requested', 'tiles', 'LDS writes', 'barrier'),
                     ('dx1w1', 1): ('(nothing)', 'tiles with the request between them', 'LDS writes', 'barrier')}
        need = {'dwxh': 272, 'dx1w1': 192}
        for name, base in (('dwxh', 0), ('dx1w1', 16)):
            for w in (0, 1):
                t = st[base + 8 * w: base + 8 * w + 5]
                seg = [int(t[i + 1] - t[i]) for i in range(4)]
                if (t <= 0).any() or min(seg) < 0:
                    print('stamps %-5s wave %d: not taken (library without -DTSC_UPD_STAMPS=1, or splits shorter than %d rows)'
                          % (name, 4 * w, need[name]))
                    continue
                print('stamps %-5s wave %d: %s, step %d cycles'
                      % (name, 4 * w, ', '.join('%s %d' % (n, c) for n, c in zip(seg_names[name, w], seg)), int(t[4] - t[0])))
    prof = _lib.profile()
    _lib.profile(enable=False)
    tot, kern = 0.0, {}
    for k, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
        if k in ('policy_fwd_fused',):
            continue
        per = kern[k] = ms / args.reps
        tot += per
        print('%-18s %8.3f ms per update  (%d launches)' % (k, per, cnt))
    print('%-18s %8.3f ms' % ('update total', tot))

    # wall time per update without the event pairs: epoch by epoch, the stream drained before and after
    import json
    import time
    # (getattr: the file also runs against a checkout from before `algo` existed, for A/B runs of the A2C update across commits)
    n_epoch = getattr(m, 'n_epoch', 1)
    wall = [[] for _ in range(n_epoch)]
    for rep in range(args.reps):
        m.reset()
        sl['obs'].copy_(torch.rand(sl['obs'].shape, generator=g, device='cuda') * 2)
        sl['done'].zero_(); sl['done'][0].fill_(1)
        m.cur_t = 0
        for t in range(T):
            m.forward_sample(sl['obs'][t], sl['done'][t], v_out=sl['value'][t], action_out=sl['action'][t])
            m.commit_transition()
        R = m.forward(sl['obs'][T], False, 'v')
        for k in range(n_epoch):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if n_epoch > 1 or getattr(m, 'algo', 'a2c') == 'ppo':
                m.compute_grads(R, k); m.apply_grads(1.0, epoch=k)
            else:
                m.compute_grads(R); m.apply_grads(1.0)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    for k, w in enumerate(wall):
        print('wall: %s update, epoch %d: %s ms (median %.3f)' % (args.algo, k, ' '.join('%.3f' % x for x in w), float(np.median(w))))
    if args.json:
        print(json.dumps(dict(algo=args.algo, envs=args.envs, agent=args.agent, scenario=args.scenario, n_step=T, wall_ms_per_epoch=wall,
                              kernel_ms_per_update=kern, dw_split=getattr(m, 'dw_split', None), dx_split=getattr(m, 'dx_split', None),
                              share_sizes=m.share_sizes() if getattr(m, 'share', None) is not None else None)))


if __name__ == '__main__':
    main()
