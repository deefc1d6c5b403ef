"""Synthetic agent layouts for the learner parity tests -- TEST INFRASTRUCTURE ONLY, host only (no GPU, no library).

Both learners choose their kernels from the shape of the agents (csrc/tsc_model.hip "The plan", csrc/tsc_iql.hip tsc_iql_create); the
three built-in scenarios visit only a corner of what those choices accept.  A Layout carries exactly what the test helpers read from a
scenario -- n_agent, n_s_ls, n_a_ls, n_w_ls, n_f_ls, s_max, a_max -- and nothing else: no environment, no scenario tables.  Every
layout of the two registries exists because of one declared limit ("Supported layouts"); the limit is named
next to it.

Every layout is uniform the way the reference is: either every agent has wait inputs or none has, and in MA2C every agent has at least
one fingerprint input.  A mixed layout (some agents with a wait / fingerprint part, some without) has no definition in the oracle or
the reference -- tower() drops the whole block of an agent whose count is zero while the device keeps the block's bias columns -- and
is out of scope here.

Routes.  `route[policy]` is what tsc_model_plan must report: LSTM (rollout forward, dwxh, dx1w1), FC (rollout forward, fc_bwd), with
the forward numbered as in include/tsc.h (0 Dense, 1 Tile, 2 Ws, 3 FcThread, 4 FcMfma).  They follow from the width table and the
s_max <= 64 gate of the plan; the three that also depend on an LDS budget (obs64 LSTM: Ws or Tile; h96 / h112 FC: FcThread or Dense)
are the values an MI355X handle reported, recorded here and asserted from then on (RECORDED).

The rollouts of tests/test_layouts_gpu.py are redrawn on the host by forward_inputs / fill_host / iql_transitions below: the same
RandomState seeds in the same order of draws as tests/test_model_gpu.py::_fill and tests/iql_harness.py::replay_vs_oracle, so that
tests/test_layouts_host.py states conditions about the very samples the GPU tests compare.

The agent-count axis.  A2C_COUNT_LAYOUTS holds layouts of 1, 64, 65, 130, 340 and 341 agents: the number of agents sets the row splits
per tower (upd_splits), the forward workgroups per tower (fwd_splits), the head slices (head_slices) and, through the workspace, the
choice of dwxh_kernel at all (dwxh_fits).  Those functions restate the lines of csrc/tsc_model.hip they name.  From 64 agents on the
float64 oracle evaluates pick(A) agents only.

ROWS.  From 65 agents on s_upd = 1, so one workgroup of dwxh_kernel / dx1w1_kernel2 / fc_bwd_kernel walks the whole batch and a case
(E, T) chooses its rows R = E T directly.  dwxh_schedule(R) and w1_schedule(R) restate the kernels' row loops -- full 64-row intervals
and the clamped tail of 16-row sub-chunks; plain and clamped 32-row chunks -- and ROWS is the list of (E, T) with R <= 300 that walks
every class of them: no, one and several full intervals, every tail length a full interval can leave behind (5 - 9) and every one
without (1 - 8), last sub-chunks of 1, 2, 15 and 16 rows.  At R <= 300 a lost or doubled row is at least 3e-3 of a weight gradient;
at the benchmarked batches, the only other place these schedules run, it is 1e-5 and below tolerance.  What ROWS must cover is
asserted by tests/test_layouts_host.py::test_rows_cover_the_schedules, not by the list.  count_cases() lists every update case of
the three axes (agent count, rows, time) for the GPU module and the host module alike."""
import contextlib

import numpy as np


class Layout:
    """agents: one (n_wave, n_wait, n_fp, n_a) per agent, observation = [wave | wait | fingerprint] like the environment's."""

    def __init__(self, agents, s_max):
        self.agents = [tuple(int(x) for x in a) for a in agents]
        self.n_agent = len(self.agents)
        self.n_wave_ls = [a[0] for a in self.agents]
        self.n_w_ls = [a[1] for a in self.agents]
        self.n_f_ls = [a[2] for a in self.agents]
        self.n_a_ls = [a[3] for a in self.agents]
        self.n_s_ls = [a[0] + a[1] + a[2] for a in self.agents]
        self.s_max, self.a_max = int(s_max), max(self.n_a_ls)
        assert self.s_max % 4 == 0 and max(self.n_s_ls) <= self.s_max
        waits, fps = [w > 0 for w in self.n_w_ls], [f > 0 for f in self.n_f_ls]
        assert all(waits) or not any(waits), 'mixed wait inputs: out of scope (module docstring)'
        assert all(fps) or not any(fps), 'mixed fingerprint inputs: out of scope (module docstring)'

    def only(self, keep):
        """The layout of the agents for which keep(n_a) holds (same s_max)."""
        return Layout([a for a in self.agents if keep(a[3])], self.s_max)


# large_grid's ranges (build_scenario prints them): MA2C wave 18-30, wait 6, fingerprint 8-16, five actions; IA2C the same without fingerprints
_LG_MA2C = [(30, 6, 16, 5), (24, 6, 12, 5), (18, 6, 8, 5), (24, 6, 12, 5), (18, 6, 8, 5)]
_LG_IA2C = [(30, 6, 0, 5), (24, 6, 0, 5), (18, 6, 0, 5), (24, 6, 0, 5)]
# real_net's ranges, MA2C: wave 5-34, no wait, fingerprint 1-16, two to six actions
_RN_MA2C = [(34, 0, 16, 6), (5, 0, 1, 2), (20, 0, 8, 4), (12, 0, 16, 3), (34, 0, 2, 5)]

DENSE, TILE, WS, FC_THREAD, FC_MFMA = 0, 1, 2, 3, 4


def _a2c(agent, widths, s_max, agents, lstm, fc, why, wide=False):
    fw, fp, ft = widths
    return dict(agent=agent, layout=Layout(agents, s_max), cfg=dict(num_fw=fw, num_fp=fp, num_ft=ft), H=fw + fp + ft,
                route=dict(lstm=lstm, fc=fc), why=why, wide=wide)


# name -> agent kind, widths fw / fp / ft, s_max, agents, LSTM route (forward, dwxh, dx1w1), FC route (forward, fc_bwd), the limit it drives
A2C_LAYOUTS = {
    'head8': _a2c('ma2c', (128, 64, 32), 52, [(30, 6, 16, 8), (24, 6, 12, 7), (18, 6, 8, 2), (24, 6, 12, 5), (30, 6, 16, 8)],
                  (WS, 1, 1), (FC_MFMA, 1), 'full 8-wide head, n_a = 7'),
    'obs64': _a2c('ma2c', (128, 64, 32), 64, [(40, 8, 16, 5), (37, 8, 16, 3), (2, 1, 1, 2), (30, 6, 12, 8)],
                  (WS, 1, 1), (FC_MFMA, 1), 'full fourth 16-row obs tile; an agent with 4 inputs beside one with 64', wide=True),
    # s_max > 64: every kernel that stages the observation falls back.  dwxh reads X1 / h_prev / dZ only, never the observation, and stays.
    'obs68': _a2c('ia2c', (128, 0, 32), 68, [(60, 8, 0, 5), (57, 8, 0, 4), (9, 1, 0, 2)],
                  (DENSE, 1, 0), (DENSE, 0), 'narrow_obs false: dense forward, grouped first-layer update', wide=True),
    'tiny': _a2c('ia2c', (128, 0, 32), 4, [(3, 1, 0, 2), (1, 1, 0, 2), (2, 1, 0, 3)],
                 (WS, 1, 1), (FC_MFMA, 1), 'one partial obs tile, K = 4 GEMMs'),
    'edges160': _a2c('ma2c', (100, 28, 32), 52, _LG_MA2C, (WS, 1, 1), (FC_MFMA, 1), 'H = 160, block edges at columns 100 and 128'),
    'edges224': _a2c('ma2c', (150, 42, 32), 52, _LG_MA2C, (WS, 1, 1), (FC_MFMA, 1), 'H = 224, block edges at columns 150 and 192'),
    'edges128': _a2c('ia2c', (104, 0, 24), 36, _LG_IA2C, (WS, 1, 1), (FC_MFMA, 1), 'H = 128, block edge at column 104'),
    'edges192': _a2c('ma2c', (130, 62, 0), 52, _RN_MA2C, (WS, 1, 1), (FC_MFMA, 1), 'H = 192 without a wait block, edge at column 130'),
    'h96': _a2c('ia2c', (64, 0, 32), 36, _LG_IA2C, (TILE, 0, 0), (FC_THREAD, 0), 'off the width table, H % 32 == 0'),
    'h112': _a2c('ia2c', (96, 0, 16), 36, _LG_IA2C, (DENSE, 0, 0), (FC_THREAD, 0), 'H % 16 == 0 only'),
    'h124': _a2c('ia2c', (100, 0, 24), 36, _LG_IA2C, (DENSE, 0, 0), (DENSE, 0), 'H % 4 == 0 only'),
}
RECORDED = [('obs64', 'lstm'), ('h96', 'fc'), ('h112', 'fc')]       # routes behind an LDS budget: as reported by an MI355X handle
# tsc_model_create must refuse this one: "hidden width must be a multiple of 4"
A2C_REFUSED = _a2c('ia2c', (101, 0, 32), 36, _LG_IA2C, None, None, 'H = 133')


def _iql(model_type, num_fc, num_h, s_max, agents, fused, why, wide=False):
    return dict(model_type=model_type, layout=Layout([(w, t, 0, a) for w, t, a in agents], s_max), cfg=dict(num_fc=num_fc, num_h=num_h),
                fused=fused, why=why, wide=wide)


_Q160 = [(32, 16, 8), (31, 16, 7), (17, 16, 2), (16, 16, 3), (15, 1, 5), (1, 1, 8)]
_LG_IQL = [(30, 6, 5), (24, 6, 5), (18, 6, 5), (24, 6, 5)]
# name -> model type, num_fc / num_h, s_max, agents (wave, wait, n_a), fused?, the limit it drives.  batch_size 20 throughout.
IQL_LAYOUTS = {
    'q160_edge': _iql('dqn', 128, 64, 48, _Q160, True, 'fused limit with a wait part: n_wave = 32, n_wait = 16, s_max = 48'),
    'q160_past_wave': _iql('dqn', 128, 64, 48, [(33, 15, 8)] + _Q160[1:], False, 'n_wave = 33 with a wait part'),
    'q160_past_wait': _iql('dqn', 128, 64, 48, [(31, 17, 8)] + _Q160[1:], False, 'n_wait = 17'),
    'q128_edge': _iql('dqn', 128, 64, 48, [(48, 0, 8), (47, 0, 7), (33, 0, 2), (16, 0, 4), (1, 0, 6)], True, 'fused limit without a wait part: 48 wave inputs'),
    'q_obs52': _iql('dqn', 128, 64, 52, [(52, 0, 5), (49, 0, 4), (5, 0, 2)], False, 's_max > 48', wide=True),
    'q_small': _iql('dqn', 64, 32, 36, _LG_IQL, False, 'num_fc != 128: H1 = 80, H2 = 32'),
    'q_h2': _iql('dqn', 128, 32, 36, _LG_IQL, False, 'num_h != 64'),
    'lr_tiny': _iql('lr', 128, 64, 4, [(3, 1, 8), (1, 1, 2), (2, 1, 3)], False, 'IQL-LR, K = 4, n_a = 8'),
    'lr_wide': _iql('lr', 128, 64, 68, [(60, 8, 8), (57, 8, 4), (9, 1, 2)], False, 'IQL-LR, 68 inputs, n_a = 8', wide=True),
}
# tsc_iql_create must refuse this one: num_fc = 100 with wait inputs, H1 = 125, "hidden widths must be multiples of 4"
IQL_REFUSED = _iql('dqn', 100, 64, 36, _LG_IQL, None, 'H1 = 125')
# (the layouts above, in the order data_seed numbers them: names added later come behind, so that no rollout of an older case moves)
_SEED_ORDER = sorted(list(A2C_LAYOUTS) + list(IQL_LAYOUTS))


# ---- the agent-count axis ---------------------------------------------------------------------------------------------------------
# The number of agents A decides how the learner launches its kernels (csrc/tsc_model.hip tsc_model_create "The plan", launch_head_bwd,
# launch_dwxh, launch_w1); the functions below restate those lines on the host, and the layouts of A2C_COUNT_LAYOUTS sit where they change.
WS_FLOATS = 48 << 20                                    # tsc_model_create: m->ws_floats


def upd_splits(A):
    """Row splits per tower of dwxh_kernel / dx1w1_kernel2 / fc_bwd_kernel (tsc_model_create: P.s_upd = 256 / G, at least 1; G = 2 A)."""
    return max(1, 256 // (2 * A))


def fwd_splits(A, E):
    """Workgroups per tower of the Ws forward (tsc_model_create: P.s_fwd = min(s_upd, ceil(E / 32)))."""
    return min(upd_splits(A), (E + 31) // 32)


def split_rows(N, S, q):
    """Rows per split (split_rows in csrc/tsc_model.hip): ceil(N / S) rounded up to the kernel's row quantum q."""
    return ((N + S - 1) // S + q - 1) // q * q


def split_R(N, S, q):
    """The rows R = n1 - n0 each of the S workgroups of a tower sees (dwxh_kernel / dx1w1_kernel2: n0 = sp rows_per_split, n1 =
    min(n0 + rows_per_split, N)); 0 for a split that starts at or behind row N and skips its loops."""
    rps = split_rows(N, S, q)
    return [max(0, min(N, (sp + 1) * rps) - sp * rps) for sp in range(S)]


DWXH_Q, W1_Q, HEAD_Q = 2, 32, 16                        # kDwK, kW1Chunk, kHbRows: the row quanta of the three split passes


def head_slices(A, N):
    """Slices of head_bwd_kernel (launch_head_bwd: S = ceil(2048 / A), rows per slice = split_rows(N, S, kHbRows), S = ceil(N / rows))."""
    rps = split_rows(N, (8 * 256 + A - 1) // A, HEAD_Q)
    return (N + rps - 1) // rps


def dwxh_ws_floats(H):
    """A split's partial record of dwxh_kernel: [dWx ; dWh ; dbl] (dwxh_ws_floats in csrc/tsc_model.hip)."""
    return (H + 64 + 1) * 256


def dwxh_fits(A, H):
    """tsc_model_create's ws_fits(dwxh_ws_floats(H)): the fused dWx | dWh | dbl kernel is chosen only when every split's record fits."""
    return upd_splits(A) * 2 * A * dwxh_ws_floats(H) <= WS_FLOATS


def dwxh_schedule(R):
    """dwxh_kernel's row loop over a split of R rows (the two loops behind its prologue: `for (; KC * (c + 9) <= R; c += 4)`, four Plain
    16-row sub-chunks and a barrier; then `for (; KC * c < R; ++c)`, Clamp sub-chunks) -> (full intervals, tail sub-chunks, rows
    of the last sub-chunk)."""
    if R <= 0:
        return 0, 0, 0
    c = full = 0
    while 16 * (c + 9) <= R:
        c, full = c + 4, full + 1
    n = (R + 15) // 16
    return full, n - c, R - 16 * (n - 1)


def w1_schedule(R):
    """dx1w1_kernel2's row loop over a split of R rows (`for (; row + 2 * kW1Chunk <= n1; ...) chunk(Plain)`, then `for (; row < n1; ...)
    chunk(Clamp)`, 32-row chunks; fc_bwd_kernel walks the same chunks in one loop) -> (plain chunks, clamp chunks, rows of the last chunk)."""
    if R <= 0:
        return 0, 0, 0
    plain = 0
    while 32 * plain + 64 <= R:
        plain += 1
    n = (R + 31) // 32
    return plain, n - plain, R - 32 * (n - 1)


def _cycle(agents, n):
    return [agents[i % len(agents)] for i in range(n)]


def pick(A):
    """The agents the float64 oracle evaluates on a layout of A agents (the full oracle costs seconds per round from 65 agents on):
    the first, the last, two in between, and index 128 where there is one."""
    return sorted(set([0, A // 3, 2 * A // 3, A - 1] + ([128] if A > 128 else [])))


# three inputs or four per agent: the smallest observation a handle accepts (s_max % 4 == 0), so that 341 agents stay small
_EDGE_MA2C = [(2, 1, 1, 5), (1, 1, 2, 3), (1, 2, 1, 2), (1, 1, 1, 4)]
_W224, _W160, _W128, _W192 = (150, 42, 32), (100, 28, 32), (104, 0, 24), (130, 62, 0)
# name -> as A2C_LAYOUTS; what the agent count drives is the `why`.  Kept apart from A2C_LAYOUTS: the tests of that table run the full oracle.
A2C_COUNT_LAYOUTS = {
    'solo': _a2c('ma2c', _W224, 52, _LG_MA2C[:1], (WS, 1, 1), (FC_MFMA, 1), 's_upd = 128: nearly every split empty at small N; XCD map with G = 2'),
    'many64': _a2c('ma2c', _W224, 52, _cycle(_LG_MA2C, 64), (WS, 1, 1), (FC_MFMA, 1),
                   's_upd = 2, the last count before 1; s_fwd = 2 from E = 33 on; XCD map with G = 128'),
    'many65': _a2c('ma2c', _W224, 52, _cycle(_LG_MA2C, 65), (WS, 1, 1), (FC_MFMA, 1), 's_upd = 1: R = N = E T, a case chooses its R'),
    'many65_h128': _a2c('ia2c', _W128, 36, _cycle(_LG_IA2C, 65), (WS, 1, 1), (FC_MFMA, 1), 's_upd = 1 at H = 128: dwxh<6>, dx1w1<8>, fc_bwd<8>'),
    'many65_h160': _a2c('ma2c', _W160, 52, _cycle(_LG_MA2C, 65), (WS, 1, 1), (FC_MFMA, 1), 's_upd = 1 at H = 160: dwxh<7>, dx1w1<10>, fc_bwd<10>'),
    'many65_h192': _a2c('ma2c', _W192, 52, _cycle(_RN_MA2C, 65), (WS, 1, 1), (FC_MFMA, 1), 's_upd = 1 at H = 192: dwxh<8>, dx1w1<12>, fc_bwd<12>'),
    'many130': _a2c('ia2c', _W128, 36, _cycle(_LG_IA2C, 130), (WS, 1, 1), (FC_MFMA, 1),
                    '256 / G = 0 clamped to 1; head_bwd S = 16; the agent count of isolated_130'),
    'ws_edge_340': _a2c('ma2c', _W224, 4, _cycle(_EDGE_MA2C, 340), (WS, 1, 1), (FC_MFMA, 1), 'the last count whose dwxh records fit the workspace at H = 224'),
    'ws_edge_341': _a2c('ma2c', _W224, 4, _cycle(_EDGE_MA2C, 341), (WS, 0, 1), (FC_MFMA, 1), 'the first count past it: the plan must report dwxh = 0'),
}
ROW_WIDTHS = ['many65_h128', 'many65_h160', 'many65_h192']

# ROWS: the (E, T) of the row-split sweep on the 65-agent layouts, where s_upd = 1 and a split's R is the whole batch N = E T.  At
# N <= 300 one lost or doubled row is at least 3e-3 of a weight gradient, against a tolerance of 2e-5.  What the table must cover is
# stated by tests/test_layouts_host.py::test_rows_cover_the_schedules through dwxh_schedule / w1_schedule.  R = E T, in order:
#   2, 18, 33, 64, 65, 95, 111, 128, 130, 142: no full interval, tails of 1 - 9 sub-chunks, last sub-chunk of 1, 2, 14, 15, 16 rows
#   144, 146, 160, 176, 192, 195, 207: one full interval, then 5 - 9 tail sub-chunks in the ring it filled
#   208, 224, 255, 296: two and three full intervals
# The pairs of R = 95, 111, 130, 142, 146, 195, 207, 255 and 296 have E % 16 != 0: the BPTT tiles are ragged too.
ROWS = [(1, 2), (3, 6), (3, 11), (32, 2), (5, 13), (19, 5), (37, 3), (16, 8), (65, 2), (71, 2), (16, 9), (73, 2), (16, 10), (16, 11),
        (32, 6), (65, 3), (23, 9), (16, 13), (32, 7), (51, 5), (37, 8)]
# the reduced set of the other three widths: every tail length behind a full interval once, odd and 15-row last sub-chunks, no full interval
ROWS_REDUCED = [(5, 13), (73, 2), (65, 3), (23, 9), (51, 5)]
# many64 (s_upd = 2): split boundaries off the 16-row grid and a short last split -- N = 297: R = 150 | 147 in dwxh and 160 | 137 in
# dx1w1 / fc_bwd; N = 295: 148 | 147 and 160 | 135
ROWS_64 = [(27, 11), (59, 5)]
# fused against grouped GEMMs, and PPO: a full interval and a ragged tail
ROWS_FUSED = [(73, 2), (23, 9), (51, 5)]
PPO_ROWS = (23, 9, 5, 7, 5e-2)          # (E, T, init seed, rollout seed, lr) on many65, K = 2: epoch 1 takes the re-forward path
WS_EDGE_BATCH = (3, 2)
TIME_LAYOUTS, TIME_BATCHES = ['head8', 'edges160'], [(37, 1), (5, 2), (37, 2)]      # the edges of the lstm_fwd / lstm_bwd2 prefetch pipelines
DONE_PATTERNS = [('always', 1.0), ('never', 0.0)]       # on head8, T = 7: h_prev masked at every step / never after the reset
DONE_BATCH = (37, 7)

IQL_LAYOUTS.update({
    'q130_fused': _iql('dqn', 128, 64, 48, _cycle(_Q160, 130), True, '130 agents inside the fused limits'),
    'q130_grouped': _iql('dqn', 64, 32, 36, _cycle(_LG_IQL, 130), False, '130 agents on the grouped path'),
})
_SEED_ORDER += list(A2C_COUNT_LAYOUTS) + ['q130_fused', 'q130_grouped']

# The batches of the GPU module: A2C (E, T) -- N = 30 and N = 259 rows, ragged in every row loop; IQL E instances, ring capacity
A2C_BATCHES = [(5, 6), (37, 7)]
A2C_FORWARD_E, A2C_FORWARD_STEPS = 37, 3
IQL_E, IQL_CAP, IQL_STEPS = 5, 30, 2
IQL_REWARD_NORM = 100.0

# name -> seed of the weight init and of the rollouts (data_seed).  Chosen on the host (tests/test_layouts_host.py states what they must satisfy: few hidden units on a ReLU
# kink, no saturated head, float32 drift of the second round inside its allowance); the GPU module takes the same table.
SEEDS = {name: 5 for name in list(A2C_LAYOUTS) + list(IQL_LAYOUTS)}
SEEDS.update(tiny=11, q_small=6)        # 5 fails there: tiny 5 - 10 put more than 4 columns of a one-input block on a kink, q_small 5 a second-layer unit
# the same for the layouts of the agent-count axis: 5 meets every condition of tests/test_layouts_host.py::test_count_update_conditions
COUNT_SEEDS = {name: 5 for name in A2C_COUNT_LAYOUTS}


def seed_of(name):
    return SEEDS[name] if name in SEEDS else COUNT_SEEDS[name]


# PPO on head8 (MA2C, LSTM, K = 3): (E, T, init seed, rollout seed, lr) under tests/ppo_oracle.py's k3_conditions
PPO_HEAD8 = (16, 8, 5, 7, 5e-2)


def data_seed(name, E, T=0):
    """RandomState seed of a case's rollout: one stream per (layout, batch), moved by the layout's entry in SEEDS -- a layout whose
    agents have one or two inputs needs a rollout without an input within ~1e-3 of zero (after the first update the biases are
    ~1e-4, and such a sample puts many hidden units of the block on their kink at once)."""
    return 100000 * (_SEED_ORDER.index(name) + 1) + 1000 * seed_of(name) + 10 * E + T


def rand_obs(lay, E, rng):
    """tests/test_model_gpu.py::_rand_obs: uniform [0, 2) on an agent's own inputs, zero padding behind them."""
    obs = np.zeros((E, lay.n_agent, lay.s_max), np.float32)
    for a, n in enumerate(lay.n_s_ls):
        obs[:, a, :n] = rng.rand(E, n).astype(np.float32) * 2
    return obs


def forward_inputs(lay, E, steps, rng):
    """The (obs, done) pairs of tests/test_model_gpu.py::_forward_vs_oracle, then the bootstrap observation."""
    out = []
    for t in range(steps):
        obs = rand_obs(lay, E, rng)
        out.append((obs, (rng.rand(E) < (1.0 if t == 0 else 0.3)).astype(np.uint8)))
    return out, rand_obs(lay, E, rng)


def fill_host(lay, oracles, E, T, rng, reward_norm, p_done=0.1, terminal=False, sel=None):
    """tests/test_model_gpu.py::_fill without a device: the same draws in the same order.  The stored value is the first oracle's,
    rounded to float32 (on the GPU: the kernel's).  sel: the oracles hold these agents only (the draws are those of the whole layout).
    -> (next obs, carried done, list of per-step pi of the first oracle)."""
    pk = (lambda x: x) if sel is None else (lambda x: x[:, sel])
    obs, done, pis = rand_obs(lay, E, rng), np.ones(E, np.uint8), []
    for t in range(T):
        v = None
        for o in oracles:
            pi, ov = o.forward(pk(obs), done, 'pv')
            if v is None:
                v = np.asarray(ov, np.float64).astype(np.float32)
                pis.append(pi)
        act = np.stack([rng.randint(0, n, E) for n in lay.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, lay.n_agent) * 3.0 * reward_norm
        dpost = (rng.rand(E) < p_done).astype(np.uint8)
        if terminal and t == T - 1:
            dpost[:] = 1
        for o in oracles:
            o.add_transition(pk(obs), done, pk(act), pk(rew), v, dpost)
        obs, done = rand_obs(lay, E, rng), dpost
    return obs, done, pis


def iql_transitions(lay, E, cap, rng, reward_norm):
    """The transitions of tests/iql_harness.py::replay_vs_oracle (E < 100): -> list of (obs, act, rew, next obs, done)."""
    out, obs = [], rand_obs(lay, E, rng)
    for t in range(cap + 7):
        nobs = rand_obs(lay, E, rng)
        act = np.stack([rng.randint(0, n, E) for n in lay.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, lay.n_agent) * 3.0 * reward_norm
        done = (rng.rand(E) < 0.1).astype(np.uint8)
        out.append((obs, act, rew, nobs, done))
        obs = nobs
    return out


@contextlib.contextmanager
def oracle_dtype(dt):
    """Run oracle.nets_oracle / oracle.iql_oracle in another floating-point type: the float32 restatement of the float64 oracles (same
    code, torch float32 on the CPU), whose distance to float64 is what a correct float32 kernel may show."""
    from oracle import iql_oracle, nets_oracle
    saved = nets_oracle.DT, iql_oracle.DT
    nets_oracle.DT = iql_oracle.DT = dt
    try:
        yield
    finally:
        nets_oracle.DT, iql_oracle.DT = saved


def f32_oracle_class(base):
    """A subclass of an oracle class whose every public method runs under oracle_dtype(torch.float32)."""
    import torch

    def wrap(fn):
        def inner(*a, **k):
            with oracle_dtype(torch.float32):
                return fn(*a, **k)
        return inner

    body = {}
    for klass in reversed(base.__mro__[:-1]):
        for k, v in vars(klass).items():
            if callable(v) and not isinstance(v, (staticmethod, classmethod)) and (not k.startswith('__') or k == '__init__'):
                body[k] = wrap(getattr(base, k))
    return type(base.__name__ + 'F32', (base,), body)


def count_cases():
    """Every update case the agent-count, row-split and time axes add to tests/test_layouts_gpu.py, one tuple per rollout stream:
    (group, layout name, policy, E, T, rounds, first round ends on a terminal step, p_done).  The GPU module runs each (some with the
    activation cache on and off: the draws do not depend on it); tests/test_layouts_host.py states the oracle-only conditions of each."""
    out = []
    for name in ('solo', 'many64', 'many65', 'many130'):
        out += [('count', name, p, E, T, 2, False, 0.1) for p in ('lstm', 'fc') for E, T in A2C_BATCHES]
    out += [('rows', 'many65', p, E, T, 1, False, 0.1) for p in ('lstm', 'fc') for E, T in ROWS]
    out += [('rows', n, p, E, T, 1, False, 0.1) for n in ROW_WIDTHS for p in ('lstm', 'fc') for E, T in ROWS_REDUCED]
    out += [('rows', 'many64', p, E, T, 1, False, 0.1) for p in ('lstm', 'fc') for E, T in ROWS_64]
    out += [('time', n, p, E, T, 2, True, 0.1) for n in TIME_LAYOUTS for p in ('lstm', 'fc') for E, T in TIME_BATCHES]
    out += [('done', 'head8', 'lstm', DONE_BATCH[0], DONE_BATCH[1], 2, False, pd) for _, pd in DONE_PATTERNS]
    # (the update runs past the workspace edge only; at 340 agents the GPU module asserts the plan)
    out += [('edge', 'ws_edge_341', 'lstm', WS_EDGE_BATCH[0], WS_EDGE_BATCH[1], 1, False, 0.1)]
    return out


def spec_of(name):
    return A2C_LAYOUTS[name] if name in A2C_LAYOUTS else A2C_COUNT_LAYOUTS[name]


# ---- value regimes ------------------------------------------------------------------------------------------------------------------
# Every layout above keeps the VALUES in the regime of the initialisation: probabilities between 0.06 and 0.6, gradient norms below
# max_grad_norm.  A regime is a transform of the per-tower dicts (even towers are the policy towers) that leaves that corner:
# name -> policy -> (scale of the policy head out_w / out_b, scale of the recurrent or second layer of BOTH towers, one-hot bias).
#   peaked     the policy head scaled up: a share of the taken actions below the 1e-10 clamp of log pi, every agent's norm above the clip
#   half_clip  a smaller scale: agents on both sides of max_grad_norm in one launch
#   gates      a peaked head, and lstm_wx / lstm_wh / lstm_b (policy 'fc': fc_w / fc_b) scaled on both towers: saturated gates
#   onehot     policy out_b[a % n_a] += 200 for agent a: pi exactly one-hot in float32
# The scales were chosen on the host (tests/test_regimes_host.py states what each must produce on the cases of regime_cases(), ten
# rollout streams tried per case, REGIME_STREAM).  Starting points were 30 / 8 / (30, 6) for both policies; they moved because
#   * LSTM, peaked 30: on edges192 at N = 30 at most 2.7 % of the taken actions fall below the clamp in any stream (45: 8 %);
#   * FC, peaked 30: the head input is a ReLU layer, not h in (-1, 1), so the logits are larger: the two-action agent of head8 saturates
#     (every gradient of its policy tower below 1e-7) or stays below the clip; 12 leaves edges192 under 5 % below the clamp; 16 meets both;
#   * FC, gates (30, 6): the restatement's |dpi| leaves half the bound; (16, 2) saturates the two-action agent again, (12, 2) does not;
#   * half_clip 8: every FC agent clips (norms 74 - 175; 3: 28 - 62), and at the learning rate the clip check needs (HALF_CLIP_LR) every
#     LSTM agent of head8 at N = 259 clips in the second round (7: 37 - 75).
REGIMES = {'peaked': {'lstm': (45.0, 1.0, 0.0), 'fc': (16.0, 1.0, 0.0)}, 'half_clip': {'lstm': (7.0, 1.0, 0.0), 'fc': (3.0, 1.0, 0.0)},
           'gates': {'lstm': (45.0, 6.0, 0.0), 'fc': (12.0, 2.0, 0.0)}, 'onehot': {'lstm': (1.0, 1.0, 200.0), 'fc': (1.0, 1.0, 200.0)}}
CLAMP = 1e-10                           # tf.clip_by_value(pi, 1e-10, 1) of the loss (agents/policies.py:41-52)
REGIME_FORWARD_LAYOUTS = ['head8', 'h96', 'h124', 'edges192']
REGIME_PPO = (16, 8, 5, 7, 5e-5)        # (E, T, init seed, rollout seed, lr) on head8, 'peaked', K = 2
HALF_CLIP_LR = 2e-3                     # tests/test_regimes_gpu.py: the learning rate at which a wrong clip factor shows in the parameters


# (regime, layout, policy, E, T) -> which of ten rollout streams the case takes, where stream 0 misses a condition of the host module
REGIME_STREAM = {('half_clip', 'edges192', 'fc', 5, 6): 1, ('gates', 'head8', 'fc', 37, 7): 1, ('half_clip', 'head8', 'fc', 5, 6): 4,
                 ('gates', 'head8', 'fc', 5, 6): 1, ('half_clip', 'edges192', 'lstm', 5, 6): 2, ('gates', 'head8', 'lstm', 37, 7): 4}


def regime_data_seed(regime, name, policy, E, T):
    """RandomState seed of a regime case's rollout: data_seed's stream of the batch, or one of nine more (REGIME_STREAM)."""
    return data_seed(name, E, T) + 7919 * REGIME_STREAM.get((regime, name, policy, E, T), 0)


def apply_regime(towers, name, lay):
    """The towers (list of per-tower dicts as VecA2C.get_tower_params / init_tower_params return them, ALL agents of lay) under a
    regime of REGIMES -> a new list; float32 arithmetic, so that the host module and a device handle hold the same bits."""
    head, rec, hot = (np.float32(x) for x in REGIMES[name]['fc' if 'fc_w' in towers[0] else 'lstm'])
    out = [{k: np.array(v, np.float32) for k, v in p.items()} for p in towers]
    assert len(out) == 2 * lay.n_agent
    for t, p in enumerate(out):
        if t % 2 == 0:
            p['out_w'], p['out_b'] = p['out_w'] * head, p['out_b'] * head
            if hot:
                p['out_b'][(t // 2) % lay.n_a_ls[t // 2]] += hot
        for k in ('lstm_wx', 'lstm_wh', 'lstm_b', 'fc_w', 'fc_b'):
            if k in p:
                p[k] = p[k] * rec
    return out


def clip_step_gap(grads, ms, norms, clip, lr, alpha=0.99, eps=1e-5):
    """What a wrong clip factor moves: per agent whose norm exceeds clip, the largest |parameter step with factor 1 - step with clip /
    norm| over its entries under RMSProp (ms before the step) -> the largest of those figures over the clipped agents.
    grads, ms: per-tower dicts of float64 arrays."""
    def step(g, m, sc):
        g = g * sc
        return lr * g / np.sqrt(alpha * m + (1 - alpha) * g * g + eps)
    gaps = []
    for a, nrm in enumerate(norms):
        if nrm > clip:
            gaps.append(max(float(np.abs(step(np.asarray(g), np.asarray(ms[t][k]), 1.0) - step(np.asarray(g), np.asarray(ms[t][k]), clip / nrm)).max())
                            for t in (2 * a, 2 * a + 1) for k, g in grads[t].items()))
    return max(gaps)


def onehot_action(lay):
    """The action the `onehot` regime gives all of an agent's probability."""
    return [a % n for a, n in enumerate(lay.n_a_ls)]


# ---- the Q-learners' regimes: one fused and one grouped layout of IQL_LAYOUTS, and IQL-LR
IQL_REGIME_LAYOUTS = ['q160_edge', 'q_small', 'lr_tiny']
IQL_CLIP_SCALE = {'q160_edge': 5.0, 'q_small': 3.0, 'lr_tiny': 10.0}    # head scale of the `clip` regime per layout, chosen on the host
IQL_CLIP_STEPS, IQL_CLIP_LR = 3, 1e-3


def adam_step_bound(d_ref, w):
    """Bound on |d step| of one tensor in the `clip` regime's Adam steps (second moments preloaded with 1, so that a step is nearly linear
    in the clipped gradient): the gradient tolerance 2e-5 max|g| per tensor and the clip norm's rtol 1e-4 carry over to the step as
    1.2e-4 max|step|; on top the float32 rounding of the parameter itself, 2^-23 max|w|."""
    return 1.2e-4 * float(np.abs(d_ref).max()) + 2.0 ** -23 * float(np.abs(w).max())


def tie_pair(a, na):
    """The two head columns j < k of agent a the `tied` regime makes identical."""
    return a % (na - 1), na - 1


def apply_iql_regime(agents, regime, name):
    """Per-agent parameter dicts (VecIQL.get_agent_params / init_agent_params) of layout `name` under a Q-learner regime -> new list.
      tied  head column k = column j (weights and bias), every other column's bias lowered by 50: the pair is the maximum on every row
      flat  head weights and bias zero: Q is exactly 0, every action ties
      clip  head weights and bias x IQL_CLIP_SCALE[name]: gradient norms on both sides of max_grad_norm"""
    out = [{k: np.array(v, np.float32) for k, v in p.items()} for p in agents]
    for a, p in enumerate(out):
        na = p['q_b'].shape[0]
        if regime == 'tied':
            j, k = tie_pair(a, na)
            p['q_w'][:, k], p['q_b'][k] = p['q_w'][:, j], p['q_b'][j]
            p['q_b'][[c for c in range(na) if c not in (j, k)]] -= np.float32(50.0)
        elif regime == 'flat':
            p['q_w'][:], p['q_b'][:] = 0, 0
        else:
            assert regime == 'clip'
            p['q_w'], p['q_b'] = p['q_w'] * np.float32(IQL_CLIP_SCALE[name]), p['q_b'] * np.float32(IQL_CLIP_SCALE[name])
    return out


def regime_cases():
    """Every update case of tests/test_regimes_gpu.py, one tuple per rollout stream: (regime, layout, policy, E, T)."""
    out = [(r, 'head8', p, E, T) for r in ('peaked', 'half_clip', 'gates') for p in ('lstm', 'fc') for E, T in A2C_BATCHES]
    out += [(r, 'edges192', p) + A2C_BATCHES[0] for r in ('peaked', 'half_clip', 'gates') for p in ('lstm', 'fc')]
    out += [('peaked', n, p) + A2C_BATCHES[0] for n in ('h96', 'h124') for p in ('lstm', 'fc')]
    out += [('onehot', 'head8', p, E, T) for p in ('lstm', 'fc') for E, T in A2C_BATCHES]
    return out


def regime_forward_cases():
    return [(r, n, p) for r in ('peaked', 'gates', 'onehot') for n in REGIME_FORWARD_LAYOUTS for p in ('lstm', 'fc')]


def pick_of(name):
    """The agents the oracle evaluates on a layout: all of them on the small ones (None), pick() from 64 agents on."""
    A = spec_of(name)['layout'].n_agent
    return pick(A) if A >= 64 else None
