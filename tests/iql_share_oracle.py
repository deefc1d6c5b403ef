"""Float64 restatement of a parameter-shared minibatch step of the Q-learners (INTEGRATION.md "Parameter sharing"; include/tsc.h
tsc_iql_set_sharing) -- TEST INFRASTRUCTURE ONLY, never the code under test.  SharedOracleIQL extends tests/iql_ext_oracle.py's
ExtOracleIQL, whose rings, draws, targets, losses and priority write-back stay per agent; a step

  1  collects every agent's float64 gradients (ExtOracleIQL.minibatch_step's own loop, with the Adam step of each agent held back),
  2  replaces each class member's gradients by the class mean (a float64 sum in ascending member order, times 1 / k),
  3  runs the unchanged OracleQ clip + Adam (and ExtOracleQ's target refresh) of every agent on that.

`last_raw` keeps the per-agent gradients of step 1, `last_mean` those of step 2; minibatch_step returns the raw ones (what
tsc_iql_compute_grads leaves in the gradient buffer) and the norms of the class means (what tsc_iql_apply_grads reports).

pooled_grads states what the step is: at equal member parameters the class mean of the members' mean-squared-error gradients is the
gradient of ONE OracleQ on the concatenated rows of all members."""
import numpy as np
import torch

from tests import layouts as LY
from tests.iql_ext_oracle import ExtOracleIQL

# ---- the layouts of tests/test_iql_share_gpu.py (and of tests/test_iql_share_host.py, which states what their seeds must satisfy) ----
_LR_A, _LR_B = (3, 1, 2), (2, 1, 3)
_Q12 = LY._cycle(LY._Q160, 12)
# name -> tests/layouts.py's spec (model type, widths, layout, fused?) with the classes agents.share_classes must find
SHARE_LAYOUTS = {
    'lr4': dict(LY._iql('lr', 128, 64, 4, [_LR_A] * 2 + [(1, 1, 2)] + [_LR_A], False, 'stride 40 = 10 columns: one partial workgroup, a singleton in between'),
                classes=[0, 0, 2, 0]),
    'q160x12': dict(LY._iql('dqn', 128, 64, 48, _Q12, True, 'fused; members not adjacent; a stride of several workgroups, the last ragged'),
                    classes=list(range(6)) * 2),
    'solo': dict(LY._iql('lr', 128, 64, 4, [_LR_A], False, 'one agent'), classes=[0]),
    'lr65': dict(LY._iql('lr', 128, 64, 4, [_LR_A, _LR_B] * 32 + [_LR_A], False, '65 agents in two classes, 33 + 32'), classes=[0, 1] * 32 + [0]),
    # tsc_iql_set_dueling refuses n_a = 8 (column 7 of the head is V): the dueling cases take the agents of q160x12 with n_a <= 7
    'q160x8': dict(LY._iql('dqn', 128, 64, 48, [x for x in _Q12 if x[2] <= 7], True, 'q160x12 under the dueling head'), classes=list(range(4)) * 2),
    'q160x5': dict(LY._iql('dqn', 128, 64, 48, LY._Q160[:3] + LY._Q160[:2], True, 'fused, 2 + 2 + 1: an agent alone in its class'), classes=[0, 1, 2, 0, 1]),
    'q_small': dict(LY.IQL_LAYOUTS['q_small'], classes=[0, 1, 2, 1]),
}
ALL_ARMED = dict(target_update=2, double_q=1, prioritized_replay=1, dueling=1, return_steps=3)
PER_BETA = 0.7
# the update-parity cases: (layout, options, seed of the weights and of the data).  The seeds were chosen on the host: tests/test_iql_share_host.py
# states the conditions (no hidden unit on a ReLU kink, norms below the clip, decided Double DQN picks) and fails for a seed that misses them.
PARITY = [('q160x12', {}, 5), ('q_small', {}, 6), ('lr4', {}, 5), ('q160x8', ALL_ARMED, 6)]      # (q160x8: 5 puts a first-layer unit of agent 6 on a kink in step 1)
PARITY_STEPS, PARITY_LR = 2, 1e-2
# large_grid's own 25 iqld agents (12 + 9 + 4), plain, one step: (E, ring capacity, seed)
GRID_CASE = (3, 25, 5)


def spec_of(name):
    """SHARE_LAYOUTS[name]; 'large_grid': the scenario's iqld agents as a layout (built on first use)."""
    if name == 'large_grid' and name not in SHARE_LAYOUTS:
        from deeprl_signal_control_amd.agents import share_classes
        from deeprl_signal_control_amd.scenario import build_scenario
        scn = build_scenario('large_grid', 'iqld')
        lay = LY.Layout([(s - w, w, 0, a) for s, w, a in zip(scn.n_s_ls, scn.n_w_ls, scn.n_a_ls)], scn.s_max)
        SHARE_LAYOUTS[name] = dict(model_type='dqn', layout=lay, cfg={}, fused=True, why='the 25 agents of large_grid', wide=False,
                                   classes=share_classes(lay.n_wave_ls, lay.n_w_ls, lay.n_f_ls, lay.n_a_ls))
    return SHARE_LAYOUTS[name]


def tie(agents, classes):
    """Per-agent parameter dicts -> a new list in which every agent holds (a copy of) its class's lowest member's."""
    low = {}
    return [{k: np.array(v, np.float32) for k, v in agents[low.setdefault(c, a)].items()} for a, c in enumerate(classes)]


def case_params(name, cfg, seed, target=False):
    """The parameters a shared handle of the case starts from: init_agent_params under `seed` (VecIQL.init_params), a dueling head's biases
    moved off zero (tests/iql_harness.py::nontrivial), every member its class's lowest member's.  target: a second draw (seed + 1000), for a
    frozen copy that disagrees with the parameters."""
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS, QParamLayout, init_agent_params
    from tests.iql_harness import nontrivial
    spec = spec_of(name)
    lay, c = spec['layout'], dict(IQL_DEFAULTS, **spec['cfg'])
    ql = QParamLayout(lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, lay.s_max, spec['model_type'], c['num_fc'], c['num_h'], dueling=bool(cfg.get('dueling')))
    s = seed + (1000 if target else 0)
    agents = init_agent_params(ql, np.random.RandomState(s))
    if cfg.get('dueling'):
        agents = nontrivial(agents, np.random.RandomState(s + 100))
    return tie(agents, spec['classes'])


def case_data(name, seed, E=LY.IQL_E, cap=LY.IQL_CAP, steps=PARITY_STEPS, B=20):
    """-> (transitions of LY.iql_transitions, caller's draws [steps][E][A][B] int32, priorities [E][A][cap] float32) of a parity case: one
    RandomState stream, consumed in this order."""
    lay = spec_of(name)['layout']
    rng = np.random.RandomState(7000 + 100 * seed + len(name))
    trans = LY.iql_transitions(lay, E, cap, rng, LY.IQL_REWARD_NORM)
    size = min(cap, len(trans))
    idx = np.stack([np.stack([np.stack([rng.permutation(size)[:B] for _ in range(lay.n_agent)]) for _ in range(E)]) for _ in range(steps)]).astype(np.int32)
    prio = (10.0 ** rng.uniform(-2, 2, (E, lay.n_agent, cap))).astype(np.float32)
    prio[:, :, size:] = 0
    return trans, idx, prio


def host_oracle(name, cfg, seed, E=LY.IQL_E, cap=LY.IQL_CAP):
    """The shared oracle of a parity case without a device: case_params, the options of cfg, VecIQL's replay seed."""
    from deeprl_signal_control_amd.iql import IQL_DEFAULTS
    spec = spec_of(name)
    lay, c = spec['layout'], dict(IQL_DEFAULTS, **spec['cfg'])
    o = SharedOracleIQL(case_params(name, cfg, seed), lay.n_wave_ls, lay.n_w_ls, lay.n_a_ls, E, classes=spec['classes'],
                        per=bool(cfg.get('prioritized_replay')), alpha=c['per_alpha'], eps=c['per_eps'], target_update=cfg.get('target_update', 0),
                        double_q=bool(cfg.get('double_q')), return_steps=cfg.get('return_steps'), batch_size=20, buffer_size=cap, gamma=c['gamma'],
                        reward_norm=LY.IQL_REWARD_NORM, reward_clip=c['reward_clip'], max_grad_norm=c['max_grad_norm'], replay_seed=seed ^ 0x5DEECE66D)
    if cfg.get('target_update'):
        o.set_target_params(case_params(name, cfg, seed, target=True))
    return o


def preload_second_moments(o):
    """Adam's second moments 1 (first moments 0, t = 0), the precondition of tests/layouts.py::adam_step_bound."""
    for q in o.qs:
        q.v = {k: torch.ones_like(v) for k, v in q.p.items()}


def members_of(classes):
    """class id -> ascending member indices, classes of two or more agents only."""
    out = {}
    for a, c in enumerate(classes):
        out.setdefault(int(c), []).append(a)
    return {c: m for c, m in out.items() if len(m) >= 2}


def class_mean(grads, classes):
    """grads: list[A] of dicts of float64 arrays -> a new list in which every member of a class of two or more holds the class mean."""
    out = [dict(g) for g in grads]
    for members in members_of(classes).values():
        for k in grads[members[0]]:
            acc = np.zeros_like(np.asarray(grads[members[0]][k], np.float64))
            for a in members:
                acc = acc + np.asarray(grads[a][k], np.float64)
            mean = acc * (1.0 / len(members))
            for a in members:
                out[a][k] = mean
    return out


class SharedOracleIQL(ExtOracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, classes=None, **kw):
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, **kw)
        self.classes = list(range(self.A)) if classes is None else [int(c) for c in classes]
        assert len(self.classes) == self.A
        for members in members_of(self.classes).values():
            assert len({(self.nw[a], self.nt[a], self.na[a]) for a in members}) == 1, 'a class of unequal shapes'
        self.last_raw = self.last_mean = None
        self.last_rows = None               # per agent: (obs, acts, next obs, dones, rewards or returns) of the last step, row order

    def minibatch_step(self, lr, beta=1.0, idx_given=None):
        held = []
        for q in self.qs:                   # step 1: the parent's loop; an agent's clip + Adam waits for the class
            q.backward = lambda *args, _h=held: (_h.append(args), (None, None))[1]
        try:
            losses, _, raw = super().minibatch_step(lr, beta=beta, idx_given=idx_given)
        finally:
            for q in self.qs:
                del q.backward
        assert len(held) == self.A
        mean = class_mean(raw, self.classes)                                 # step 2
        norms = []
        for a, q in enumerate(self.qs):                                      # step 3: OracleQ.backward as it is, fed the class mean
            g = {k: torch.as_tensor(np.asarray(v)) for k, v in mean[a].items()}
            q.loss_and_grads = lambda *args, _l=losses[a], _g=g: (_l, _g)
            try:
                _, norm = q.backward(*held[a])
            finally:
                del q.loss_and_grads
            norms.append(norm)
        self.last_raw, self.last_mean = raw, mean
        self.last_rows = [args[:5] for args in held]
        return losses, np.array(norms), raw


def shared_oracle_for(m, classes=None, **over):
    """tests/iql_harness.py::oracle_for with the handle's classes (m.get_sharing() unless given): the options the model was made with."""
    kw = dict(per=bool(m.prioritized_replay), alpha=m.per_alpha, eps=m.per_eps, target_update=m.target_update, double_q=bool(m.double_q),
              return_steps=m.return_steps if m.return_steps > 1 else None, batch_size=m.n_step, buffer_size=int(m.cfg['buffer_size']),
              gamma=m.cfg['gamma'], reward_norm=m.cfg['reward_norm'], reward_clip=m.cfg['reward_clip'], max_grad_norm=m.cfg['max_grad_norm'],
              replay_seed=m.replay_seed)
    kw.update(over)
    return SharedOracleIQL(m.get_agent_params(), m.n_wave_ls, m.n_w_ls, m.n_a_ls, m.E, classes=m.get_sharing() if classes is None else classes, **kw)


def pooled_grads(o, members):
    """One OracleQ-family learner (the first member's, at its parameters) on the concatenated rows the members met in o's last step
    -> (loss, float64 gradient dict).  Uniform row weights only: with prioritized replay a row's weight belongs to its member."""
    q = o.qs[members[0]]
    assert q.weights is None and q.row_disc is None
    rows = [o.last_rows[a] for a in members]
    cat = [[x for r in rows for x in r[i]] for i in range(5)]
    loss, g = q.loss_and_grads(*cat)
    return loss, {k: v.numpy().copy() for k, v in g.items()}
