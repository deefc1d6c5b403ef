"""Float64 restatement of the multi-step (n-step) returns of the Q-learners -- TEST INFRASTRUCTURE ONLY, never the code under test
(include/tsc.h tsc_iql_set_return_steps; INTEGRATION.md "Multi-step returns").  Extends tests/iql_ext_oracle.py:

  * nstep_window: the rule in plain Python, for one sampled slot of one ring;
  * NStepOracleQ(ExtOracleQ): the targets take a discount per row, y = done ? G : G + disc Qsel(s'), in place of self.gamma;
  * NStepOracleIQL(ExtOracleIQL): every minibatch row is assembled from its ring -- observation and action of the sampled slot s; the
    return G, the discount gamma^k, the next observation and the done flag of the bootstrap slot j.  The draw, the importance weights,
    the priority write-back (slot s), clip + Adam and the target refresh are ExtOracleIQL's, untouched: minibatch_step runs the inherited
    method over a view of the rings whose buffer[s] is the assembled row.

`last_slot` [E][A][B] and `last_G`, `last_disc`, `last_k`, `last_s` [A][E * B] keep the windows of the last minibatch_step (float64, not
rounded).  A window is `wrapped` when its bootstrap slot lies before its sampled slot: the walk crossed cap - 1 -> 0."""
import numpy as np
import torch

from oracle import iql_oracle
from tests.iql_ext_oracle import ExtOracleIQL, ExtOracleQ


def nstep_window(rews, dones, s, size, cap, cum, n, gamma):
    """rews / dones: the ring's stored rewards (float32 values) and done flags by slot; s the sampled slot in [0, size); `size` filled
    slots of `cap`, `cum` transitions added so far; horizon n >= 1.  -> (bootstrap slot j, G, gamma^k, k), G and gamma^k as Python
    floats: float64, one rounding per product and per sum."""
    assert 0 <= s < size <= cap and size == min(cum, cap) and n >= 1
    w = (cum - 1) % cap
    j, G, c, k = int(s), 0.0, 1.0, 0
    while True:
        G += c * float(rews[j])
        c *= float(gamma)
        k += 1
        if dones[j] or j == w or k == n:
            return j, G, c, k
        j = (j + 1) % cap


class NStepOracleQ(ExtOracleQ):
    """row_disc: the discounts of the rows of the next loss, in row order (None: self.gamma on every row, ExtOracleQ's targets)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.row_disc = None

    def targets(self, next_obs, dones, rs):
        if self.row_disc is None:
            return super().targets(next_obs, dones, rs)
        assert len(self.row_disc) == len(rs)
        saved, self.gamma = self.gamma, torch.as_tensor(np.asarray(self.row_disc, np.float64), dtype=iql_oracle.DT)
        try:
            return super().targets(next_obs, dones, rs)          # r + gamma q1, element-wise with the rows' own discounts
        finally:
            self.gamma = saved


class _WindowRing:
    """One ring as ExtOracleIQL.minibatch_step reads it: size, and buffer[s] = (obs_s, act_s, G, next_obs_j, done_j).  Every read appends
    the row's window to its agent's list, in the row order of the minibatch."""

    def __init__(self, ring, owner, q, log):
        self.ring, self.owner, self.q, self.log = ring, owner, q, log
        self.buffer = self

    @property
    def size(self):
        return self.ring.size

    def __getitem__(self, s):
        buf, o = self.ring.buffer, self.owner
        j, G, disc, k = nstep_window([t[2] for t in buf], [t[4] for t in buf], s, self.ring.size, o.cap, self.ring.cum_size, o.return_steps,
                                     o.gamma)
        self.q.row_disc.append(disc)
        self.log.append((s, j, G, disc, k))
        return buf[s][0], buf[s][1], G, buf[j][3], buf[j][4]


class NStepOracleIQL(ExtOracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, return_steps=1, target_update=0, double_q=False, gamma=0.99,
                 max_grad_norm=40.0, **kw):
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, target_update=target_update, double_q=double_q, gamma=gamma,
                         max_grad_norm=max_grad_norm, **kw)
        self.qs = [NStepOracleQ(p, nw, nt, gamma, max_grad_norm, target_update, double_q) for p, nw, nt in zip(agent_params, n_wave_ls, n_w_ls)]
        self.return_steps, self.gamma = int(return_steps), float(gamma)
        assert self.return_steps >= 1
        self.last_slot = self.last_G = self.last_disc = self.last_k = self.last_s = None

    def minibatch_step(self, lr, beta=1.0, idx_given=None):
        real = self.rings
        logs = [[] for _ in range(self.A)]
        for q in self.qs:
            q.row_disc = []
        self.rings = [[_WindowRing(real[e][a], self, self.qs[a], logs[a]) for a in range(self.A)] for e in range(self.E)]
        try:
            out = super().minibatch_step(lr, beta, idx_given)
        finally:
            self.rings = real
            for q in self.qs:
                q.row_disc = None
        R = self.E * self.B
        assert all(len(l) == R for l in logs)
        win = np.array(logs, np.float64)                          # [A][R][5]
        self.last_s, self.last_k = win[:, :, 0].astype(np.int64), win[:, :, 4].astype(np.int32)
        self.last_G, self.last_disc = win[:, :, 2].copy(), win[:, :, 3].copy()
        self.last_slot = win[:, :, 1].astype(np.int32).reshape(self.A, self.E, self.B).transpose(1, 0, 2).copy()
        return out

    def categories(self):
        """-> dict of bool [A][R] over the rows of the last minibatch_step: full horizon (k = n), cut by done, cut by the newest slot,
        wrapped window.  (A row can be in several: the done slot can be the newest one, a full window can end on either.)"""
        size, cum = real_size_cum(self)
        w = (cum - 1) % self.cap
        j = self.last_slot.transpose(1, 0, 2).reshape(self.A, -1)
        done_j = np.array([[self.rings[r // self.B][a].buffer[j[a, r]][4] for r in range(j.shape[1])] for a in range(self.A)], bool)
        return dict(full=self.last_k == self.return_steps, done=done_j, newest=(j == w) & ~done_j, wrapped=j < self.last_s)


def real_size_cum(o):
    return o.rings[0][0].size, o.rings[0][0].cum_size
