"""Float64 restatement of the opt-in prioritized replay of the Q-learners (include/tsc.h tsc_iql_set_per; proportional, Schaul et al.
2016) -- TEST INFRASTRUCTURE ONLY, never the code under test.  PerOracleQ / PerOracleIQL extend tests.iql_target_oracle's classes
(their nets, rings, targets, clip + Adam) with

  * stored priorities q[E][A][cap] (float32 values: what the device stores) and running maxima qmax[E][A], 1 when the oracle is made;
    a new transition enters its ring at the ring's qmax;
  * the stratified proportional draw with replacement of one ring: C[k] = sum_{s <= k} q[s] over the filled slots (float64),
    t_i = (i + U_i) C[size - 1] / B, pick i = the smallest k with C[k] > t_i, clamped to the last slot with q > 0;
  * the importance weights w_i = (size q[k_i] / total)^-beta, divided by the largest of the ring's B weights;
  * the loss mean(w (Q(s)[a] - stop_grad(y))^2) with y the target oracle's (target_update = 0: the net being updated evaluates s');
  * the write-back q[k_i] = float32((|delta_i| + eps)^alpha) in pick order, qmax = the running maximum.

`last_w`, `last_td` [A][E * B] keep the weights and |delta| of the last minibatch_step."""
import numpy as np
import torch

from oracle.iql_oracle import DT, q_net
from tests.iql_target_oracle import TargetOracleIQL, TargetOracleQ


def per_draw(q, size, B, uniform):
    """picks [B] of one ring: q its stored priorities (any float array), uniform(i) the i-th uniform of the ring."""
    C = np.cumsum(np.asarray(q[:size], np.float64))
    total = C[-1]
    last = int(np.nonzero(np.asarray(q[:size]) > 0)[0][-1])
    picks = []
    for i in range(B):
        t = (i + uniform(i)) * total / B
        picks.append(min(int(np.searchsorted(C, t, side='right')), last))         # the smallest k with C[k] > t
    return picks


def per_weights(q, size, picks, beta):
    """float64 weights [B] of the picks, normalised by the ring's own maximum."""
    q64 = np.asarray(q[:size], np.float64)
    total = q64.cumsum()[-1]
    w = (size * q64[np.asarray(picks)] / total) ** (-beta)
    return w / w.max()


def per_priority(abs_delta, eps, alpha):
    return np.float32((np.float64(abs_delta) + eps) ** alpha)


class PerOracleQ(TargetOracleQ):
    def __init__(self, params, n_s, n_w, gamma=0.99, max_grad_norm=40.0, target_update=0, double_q=False):
        super().__init__(params, n_s, n_w, gamma, max_grad_norm, max(int(target_update), 1), double_q)
        self.has_target = int(target_update) > 0           # without one theta- follows theta before every loss
        self.weights = None
        self.last_delta = None

    def loss_and_grads(self, obs, acts, next_obs, dones, rs):
        if not self.has_target:
            self.sync_target()
        P = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        S = torch.as_tensor(np.asarray(obs), dtype=DT)
        q0 = q_net(P, S, self.n_s, self.n_w).gather(1, torch.as_tensor(np.asarray(acts), dtype=torch.long)[:, None])[:, 0]
        y, astar, qo, qt = self.targets(next_obs, dones, rs)
        self.last_y = y.numpy().copy()
        w = torch.ones_like(y) if self.weights is None else torch.as_tensor(np.asarray(self.weights), dtype=DT)
        d = q0 - y
        self.last_delta = d.detach().numpy().copy()
        loss = (w * d ** 2).mean()
        loss.backward()
        return loss.item(), {k: v.grad.detach() for k, v in P.items()}


class PerOracleIQL(TargetOracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, alpha=0.6, eps=0.01, target_update=0, double_q=False, gamma=0.99,
                 max_grad_norm=40.0, **kw):
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, target_update=max(int(target_update), 1), double_q=double_q,
                         gamma=gamma, max_grad_norm=max_grad_norm, **kw)
        self.qs = [PerOracleQ(p, nw, nt, gamma, max_grad_norm, target_update, double_q) for p, nw, nt in zip(agent_params, n_wave_ls, n_w_ls)]
        self.alpha, self.eps = float(alpha), float(eps)
        self.prio = np.zeros((self.E, self.A, self.cap), np.float32)
        self.qmax = np.ones((self.E, self.A), np.float32)
        self.last_w = self.last_td = None

    def add_transition(self, obs, actions, rewards, next_obs, done):
        slot = self.rings[0][0].cum_size % self.cap
        super().add_transition(obs, actions, rewards, next_obs, done)
        self.prio[:, :, slot] = self.qmax

    def minibatch_step(self, lr, beta=1.0, idx_given=None):
        """-> (per-agent loss, per-agent grad norm, grads list[A] of dict); applies Adam and the priority write-back.
        idx_given [E, A, B]: the caller's draw (the weights still come from the priorities of those slots)."""
        from oracle.nets_oracle import sample_uniform
        size, B = self.rings[0][0].size, self.B
        idx = np.zeros((self.E, self.A, B), np.int32)
        R = self.E * B
        self.last_w, self.last_td = np.zeros((self.A, R)), np.zeros((self.A, R))
        losses, norms, grads = [], [], []
        for a, q in enumerate(self.qs):
            obs, acts, nobs, rs, dones = [], [], [], [], []
            for e in range(self.E):
                p = e * self.A + a
                ids = (per_draw(self.prio[e, a], size, B, lambda i: sample_uniform(self.replay_seed, self.update_step, p * B + i))
                       if idx_given is None else [min(max(int(x), 0), size - 1) for x in idx_given[e, a]])
                idx[e, a] = ids
                self.last_w[a, e * B:(e + 1) * B] = per_weights(self.prio[e, a], size, ids, beta)
                for s in ids:
                    ob, ac, r, nob, d = self.rings[e][a].buffer[s]
                    obs.append(ob); acts.append(ac); rs.append(r); nobs.append(nob); dones.append(d)
            q.weights = self.last_w[a]
            loss, g = q.loss_and_grads(obs, acts, nobs, dones, rs)
            self.last_td[a] = np.abs(q.last_delta)
            grads.append({k: v.numpy().copy() for k, v in g.items()})
            _, norm = q.backward(obs, acts, nobs, dones, rs, lr)
            losses.append(loss); norms.append(norm)
            for e in range(self.E):
                for i, s in enumerate(idx[e, a]):
                    v = per_priority(self.last_td[a, e * B + i], self.eps, self.alpha)
                    self.prio[e, a, s] = v
                    self.qmax[e, a] = max(self.qmax[e, a], v)
        self.update_step += 1
        self.last_idx = idx
        return np.array(losses), np.array(norms), grads
