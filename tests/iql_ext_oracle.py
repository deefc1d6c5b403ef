"""Float64 restatement of the opt-in extensions of the Q-learners -- TEST INFRASTRUCTURE ONLY, never the code under test.  ExtOracleQ /
ExtOracleIQL extend oracle.iql_oracle.OracleQ / OracleIQL (their nets, rings, clip + Adam), which stay the restatement of the reference,
with four options that combine freely:

target network / Double DQN (include/tsc.h tsc_iql_set_target)
  * `target`: a second parameter dict theta-, a copy of the parameters when the oracle is made;
  * the two targets   y = done ? r : r + gamma max_j Q_theta-(s')[j]                         (double_q = 0)
                      a* = argmax_j Q_theta(s')[j] (np.argmax: first maximum);
                      y = done ? r : r + gamma Q_theta-(s')[a*]                               (double_q = 1)
  * the refresh theta- <- theta after every `target_update`-th Adam step, counted by the oracle's Adam counter t;  target_update = 0
    means no target network: theta- follows theta before every loss (the net being updated evaluates s'), and double_q needs one.

prioritized replay (tsc_iql_set_per; proportional, Schaul et al. 2016), `per`
  * stored priorities prio[E][A][cap] (float32 values: what the device stores) and running maxima qmax[E][A], 1 when the oracle is made;
    a new transition enters its ring at the ring's qmax;
  * the stratified proportional draw with replacement of one ring: C[k] = sum_{s <= k} q[s] over the filled slots (float64),
    t_i = (i + U_i) C[size - 1] / B, pick i = the smallest k with C[k] > t_i, clamped to the last slot with q > 0;
  * the importance weights w_i = (size q[k_i] / total)^-beta, divided by the largest of the ring's B weights;
  * the write-back q[k_i] = float32((|delta_i| + eps)^alpha) in pick order, qmax = the running maximum;
  without it the draw is oracle.iql_oracle.floyd_sample's and every row weighs 1.

dueling head (tsc_iql_set_dueling; Wang et al. 2016), chosen by the parameters: a dict with v_w / v_b is the net
    h = the hidden layers of oracle.iql_oracle.q_net;  A = h q_w + q_b  [n_a];  V = h v_w + v_b  [1]
    Q[j] = V + A_j - (1 / n_a) sum_{k < n_a} A_k
  wherever a Q value is used: forward, max_j Q(s'), Double DQN's a* and picked value, Q(s)[a], |delta|.

multi-step returns (tsc_iql_set_return_steps; INTEGRATION.md "Multi-step returns"), `return_steps` = None | n >= 1
  * nstep_window: the rule in plain Python, for one sampled slot of one ring;
  * every minibatch row is assembled from its ring -- observation and action of the sampled slot s; the return G, the discount gamma^k,
    the next observation and the done flag of the bootstrap slot j -- and y = done ? G : G + gamma^k Qsel(s').  return_steps = 1 runs the
    window code too (k = 1 on every row); None is the stored tuple of slot s and the scalar gamma.  The draw, the importance weights and
    the priority write-back (slot s) do not change;
  * `last_slot` [E][A][B] and `last_G`, `last_disc`, `last_k`, `last_s` [A][E * B] keep the windows of the last minibatch_step (float64,
    not rounded).  A window is `wrapped` when its bootstrap slot lies before its sampled slot: the walk crossed cap - 1 -> 0.

The loss is mean(w (Q_theta(s)[a] - stop_grad(y))^2), its gradient torch autograd's.  `last_y`, `last_astar`, `last_q1_online`,
`last_q1_target`, `last_delta` keep the targets, the picks, both nets' Q(s') and delta of the last loss_and_grads; `last_w`, `last_td`
[A][E * B] and `last_idx` the weights, |delta| and draw of the last minibatch_step.  The floating-point type is oracle.iql_oracle.DT
when a method runs (tests/layouts.oracle_dtype)."""
import numpy as np
import torch

from oracle import iql_oracle
from oracle.iql_oracle import OracleIQL, OracleQ, floyd_sample, q_net


def q_net_duel(p, S, n_s, n_w):
    """p: dict of float64 tensors {fcw_w, fcw_b, [fct_w, fct_b], fc0_w, fc0_b, q_w, q_b, v_w, v_b} -> combined Q [rows, n_a]."""
    h = torch.relu(S[:, :n_s] @ p['fcw_w'] + p['fcw_b'])
    if n_w:
        h = torch.cat([h, torch.relu(S[:, n_s:] @ p['fct_w'] + p['fct_b'])], 1)
    h = torch.relu(h @ p['fc0_w'] + p['fc0_b'])
    adv = h @ p['q_w'] + p['q_b']
    val = h @ p['v_w'] + p['v_b']
    return val + adv - adv.mean(1, keepdim=True)


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


class ExtOracleQ(OracleQ):
    def __init__(self, params, n_s, n_w, gamma=0.99, max_grad_norm=40.0, target_update=0, double_q=False):
        super().__init__(params, n_s, n_w, gamma, max_grad_norm)
        assert target_update >= 0 and not (double_q and not target_update), 'Double DQN needs a target network'
        self.target_update, self.double_q = int(target_update), bool(double_q)
        self.weights = None                                   # per-row loss weights of the next loss; None: every row weighs 1
        self.row_disc = None                                  # per-row discounts of the next loss; None: self.gamma on every row
        self.sync_target()
        self.last_y = self.last_astar = self.last_q1_online = self.last_q1_target = self.last_delta = None

    def net(self, p, S):
        return (q_net_duel if 'v_w' in p else q_net)(p, S, self.n_s, self.n_w)

    def forward(self, ob):
        with torch.no_grad():
            return self.net(self.p, torch.as_tensor(np.asarray(ob)[None], dtype=iql_oracle.DT))[0].numpy()

    def sync_target(self):
        self.target = {k: v.clone() for k, v in self.p.items()}

    def set_target(self, params):
        self.target = {k: torch.as_tensor(np.asarray(v), dtype=iql_oracle.DT).clone() for k, v in params.items()}

    def targets(self, next_obs, dones, rs, disc=None):
        """disc: the rows' discounts, a tensor in row order, or None for self.gamma.
        -> (y, a* or None, online Q(s'), target Q(s')) as float64 tensors."""
        S1 = torch.as_tensor(np.asarray(next_obs), dtype=iql_oracle.DT)
        with torch.no_grad():
            qt = self.net(self.target, S1)
            qo = self.net(self.p, S1)
            if self.double_q:
                astar = torch.as_tensor(np.argmax(qo.numpy(), 1))                     # first maximum
                q1 = qt.gather(1, astar[:, None])[:, 0]
            else:
                astar, q1 = None, qt.max(1).values
            r = torch.as_tensor(np.asarray(rs), dtype=iql_oracle.DT)
            d = torch.as_tensor(np.asarray(dones).astype(bool))
            return torch.where(d, r, r + (self.gamma if disc is None else disc) * q1), astar, qo, qt

    def loss_and_grads(self, obs, acts, next_obs, dones, rs):
        if not self.target_update:
            self.sync_target()
        P = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        S = torch.as_tensor(np.asarray(obs), dtype=iql_oracle.DT)
        q0 = self.net(P, S).gather(1, torch.as_tensor(np.asarray(acts), dtype=torch.long)[:, None])[:, 0]
        disc = None
        if self.row_disc is not None:
            assert len(self.row_disc) == len(rs)
            disc = torch.as_tensor(np.asarray(self.row_disc, np.float64), dtype=iql_oracle.DT)
        y, astar, qo, qt = self.targets(next_obs, dones, rs, disc)
        self.last_y, self.last_q1_online, self.last_q1_target = y.numpy().copy(), qo.numpy().copy(), qt.numpy().copy()
        self.last_astar = None if astar is None else astar.numpy().astype(np.int32)
        w = torch.ones_like(y) if self.weights is None else torch.as_tensor(np.asarray(self.weights), dtype=iql_oracle.DT)
        d = q0 - y
        self.last_delta = d.detach().numpy().copy()
        loss = (w * d ** 2).mean()
        loss.backward()
        return loss.item(), {k: v.grad.detach() for k, v in P.items()}

    def backward(self, obs, acts, next_obs, dones, rs, lr):
        out = super().backward(obs, acts, next_obs, dones, rs, lr)       # (uses this class's loss_and_grads), self.t += 1
        if not self.target_update or self.t % self.target_update == 0:      # no target network: theta- is theta after the step as well
            self.sync_target()
        return out


class ExtOracleIQL(OracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, per=False, alpha=0.6, eps=0.01, target_update=0, double_q=False,
                 return_steps=None, gamma=0.99, max_grad_norm=40.0, **kw):
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, gamma=gamma, max_grad_norm=max_grad_norm, **kw)
        assert return_steps is None or int(return_steps) >= 1
        self.return_steps, self.gamma = None if return_steps is None else int(return_steps), float(gamma)
        self.last_slot = self.last_G = self.last_disc = self.last_k = self.last_s = None
        self.qs = [ExtOracleQ(p, nw, nt, gamma, max_grad_norm, target_update, double_q) for p, nw, nt in zip(agent_params, n_wave_ls, n_w_ls)]
        self.per, self.alpha, self.eps = bool(per), float(alpha), float(eps)
        self.prio = np.zeros((self.E, self.A, self.cap), np.float32)
        self.qmax = np.ones((self.E, self.A), np.float32)
        self.last_w = self.last_td = None

    def set_target_params(self, agent_params):
        for q, p in zip(self.qs, agent_params):
            q.set_target(p)

    def target_params(self):
        return [{k: v.numpy().astype(np.float32) for k, v in q.target.items()} for q in self.qs]

    def forward(self, obs):
        """obs [E, A, SMAX] -> list[A] of q [E, n_a] (float64; the combined values of a dueling agent)."""
        out = []
        for a, q in enumerate(self.qs):
            n = self.nw[a] + self.nt[a]
            with torch.no_grad():
                out.append(q.net(q.p, torch.as_tensor(np.asarray(obs)[:, a, :n], dtype=iql_oracle.DT)).numpy())
        return out

    def add_transition(self, obs, actions, rewards, next_obs, done):
        slot = self.rings[0][0].cum_size % self.cap
        super().add_transition(obs, actions, rewards, next_obs, done)
        if self.per:
            self.prio[:, :, slot] = self.qmax

    def row(self, e, a, s, log):
        """The minibatch row of slot s of ring (e, a) -> (obs, action, reward or return, next obs, done).  return_steps = None: the stored
        tuple.  Else the row of the window from s, which is appended to log as (s, j, G, gamma^k, k)."""
        buf = self.rings[e][a].buffer
        if self.return_steps is None:
            return buf[s]
        ring = self.rings[e][a]
        j, G, disc, k = nstep_window([t[2] for t in buf], [t[4] for t in buf], s, ring.size, self.cap, ring.cum_size, self.return_steps,
                                     self.gamma)
        log.append((s, j, G, disc, k))
        return buf[s][0], buf[s][1], G, buf[j][3], buf[j][4]

    def minibatch_step(self, lr, beta=1.0, idx_given=None):
        """-> (per-agent loss, per-agent grad norm, grads list[A] of dict); applies Adam and, with per, the priority write-back.
        idx_given [E, A, B]: the caller's draw, clamped into [0, size) as include/tsc.h documents for the device (with per the weights
        still come from the priorities of those slots)."""
        from oracle.nets_oracle import sample_uniform
        size, B = self.rings[0][0].size, self.B
        idx = np.zeros((self.E, self.A, B), np.int32)
        self.last_w, self.last_td = np.ones((self.A, self.E * B)), np.zeros((self.A, self.E * B))
        losses, norms, grads, logs = [], [], [], []
        for a, q in enumerate(self.qs):
            obs, acts, nobs, rs, dones, log = [], [], [], [], [], []
            for e in range(self.E):
                uniform = lambda i, p=e * self.A + a: sample_uniform(self.replay_seed, self.update_step, p * B + i)
                if idx_given is not None:
                    ids = [min(max(int(x), 0), size - 1) for x in idx_given[e, a]]
                elif self.per:
                    ids = per_draw(self.prio[e, a], size, B, uniform)
                else:
                    ids = floyd_sample(size, B, uniform)
                idx[e, a] = ids
                if self.per:
                    self.last_w[a, e * B:(e + 1) * B] = per_weights(self.prio[e, a], size, ids, beta)
                for s in ids:
                    ob, ac, r, nob, d = self.row(e, a, s, log)
                    obs.append(ob); acts.append(ac); rs.append(r); nobs.append(nob); dones.append(d)
            logs.append(log)
            q.weights = self.last_w[a] if self.per else None
            q.row_disc = None if self.return_steps is None else [w[3] for w in log]
            loss, g = q.loss_and_grads(obs, acts, nobs, dones, rs)
            self.last_td[a] = np.abs(q.last_delta)
            grads.append({k: v.numpy().copy() for k, v in g.items()})
            _, norm = q.backward(obs, acts, nobs, dones, rs, lr)
            q.row_disc = None
            losses.append(loss); norms.append(norm)
            if self.per:
                for e in range(self.E):
                    for i, s in enumerate(idx[e, a]):
                        v = per_priority(self.last_td[a, e * B + i], self.eps, self.alpha)
                        self.prio[e, a, s] = v
                        self.qmax[e, a] = max(self.qmax[e, a], v)
        self.update_step += 1
        self.last_idx = idx
        if self.return_steps is not None:
            win = np.array(logs, np.float64)                          # [A][R][5]
            self.last_s, self.last_k = win[:, :, 0].astype(np.int64), win[:, :, 4].astype(np.int32)
            self.last_G, self.last_disc = win[:, :, 2].copy(), win[:, :, 3].copy()
            self.last_slot = win[:, :, 1].astype(np.int32).reshape(self.A, self.E, self.B).transpose(1, 0, 2).copy()
        return np.array(losses), np.array(norms), grads

    def categories(self):
        """-> dict of bool [A][R] over the rows of the last minibatch_step: full horizon (k = n), cut by done, cut by the newest slot,
        wrapped window.  (A row can be in several: the done slot can be the newest one, a full window can end on either.)"""
        w = (self.rings[0][0].cum_size - 1) % self.cap
        j = self.last_slot.transpose(1, 0, 2).reshape(self.A, -1)
        done_j = np.array([[self.rings[r // self.B][a].buffer[j[a, r]][4] for r in range(j.shape[1])] for a in range(self.A)], bool)
        return dict(full=self.last_k == self.return_steps, done=done_j, newest=(j == w) & ~done_j, wrapped=j < self.last_s)
