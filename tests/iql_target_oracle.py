"""Float64 restatement of the opt-in target network / Double DQN of the Q-learners (include/tsc.h tsc_iql_set_target) -- TEST
INFRASTRUCTURE ONLY, never the code under test.  TargetOracleQ / TargetOracleIQL extend oracle.iql_oracle.OracleQ / OracleIQL
(their nets, rings, clip + Adam) with

  * `target`: a second parameter dict theta-, a copy of the parameters when the oracle is made;
  * the two targets   y = done ? r : r + gamma max_j Q_theta-(s')[j]                         (double_q = 0)
                      a* = argmax_j Q_theta(s')[j] (np.argmax: first maximum);
                      y = done ? r : r + gamma Q_theta-(s')[a*]                               (double_q = 1)
    with the loss mean((Q_theta(s)[a] - stop_grad(y))^2) unchanged;
  * the refresh theta- <- theta after every `target_update`-th Adam step, counted by the oracle's Adam counter t.

`last_y`, `last_astar`, `last_q1_online`, `last_q1_target` keep the targets, the picks and both nets' Q(s') of the last loss_and_grads."""
import numpy as np
import torch

from oracle.iql_oracle import DT, OracleIQL, OracleQ, q_net


class TargetOracleQ(OracleQ):
    def __init__(self, params, n_s, n_w, gamma=0.99, max_grad_norm=40.0, target_update=1, double_q=False):
        super().__init__(params, n_s, n_w, gamma, max_grad_norm)
        assert target_update > 0
        self.target_update, self.double_q = int(target_update), bool(double_q)
        self.sync_target()
        self.last_y = self.last_astar = self.last_q1_online = self.last_q1_target = None

    def sync_target(self):
        self.target = {k: v.clone() for k, v in self.p.items()}

    def set_target(self, params):
        self.target = {k: torch.as_tensor(np.asarray(v), dtype=DT).clone() for k, v in params.items()}

    def targets(self, next_obs, dones, rs):
        """-> (y, a* or None, online Q(s'), target Q(s')) as float64 tensors."""
        S1 = torch.as_tensor(np.asarray(next_obs), dtype=DT)
        with torch.no_grad():
            qt = q_net(self.target, S1, self.n_s, self.n_w)
            qo = q_net(self.p, S1, self.n_s, self.n_w)
            if self.double_q:
                astar = torch.as_tensor(np.argmax(qo.numpy(), 1))                     # first maximum
                q1 = qt.gather(1, astar[:, None])[:, 0]
            else:
                astar, q1 = None, qt.max(1).values
            r = torch.as_tensor(np.asarray(rs), dtype=DT)
            d = torch.as_tensor(np.asarray(dones).astype(bool))
            return torch.where(d, r, r + self.gamma * q1), astar, qo, qt

    def loss_and_grads(self, obs, acts, next_obs, dones, rs):
        P = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        S = torch.as_tensor(np.asarray(obs), dtype=DT)
        q0 = q_net(P, S, self.n_s, self.n_w).gather(1, torch.as_tensor(np.asarray(acts), dtype=torch.long)[:, None])[:, 0]
        y, astar, qo, qt = self.targets(next_obs, dones, rs)
        self.last_y, self.last_q1_online, self.last_q1_target = y.numpy().copy(), qo.numpy().copy(), qt.numpy().copy()
        self.last_astar = None if astar is None else astar.numpy().astype(np.int32)
        loss = ((q0 - y) ** 2).mean()
        loss.backward()
        return loss.item(), {k: v.grad.detach() for k, v in P.items()}

    def backward(self, obs, acts, next_obs, dones, rs, lr):
        out = super().backward(obs, acts, next_obs, dones, rs, lr)       # (uses this class's loss_and_grads), self.t += 1
        if self.t % self.target_update == 0:
            self.sync_target()
        return out


class TargetOracleIQL(OracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, target_update=1, double_q=False, gamma=0.99,
                 max_grad_norm=40.0, **kw):
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, gamma=gamma, max_grad_norm=max_grad_norm, **kw)
        self.qs = [TargetOracleQ(p, nw, nt, gamma, max_grad_norm, target_update, double_q)
                   for p, nw, nt in zip(agent_params, n_wave_ls, n_w_ls)]

    def set_target_params(self, agent_params):
        for q, p in zip(self.qs, agent_params):
            q.set_target(p)

    def target_params(self):
        return [{k: v.numpy().astype(np.float32) for k, v in q.target.items()} for q in self.qs]
