"""Float64 restatement of the opt-in dueling head of the IQL-DNN learner (include/tsc.h tsc_iql_set_dueling; Wang et al. 2016) -- TEST
INFRASTRUCTURE ONLY, never the code under test.  DuelOracleQ / DuelOracleIQL extend tests.iql_per_oracle's classes (and through them
tests.iql_target_oracle's: nets, rings, targets, weights, clip + Adam) with the net

    h = the hidden layers of oracle.iql_oracle.q_net;  A = h q_w + q_b  [n_a];  V = h v_w + v_b  [1]
    Q[j] = V + A_j - (1 / n_a) sum_{k < n_a} A_k

(q_net_duel; oracle.iql_oracle.q_net cannot take the value stream and stays as it is) wherever a Q value is used: forward, max_j Q(s'),
Double DQN's a* and picked value, Q(s)[a], |delta|.  The gradient is torch autograd's, so dOut is never written down here.

target_update = 0 means no target network (theta- follows theta before every loss, PerOracleQ.has_target), double_q needs one;
per = False draws with Floyd's algorithm and weighs every row 1, per = True is tests.iql_per_oracle's draw, weights and write-back."""
import numpy as np
import torch

from oracle.iql_oracle import DT, OracleIQL
from tests.iql_per_oracle import PerOracleIQL, PerOracleQ


def q_net_duel(p, S, n_s, n_w):
    """p: dict of float64 tensors {fcw_w, fcw_b, [fct_w, fct_b], fc0_w, fc0_b, q_w, q_b, v_w, v_b} -> combined Q [rows, n_a]."""
    h = torch.relu(S[:, :n_s] @ p['fcw_w'] + p['fcw_b'])
    if n_w:
        h = torch.cat([h, torch.relu(S[:, n_s:] @ p['fct_w'] + p['fct_b'])], 1)
    h = torch.relu(h @ p['fc0_w'] + p['fc0_b'])
    adv = h @ p['q_w'] + p['q_b']
    val = h @ p['v_w'] + p['v_b']
    return val + adv - adv.mean(1, keepdim=True)


class DuelOracleQ(PerOracleQ):
    def forward(self, ob):
        with torch.no_grad():
            return q_net_duel(self.p, torch.as_tensor(np.asarray(ob)[None], dtype=DT), self.n_s, self.n_w)[0].numpy()

    def targets(self, next_obs, dones, rs):
        """TargetOracleQ.targets on the combined values -> (y, a* or None, online Q(s'), target Q(s'))."""
        S1 = torch.as_tensor(np.asarray(next_obs), dtype=DT)
        with torch.no_grad():
            qt = q_net_duel(self.target, S1, self.n_s, self.n_w)
            qo = q_net_duel(self.p, S1, self.n_s, self.n_w)
            if self.double_q:
                astar = torch.as_tensor(np.argmax(qo.numpy(), 1))                     # first maximum
                q1 = qt.gather(1, astar[:, None])[:, 0]
            else:
                astar, q1 = None, qt.max(1).values
            r = torch.as_tensor(np.asarray(rs), dtype=DT)
            d = torch.as_tensor(np.asarray(dones).astype(bool))
            return torch.where(d, r, r + self.gamma * q1), astar, qo, qt

    def loss_and_grads(self, obs, acts, next_obs, dones, rs):
        if not self.has_target:
            self.sync_target()
        P = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        S = torch.as_tensor(np.asarray(obs), dtype=DT)
        q0 = q_net_duel(P, S, self.n_s, self.n_w).gather(1, torch.as_tensor(np.asarray(acts), dtype=torch.long)[:, None])[:, 0]
        y, astar, qo, qt = self.targets(next_obs, dones, rs)
        self.last_y, self.last_q1_online, self.last_q1_target = y.numpy().copy(), qo.numpy().copy(), qt.numpy().copy()
        self.last_astar = None if astar is None else astar.numpy().astype(np.int32)
        w = torch.ones_like(y) if self.weights is None else torch.as_tensor(np.asarray(self.weights), dtype=DT)
        d = q0 - y
        self.last_delta = d.detach().numpy().copy()
        loss = (w * d ** 2).mean()
        loss.backward()
        return loss.item(), {k: v.grad.detach() for k, v in P.items()}


class DuelOracleIQL(PerOracleIQL):
    def __init__(self, agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, per=False, alpha=0.6, eps=0.01, target_update=0, double_q=False,
                 gamma=0.99, max_grad_norm=40.0, **kw):
        assert all('v_w' in p and 'v_b' in p for p in agent_params), 'a dueling oracle needs the value stream of every agent'
        assert not (double_q and not target_update)
        super().__init__(agent_params, n_wave_ls, n_w_ls, n_a_ls, n_env, alpha=alpha, eps=eps, target_update=target_update,
                         double_q=double_q, gamma=gamma, max_grad_norm=max_grad_norm, **kw)
        self.qs = [DuelOracleQ(p, nw, nt, gamma, max_grad_norm, target_update, double_q) for p, nw, nt in zip(agent_params, n_wave_ls, n_w_ls)]
        self.per = bool(per)

    def forward(self, obs):
        """obs [E, A, SMAX] -> list[A] of combined q [E, n_a] (float64)."""
        out = []
        for a, q in enumerate(self.qs):
            n = self.nw[a] + self.nt[a]
            with torch.no_grad():
                out.append(q_net_duel(q.p, torch.as_tensor(np.asarray(obs)[:, a, :n], dtype=DT), q.n_s, q.n_w).numpy())
        return out

    def minibatch_step(self, lr, beta=1.0, idx_given=None):
        if self.per:
            return super().minibatch_step(lr, beta=beta, idx_given=idx_given)
        for q in self.qs:
            q.weights = None
        return OracleIQL.minibatch_step(self, lr, idx_given=idx_given)        # Floyd's draw, every row weighs 1
