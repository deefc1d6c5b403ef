"""tests/env_harness.py on the host (no GPU, no library): a harness that compares nothing passes everything, and one copy decides for
every simulator test.  A stand-in handle wraps E OracleEnvs behind the part of VecTrafficEnv the harness uses and takes one planted
error (what, control step, instance); the walks must pass the clean stand-in and name step and instance of every planted error.

Shape: small_grid MA2C, E = 2, seeds 5 and 6, 10 control steps, uniform actions from RandomState(0): every instance holds at least 50
vehicles after step 9, 14 vehicles have arrived in instance 0 and the rewards are non-zero from step 3 on -- asserted below, so that
every planted error hits live data."""
import numpy as np
import pytest
import torch

from deeprl_signal_control_amd.scenario import build_small_grid
from tests import env_harness as H

E, SEEDS, STEPS = 2, (5, 6), 10
PLANTS = [('obs', 5, 1), ('reward', 5, 1), ('global_reward', 5, 1), ('done', 5, 1), ('arrived', 9, 0)] + [(k, 9, 1) for k in H.STATE_KEYS]


class StandIn:
    """E OracleEnvs as a handle on the CPU; plant = (what, control step, instance) changes one value the handle reports."""
    device = torch.device('cpu')

    def __init__(self, scn, plant=(None, -1, -1)):
        from oracle.env_oracle import OracleEnv
        self.scn, self.E, self.plant, self.t = scn, E, plant, -1
        self.orc = [OracleEnv(scn, seed=s) for s in SEEDS]

    def _hit(self, what, e=None):
        return self.plant[0] == what and self.plant[1] == self.t and (e is None or e == self.plant[2])

    def _obs(self, obs):
        out = np.zeros((self.E, self.scn.n_agent, self.scn.s_max), np.float32)
        for e, ob in enumerate(obs):
            for a, x in enumerate(ob):
                out[e, a, :len(x)] = x
        return out

    def reset(self):
        self.t = -1
        return torch.from_numpy(self._obs([o.reset() for o in self.orc]))

    def update_fingerprint(self, pol):
        for e, o in enumerate(self.orc):
            o.update_fingerprint([pol[e, a, :n].numpy() for a, n in enumerate(self.scn.n_a_ls)])

    def step(self, act):
        self.t += 1
        res = [o.step(list(act[e].numpy())) for e, o in enumerate(self.orc)]
        out = [self._obs([r[0] for r in res]), np.array([r[1] for r in res], np.float64), np.array([r[2] for r in res], np.uint8),
               np.array([r[3] for r in res], np.float64)]
        for i, what in enumerate(('obs', 'reward', 'done', 'global_reward')):
            if self._hit(what):
                at = (self.plant[2], 1, 0)[:out[i].ndim]
                out[i][at] = 1 - out[i][at] if what == 'done' else out[i][at] + 1
        return [torch.from_numpy(x) for x in out]

    def get_state(self, e):
        st = {k: v.copy() for k, v in self.orc[e].ms.snapshot().items()}
        for k in H.STATE_KEYS:
            if self._hit(k, e):
                l = int(np.argmax(st['n']))                      # an occupied lane
                st[k][(l,) if k == 'n' else (l, 0)] += 1
        return st

    def counters(self):
        tot = [o.ms.totals() for o in self.orc]
        arrived = np.array([x['arrived'] for x in tot])
        if self._hit('arrived'):
            arrived[self.plant[2]] += 1
        return arrived, np.array([x['teleported'] for x in tot])

    def mean_live_vehicles(self):
        return float(np.mean([o.ms.totals()['live'] for o in self.orc]))

    def close(self):
        pass


@pytest.fixture(scope='module')
def scn():
    return build_small_grid('ma2c')


def _walk(scn, env):
    from oracle.env_oracle import OracleEnv
    orc = [OracleEnv(scn, seed=s) for s in SEEDS]
    env.reset()
    obs = [o.reset() for o in orc]
    rng = np.random.RandomState(0)
    rewards = []
    H.follow(env, H.oracle_steps(scn, orc, obs, STEPS, lambda t, obs: (H.uniform_actions(scn, rng, E), None)), state_at=[STEPS - 1],
             counters=True, after=lambda t, out, res, orc: rewards.append(out[1].copy()))
    return orc, rewards


def test_clean_stand_in_passes_and_the_run_is_live(scn):
    env = StandIn(scn)
    orc, rewards = _walk(scn, env)
    tot = [o.ms.totals() for o in orc]
    print('live %s, arrived %s, reward rows that are all zero: %s' % ([x['live'] for x in tot], [x['arrived'] for x in tot],
                                                                      [t for t, r in enumerate(rewards) if not r.any()]))
    assert min(x['live'] for x in tot) >= 50 and tot[0]['arrived'] == 14
    assert all(r[e].any() for r in rewards[3:] for e in range(E))
    assert env.mean_live_vehicles() >= 50
    # the planted state entries lie on occupied lanes
    assert all(o.ms.snapshot()['n'].max() > 0 for o in orc)


@pytest.mark.parametrize('plant', PLANTS, ids=lambda p: p[0])
def test_a_planted_error_is_found_and_named(scn, plant):
    what, t, e = plant
    with pytest.raises(AssertionError) as ei:
        _walk(scn, StandIn(scn, plant))
    msg = str(ei.value)
    assert 't=%d' % t in msg and 'e=%d' % e in msg, msg
    assert ('state %s ' % what if what in H.STATE_KEYS else {'arrived': 'counters'}.get(what, what)) in msg, msg


def _two(scn, envs, **kw):
    for env in envs:
        env.reset()
    rng = np.random.RandomState(0)
    return H.lockstep(envs, STEPS, lambda t: (H.uniform_actions(scn, rng, E), H.agent_policies(scn, rng, E)), **kw)


def test_two_handles_walk(scn):
    first = _two(scn, [StandIn(scn), StandIn(scn)], state_of=range(E))
    assert len(first) == STEPS and first[-1][1].any()
    with pytest.raises(AssertionError, match='reward t=5'):
        _two(scn, [StandIn(scn), StandIn(scn, ('reward', 5, 1))])
    with pytest.raises(AssertionError, match='state v t=9 e=1'):
        _two(scn, [StandIn(scn), StandIn(scn, ('v', 9, 1))], state_of=range(E))
