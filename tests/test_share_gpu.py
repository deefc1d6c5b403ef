"""GPU tests of opt-in parameter sharing (INTEGRATION.md "Parameter sharing"; include/tsc.h tsc_model_set_sharing /
tsc_model_get_sharing / tsc_model_share_grads; csrc/tsc_model.hip share_reduce_kernel).

  1  the reduce kernel equals tests/test_share_host.py::share_mean bit for bit;
  2  a shared update against the float64 oracle, whose gradients are averaged over each class before its own apply_grads;
  3  members stay bit-identical over three updates (A2C, and PPO with an active clip), an agent alone in its class is untouched;
  4  nothing changes while the key is off;
  5  arming and the refusals;
  6  checkpoints and replicas.

Tolerances are the existing ones of tests/test_model_gpu.py::_update_vs_oracle and tests/test_ppo_gpu.py: raw gradients
|d| <= 2e-5 max|g| per tensor against the oracle, parameters atol 3e-5, norms rtol 2e-3, hidden units on a ReLU kink as _grad_err treats them.  Everything about the reduce itself and
about the members' equality is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.layouts import Layout
from tests.ppo_oracle import K3_REWARD_NORM, K3_SMALL, fill, rand_obs
from tests.test_ppo_gpu import _check_grads, _check_params, _dev, _make, _put_copy, _vec
from tests.test_share_host import share_mean

pytestmark = pytest.mark.gpu

# ---- layouts -----------------------------------------------------------------------------------------------------------------------
_BIG, _MID, _SML = (30, 6, 16, 5), (24, 6, 12, 5), (18, 6, 8, 5)      # large_grid's three shapes (MA2C; IA2C: without the fingerprint)
FIVE_CLASSES = [0, 1, 0, 1, 4]                                         # 2 + 2 + 1, members not next to each other


def five(agent):
    """Five large_grid-shaped agents in classes 2 + 2 + 1."""
    shapes = [_BIG, _MID, _BIG, _MID, _SML]
    if agent == 'ia2c':
        return Layout([(w, t, 0, a) for w, t, f, a in shapes], 36)
    return Layout(shapes, 52)


# name -> (agent kind, layout, the classes share_classes must find)
KERNEL_LAYOUTS = {
    'tiny4': ('ia2c', Layout([(3, 1, 0, 2)] * 2 + [(1, 1, 0, 2)] + [(3, 1, 0, 2)], 4), [0, 0, 2, 0]),   # smallest stride, a singleton in between
    'one_class5': ('ma2c', Layout([_MID] * 5, 52), [0] * 5),
    'solo': ('ia2c', Layout([(3, 1, 0, 2)], 4), [0]),
    'two_of_65': ('ia2c', Layout([(3, 1, 0, 2), (2, 1, 0, 3)] * 32 + [(3, 1, 0, 2)], 4), [0, 1] * 32 + [0]),
}


def _arbitrary(A, n, rng):
    """float32 [A, n]: mixed magnitudes over sixteen decades, and 1e30, -1e30, 1 and denormals sprinkled over a tenth of the entries;
    the first columns hold the cancelling and the denormal cases for certain, the LAST four the tail column of the grid."""
    g = (rng.standard_normal((A, n)) * 10.0 ** rng.randint(-8, 9, (A, n))).astype(np.float32)
    special = np.array([1e30, -1e30, 1.0, 1e-40, -1e-45, 1e-38, 0.0, -0.0], np.float32)
    pick = rng.rand(A, n) < 0.1
    g[pick] = special[rng.randint(0, len(special), int(pick.sum()))]
    g[:, 0] = 1e30
    g[0::2, 1], g[1::2, 1] = 1e30, -1e30
    g[:, 2] = 1e-45
    g[:, 3] = 1.0
    g[0::2, 4], g[1::2, 4] = 1e30, 1.0
    g[:, n - 4:] = (rng.standard_normal((A, 4)) * 1e3).astype(np.float32)
    return g


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1: the kernel, exactly --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', ['lstm', 'fc'])
@pytest.mark.parametrize('name', list(KERNEL_LAYOUTS))
def test_reduce_equals_the_float64_restatement_bit_for_bit(name, policy):
    agent, lay, classes = KERNEL_LAYOUTS[name]
    m = _vec(lay, agent, policy, 1, 2, 3, share_params=1)
    assert m.share == classes and m.get_sharing() == classes
    per_agent = 2 * m.stride
    assert per_agent % 4 == 0 and m.n_param == lay.n_agent * per_agent
    g = _arbitrary(lay.n_agent, per_agent, np.random.RandomState(len(name) + per_agent))
    want = share_mean(g, classes)
    if lay.n_agent > 1:
        assert (_bits(want) != _bits(g)).any()
    m.grad_tensor().copy_(_dev(g.ravel()))
    m.share_grads()
    got = m.grad_tensor().cpu().numpy().reshape(lay.n_agent, per_agent)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, '%d entries differ, first (agent, offset) %r: got %r, want %r, inputs %r' % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], g[[a for a, c in enumerate(classes) if c == classes[bad[0][0]]], bad[0][1]])
    m.share_grads()                                         # a second pass over equal members: the mean of k equal values
    again = m.grad_tensor().cpu().numpy().reshape(lay.n_agent, per_agent)
    np.testing.assert_array_equal(_bits(again), _bits(share_mean(want, classes)))
    m.set_sharing(None)                                     # disarmed: a no-op
    m.grad_tensor().copy_(_dev(g.ravel()))
    m.share_grads()
    np.testing.assert_array_equal(_bits(m.grad_tensor().cpu().numpy()), _bits(g.ravel()))
    m.close()


# ---- 2: update parity ----------------------------------------------------------------------------------------------------------------
def _class_mean(ograds, classes):
    """The oracle's float64 gradient dicts (list[2A], agent-major, pi then v) with every class member's replaced by the class mean."""
    out = [dict(g) for g in ograds]
    for c in set(classes):
        members = [a for a, x in enumerate(classes) if x == c]
        if len(members) < 2:
            continue
        for tower in (0, 1):
            for k in ograds[2 * members[0] + tower]:
                mean = sum(ograds[2 * a + tower][k] for a in members) / len(members)
                for a in members:
                    out[2 * a + tower][k] = mean
    return out


@pytest.mark.parametrize('agent,policy', [('ma2c', 'lstm'), ('ia2c', 'lstm'), ('ma2c', 'fc'), ('ia2c', 'fc')])
def test_shared_update_matches_the_oracle(agent, policy):
    """Two consecutive updates, E = 16, T = 8, on five agents in classes 2 + 2 + 1.  compute_grads leaves the raw per-agent gradients
    (sharing does not touch them): each within 2e-5 max|g| of the oracle's, in both rounds (on an MI355X: at most 9.8e-7).
    apply_grads: the oracle applies the class mean of its own float64 gradients; parameters within 3e-5, the reported norm is the
    class's for every member."""
    E, T = 16, 8
    lay = five(agent)
    _, m, o = _make(agent, policy, E, T, 5, layout=lay, share_params=1)
    assert m.share == FIVE_CLASSES and m.share_sizes() == [2, 2, 1] and m.algo == 'a2c'
    o.lam = 1.0                                             # the A2C update: n-step returns
    rng = np.random.RandomState(21)
    obs = done = None
    for it in range(2):
        obs, done = fill(lay, o, E, T, rng, m.cfg['reward_norm'], obs=obs, done=done, put=_put_copy(m))
        Rb = m.forward(_dev(obs), False, 'v').clone()
        m.compute_grads(Rb)
        ograds, ostats = o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=0, slack=False)
        worst = _check_grads(m, o, ograds, 2e-5, what='round %d' % it)
        raw = m.grad_tensor().cpu().numpy().reshape(lay.n_agent, -1)
        assert (_bits(raw[0]) != _bits(raw[2])).any()       # members of a class, different samples: different raw gradients
        stats = m.apply_grads(1.0, want_stats=True)
        shared = m.grad_tensor().cpu().numpy().reshape(lay.n_agent, -1)
        np.testing.assert_array_equal(_bits(shared), _bits(share_mean(raw, FIVE_CLASSES)))
        onorm = o.apply_grads(_class_mean(ograds, FIVE_CLASSES), m._cur_lr)
        print('%s %s round %d: worst raw |dg| / max|g| %.1e, norms %s' % (agent, policy, it, worst, np.round(stats[:, 3], 4)))
        np.testing.assert_allclose(stats[:, 1:3], ostats[:, 1:], rtol=2e-3, atol=1e-6)     # value / entropy loss (column 0 of the oracle is PPO's surrogate)
        np.testing.assert_allclose(stats[:, 3], onorm, rtol=2e-3)
        assert stats[0, 3] == stats[2, 3] and stats[1, 3] == stats[3, 3] and len(set(stats[[0, 1, 4], 3])) == 3
        _check_params(m, o, what='round %d' % it)
        p = m.get_flat().reshape(lay.n_agent, -1)
        np.testing.assert_array_equal(_bits(p[0]), _bits(p[2])); np.testing.assert_array_equal(_bits(p[1]), _bits(p[3]))
    m.close()


# ---- 3: the invariant ----------------------------------------------------------------------------------------------------------------
def _feed(lay, models, E, T, rng, reward_norm, obs=None, done=None):
    """One rollout of random transitions into every model (tests/ppo_oracle.py::fill without an oracle); every model stores the values of
    its OWN forward.  -> (next obs, carried done)"""
    obs = rand_obs(lay, E, rng) if obs is None else obs
    done = np.ones(E, np.uint8) if done is None else done
    for t in range(T):
        act = np.stack([rng.randint(0, n, E) for n in lay.n_a_ls], 1).astype(np.int32)
        rew = -rng.rand(E, lay.n_agent) * 3.0 * reward_norm
        dpost = (rng.rand(E) < 0.1).astype(np.uint8)
        for m in models:
            _, v, _ = m.forward_sample(_dev(obs), _dev(done))
            m.add_transition(_dev(obs), _dev(done), _dev(act), _dev(rew), v.clone(), _dev(dpost))
        obs, done = rand_obs(lay, E, rng), dpost
    return obs, done


def _members_identical(m, classes):
    for what in ('params', 'ms'):
        rows = m.get_flat(what).reshape(len(classes), -1)
        for a, c in enumerate(classes):
            np.testing.assert_array_equal(_bits(rows[a]), _bits(rows[c]), err_msg='%s of agents %d and %d' % (what, c, a))


@pytest.mark.parametrize('algo', ['a2c', 'ppo'])
def test_members_stay_bit_identical_and_a_singleton_is_untouched(algo):
    """Three updates -- three A2C rollouts, or one rollout's three PPO epochs with an active clip (the batch, seeds and learning rate of
    K3_SMALL[0]) -- on the 2 + 2 + 1 layout: parameters and RMSProp accumulators of the members are bit-identical after every update,
    and agent 4, alone in its class, ends bit-identical to the same agent of an unshared handle fed the same rollouts."""
    agent, policy, E, T, seed, rseed, lr = K3_SMALL[0]
    lay = five(agent)
    cfg = dict(reward_norm=K3_REWARD_NORM, lr_init=lr, **(dict(algo='ppo', ppo_epochs=3) if algo == 'ppo' else {}))
    ms_, mu = _vec(lay, agent, policy, E, T, seed, share_params=1, **cfg), _vec(lay, agent, policy, E, T, seed, **cfg)
    ms_.reset(); mu.reset()
    p0 = ms_.get_flat().reshape(5, -1)
    np.testing.assert_array_equal(_bits(p0[[0, 1, 4]]), _bits(mu.get_flat().reshape(5, -1)[[0, 1, 4]]))    # the lowest members' draws
    _members_identical(ms_, FIVE_CLASSES)
    rng = np.random.RandomState(rseed)
    obs = done = None
    for roll in range(1 if algo == 'ppo' else 3):
        obs, done = _feed(lay, [ms_, mu], E, T, rng, K3_REWARD_NORM, obs, done)
        for m in (ms_, mu):
            Rb = m.forward(_dev(obs), False, 'v').clone()
            for k in range(m.n_epoch):
                m.compute_grads(Rb, k)
                m.apply_grads(1.0, epoch=k)
                if m is ms_:
                    _members_identical(m, FIVE_CLASSES)
    if algo == 'ppo':
        clipped = ms_.ppo_stats()[:, 0]
        print('clipped share at the last epoch:', np.round(clipped, 3))
        assert clipped.max() > 0
    for what in ('params', 'ms'):
        s, u = ms_.get_flat(what).reshape(5, -1), mu.get_flat(what).reshape(5, -1)
        np.testing.assert_array_equal(_bits(s[4]), _bits(u[4]))
        assert (_bits(s[0]) != _bits(u[0])).any() and (_bits(s[2]) != _bits(u[2])).any()
    assert (_bits(ms_.get_flat().reshape(5, -1)[0]) != _bits(p0[0])).any()
    ms_.close(); mu.close()


# ---- 4: neutral when off -------------------------------------------------------------------------------------------------------------
# launches per kernel id of ONE default update, cached-activation path (restated from tests/test_ppo_gpu.py)
A2C_UPDATE_LSTM = dict(returns=1, head_bwd=1, dwo_gemm=1, lstm_bwd=1, transpose_wx=1, dwx_gemm=1, dwh_gemm=1, dx1_gemm=1, dw1_gemm=1,
                       grad_norm=1, rmsprop=1)
A2C_UPDATE_FC = dict(returns=1, head_bwd=1, dwo_gemm=1, transpose_wx=1, dx1_gemm=1, dw1_gemm=1, grad_norm=1, rmsprop=1)


@pytest.mark.parametrize('policy,want', [('lstm', A2C_UPDATE_LSTM), ('fc', A2C_UPDATE_FC)])
def test_off_is_the_update_it_was(policy, want):
    """A never-armed handle, one armed with every agent in its own class, and one armed by the key, then disarmed and re-seeded, give
    bit-identical parameters and accumulators after an update; the default update's launch counts per kernel id are the table's, and
    an armed update shows the same ids and counts (the reduce runs inside the gradient-norm scope: no new id)."""
    from deeprl_signal_control_amd import _lib
    E, T = 16, 8
    lay = five('ia2c')
    never = _vec(lay, 'ia2c', policy, E, T, 5)
    single = _vec(lay, 'ia2c', policy, E, T, 5)
    single.set_sharing(list(range(5)))
    was = _vec(lay, 'ia2c', policy, E, T, 5, share_params=1)
    assert was.share == FIVE_CLASSES
    was.set_sharing(None)
    was.init_params(5)                                      # set_params + the accumulator reset of a fresh handle
    assert never.share is None and was.share is None and single.share == [0, 1, 2, 3, 4]
    assert never.get_sharing() == was.get_sharing() == single.get_sharing() == [0, 1, 2, 3, 4]
    armed = _vec(lay, 'ia2c', policy, E, T, 5, share_params=1)
    models = [never, single, was, armed]
    for m in models:
        m.reset()
    np.testing.assert_array_equal(_bits(never.get_flat()), _bits(was.get_flat()))
    obs, _ = _feed(lay, models, E, T, np.random.RandomState(1), never.cfg['reward_norm'])
    counts = []
    for m in models:
        Rb = m.forward(_dev(obs), False, 'v').clone()
        torch.cuda.synchronize()
        _lib.profile(enable=1, reset=True)
        try:
            m.backward(Rb)
            torch.cuda.synchronize()
            counts.append({k: c for k, (_, c) in _lib.profile().items()})
        finally:
            _lib.profile(enable=False)
            _lib.profile(reset=True)
    assert counts[0] == want, counts[0]
    assert counts[1] == want and counts[2] == want and counts[3] == want, counts
    for what in ('params', 'ms'):
        ref = never.get_flat(what)
        np.testing.assert_array_equal(_bits(single.get_flat(what)), _bits(ref))
        np.testing.assert_array_equal(_bits(was.get_flat(what)), _bits(ref))
        assert (_bits(armed.get_flat(what)) != _bits(ref)).any()
    names = _lib.profile_names()
    assert names[-2:] == ['gae', 'head_bwd_ppo'] and not any('share' in n for n in names)
    for m in models:
        m.close()


# ---- 5: arming and refusals ----------------------------------------------------------------------------------------------------------
def test_arming_copies_the_lowest_member_and_bad_classes_are_refused():
    from deeprl_signal_control_amd import _lib
    assert _lib.lib().tsc_version() >= 123
    agent, lay, classes = KERNEL_LAYOUTS['tiny4']
    m = _vec(lay, agent, 'lstm', 1, 2, 3)
    A, vp = lay.n_agent, C.c_void_p
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3] and m.share_sizes() == [1] * 4
    p0 = m.get_flat().reshape(A, -1).copy()
    assert (_bits(p0[0]) != _bits(p0[1])).any() and (_bits(p0[0]) != _bits(p0[3])).any()
    ms0 = (1.0 + np.random.RandomState(0).rand(*p0.shape)).astype(np.float32)
    _lib.check(m._L.tsc_model_set_opt_state(m._h, ms0.ctypes.data_as(vp)))

    def refused(call, *words):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert all(w in str(ex.value) for w in words), str(ex.value)

    # refusals leave the handle as it was: disarmed, parameters untouched
    refused(lambda: m.set_sharing([0, 0, 0, 0]), 'agents 0 and 2', 'unequal', '(3, 1, 0, 2) vs (1, 1, 0, 2)')
    refused(lambda: m.set_sharing([0, 0, 2, 4]), 'agent(s) 3', 'id 4')
    refused(lambda: m.set_sharing([-1, 0, 2, 7]), 'agent(s) 0 (id -1), 3 (id 7)')
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3]
    np.testing.assert_array_equal(_bits(m.get_flat()), _bits(p0.ravel()))

    m.set_sharing(classes)
    assert m.share == classes and m.get_sharing() == classes and m.share_sizes() == [3, 1]
    for what, before in (('params', p0), ('ms', ms0)):
        now = m.get_flat(what).reshape(A, -1)
        for a in (0, 1, 3):
            np.testing.assert_array_equal(_bits(now[a]), _bits(before[0]))
        np.testing.assert_array_equal(_bits(now[2]), _bits(before[2]))
    # host buffers whose members differ are refused, parameters and accumulator alike, and nothing is uploaded
    shared = m.get_flat().reshape(A, -1).copy()
    bad = shared.copy()
    bad[3, 17] += 1.0
    refused(lambda: _lib.check(m._L.tsc_model_set_params(m._h, bad.ctypes.data_as(vp))), 'tsc_model_set_params', 'agents 0 and 3', 'offset 17')
    refused(lambda: _lib.check(m._L.tsc_model_set_opt_state(m._h, bad.ctypes.data_as(vp))), 'tsc_model_set_opt_state', 'agents 0 and 3')
    np.testing.assert_array_equal(_bits(m.get_flat()), _bits(shared.ravel()))
    ok = shared.copy()
    ok[2, 17] += 1.0                                        # the singleton may hold anything
    ok[[0, 1, 3], 5] = 0.25                                 # and the members anything they agree on
    _lib.check(m._L.tsc_model_set_params(m._h, ok.ctypes.data_as(vp)))
    np.testing.assert_array_equal(_bits(m.get_flat()), _bits(ok.ravel()))
    # ids need not be lowest member indices: what was given comes back, the lowest member is still the source
    m.set_sharing([3, 3, 1, 3])
    assert m.get_sharing() == [3, 3, 1, 3] and m.share_sizes() == [3, 1]
    refused(lambda: m.set_sharing([0, 0, 0, 0]), 'agents 0 and 2')
    assert m.get_sharing() == [3, 3, 1, 3]                  # a refused call leaves an armed handle armed as it was
    m.set_sharing(None)
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3]
    _lib.check(m._L.tsc_model_set_params(m._h, bad.ctypes.data_as(vp)))        # disarmed: any buffer again
    m.close()


# ---- 6: checkpoints and replicas -------------------------------------------------------------------------------------------------------
def test_checkpoints_between_shared_and_unshared_models(tmp_path):
    from deeprl_signal_control_amd import _lib
    lay = five('ma2c')
    mk = lambda seed, **cfg: _vec(lay, 'ma2c', 'lstm', 2, 4, seed, **cfg)      # noqa: E731
    a = mk(3, share_params=1)
    ms_a = a.get_flat('ms').reshape(5, -1).copy()
    ms_a[[0, 2]] = 1.5                                      # an accumulator that is not the initial one, equal inside the classes
    _lib.check(a._L.tsc_model_set_opt_state(a._h, ms_a.ctypes.data_as(C.c_void_p)))
    a.save(str(tmp_path / 'shared'), 7)
    z = np.load(str(tmp_path / 'shared' / 'checkpoint-7.npz'))
    assert [int(x) for x in z['share']] == FIVE_CLASSES
    b = mk(4, share_params=1)
    assert (_bits(a.get_flat()) != _bits(b.get_flat())).any()
    assert b.load(str(tmp_path / 'shared'))
    for what in ('params', 'ms'):
        np.testing.assert_array_equal(_bits(b.get_flat(what)), _bits(a.get_flat(what)))
    assert b.share == FIVE_CLASSES
    u = mk(4)                                               # a shared file into an unshared model: ordinary parameters
    assert u.load(str(tmp_path / 'shared')) and u.share is None
    np.testing.assert_array_equal(_bits(u.get_flat()), _bits(a.get_flat()))
    v = mk(6)                                               # an unshared model's members differ from the start
    v.save(str(tmp_path / 'plain'), 7)
    assert [int(x) for x in np.load(str(tmp_path / 'plain' / 'checkpoint-7.npz'))['share']] == [0, 1, 2, 3, 4]
    before = b.get_flat().copy()
    with pytest.raises(ValueError, match='does not fit this model.*agents 0 and 2'):
        b.load(str(tmp_path / 'plain'))
    np.testing.assert_array_equal(_bits(b.get_flat()), _bits(before))          # and nothing was uploaded
    assert u.load(str(tmp_path / 'plain'))
    # copy_from between armed handles, and the refusal of an unshared source
    b.copy_from(a)
    with pytest.raises(RuntimeError, match='agents 0 and 2'):
        b.copy_from(v)
    for m in (a, b, u, v):
        m.close()


def test_multibatch_trainer_keeps_shared_replicas_identical():
    """MultiBatchTrainer with share_params = 1 on large_grid (classes 12 + 9 + 4): both half-batches apply the same summed gradient and
    reduce it the same way, so parameters and RMSProp slots stay bit-identical across the replicas and inside every class over three
    rollouts (following test_multibatch_trainer_keeps_ppo_replicas_identical)."""
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_large_grid
    from deeprl_signal_control_amd.trainer import MultiBatchTrainer
    scn = build_large_grid('ma2c')
    E, T = 8, 6
    cfg = {'batch_size': T, 'reward_norm': 2000.0, 'share_params': 1, 'lr_init': 5e-3}
    envs = [VecTrafficEnv(scn, E, seed=30 + 100 * b) for b in range(2)]
    models = [VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, 5, cfg, seed=3, name='ma2c') for b in range(2)]
    models[1].sample_seed = 51
    assert models[0].share_sizes() == [12, 9, 4]
    p0 = models[0].get_flat().copy()
    tr = MultiBatchTrainer(envs, models)
    for _ in range(3):
        tr.run_iteration()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(models[0].get_flat()), _bits(models[1].get_flat()))
        np.testing.assert_array_equal(_bits(models[0].get_flat('ms')), _bits(models[1].get_flat('ms')))
        _members_identical(models[0], models[0].share)
    assert np.abs(models[0].get_flat() - p0).max() > 0
    for e in envs:
        e.close()
    for m in models:
        m.close()


def test_e1_adaptors_take_the_key():
    """IA2C / MA2C (E = 1) hand `share_params` through model_config like the PPO keys (a string, as configparser delivers it)."""
    from deeprl_signal_control_amd.agents import IA2C, MA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    for cls, agent in ((MA2C, 'ma2c'), (IA2C, 'ia2c')):
        scn = build_scenario('large_grid', agent)
        args = (scn.n_s_ls, scn.n_a_ls, scn.n_w_ls) + ((scn.n_f_ls,) if agent == 'ma2c' else ())
        a = cls(*args, 1000, dict(batch_size=4, share_params='1'), seed=2)
        assert a.vec.share_sizes() == [12, 9, 4]
        _members_identical(a.vec, a.vec.share)
        a.vec.close()
        with pytest.raises(ValueError, match='share_params'):
            cls(*args, 1000, dict(batch_size=4, share_params='2'), seed=2)
