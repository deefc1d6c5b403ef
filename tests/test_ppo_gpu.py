"""GPU parity of the opt-in PPO update (include/tsc.h tsc_model_compute_grads_ppo / tsc_model_apply_grads_ex / tsc_model_ppo_stats;
csrc/tsc_model.hip head_bwd_kernel<true>, gae_kernel) against the float64 PPOOracle of tests/ppo_oracle.py, and of `algo = ppo` with
one epoch and lambda = 1 against the A2C update it must then be.

Tolerances are the ones tests/test_model_gpu.py uses for the A2C update: gradients |d| <= 2e-5 max|g| per tensor against the
oracle and between two kernel paths of one update, 10 x that once the parameters carry an earlier update's float32 rounding, 1e-4
at the benchmarked batch; parameters atol 3e-5; losses rtol 2e-3; hidden units on a ReLU kink as _grad_err treats them.  New here:
samples whose float64 ratio sits within relative 1e-4 of their clip bound may fall on either side in float32; the comparison
allows each such sample's own contribution to a gradient entry (PPOOracle.amb_slack) and their share in the clipped share."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.ppo_oracle import K3_REWARD_NORM, K3_SMALL, fill, k3_conditions, make_oracle

pytestmark = pytest.mark.gpu


def _vec(scn, agent, policy, E, T, seed, **cfg):
    from deeprl_signal_control_amd.agents import VecA2C
    mc = dict(batch_size=T)
    mc.update(cfg)
    a_max = int(scn.green_tab.shape[1]) if hasattr(scn, 'green_tab') else scn.a_max
    return VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, a_max, mc, device=0, seed=seed,
                  name=agent, policy=policy)


def _make(agent, policy, E, T, seed, sel=None, layout=None, regime=None, **cfg):
    """layout: a layout object (tests/layouts.py) in place of large_grid.  regime: a value regime of tests/layouts.py REGIMES, applied to
    the handle's parameters; the oracle is built from what the handle then returns."""
    from deeprl_signal_control_amd.scenario import build_scenario
    scn = build_scenario('large_grid', agent) if layout is None else layout
    m = _vec(scn, agent, policy, E, T, seed, **cfg)
    if regime is not None:
        from tests.layouts import apply_regime
        m.set_tower_params(apply_regime(m.get_tower_params(), regime, scn))
    o = make_oracle(scn, agent, policy, E, seed, clip_eps=m.ppo_clip, gae_lambda=m.gae_lambda, cfg=m.cfg, towers=m.get_tower_params(),
                    sel=sel)
    m.reset(); o.reset()
    return scn, m, o


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _put_copy(*models, use_cache=True):
    """fill()'s hook for the add_transition path: every model sees the same transition; the first one's forward supplies the
    stored values (models with equal parameters compute equal ones)."""
    def put(t, obs, done, act, rew, dpost):
        vs = None
        for m in models:
            if use_cache:
                _, v, _ = m.forward_sample(_dev(obs), _dev(done))
            else:
                _, v = m.forward(_dev(obs), _dev(done), 'pv')
            vs = v.clone() if vs is None else vs
            m.add_transition(_dev(obs), _dev(done), _dev(act), _dev(rew), vs, _dev(dpost))
        return vs.cpu().numpy()
    return put


def _put_slots(m):
    """fill()'s hook for the zero-copy path: the transition is written straight into the rollout slots (what VecTrainer does)."""
    sl = m.rollout_slots()
    first = [True]

    def put(t, obs, done, act, rew, dpost):
        if t > 0:
            sl['obs'][t].copy_(_dev(obs))                       # the env wrote it there after step t - 1
        elif first[0]:                                          # slot 0 of a LATER rollout is the library's carry: left as it is
            sl['obs'][0].copy_(_dev(obs)); sl['done'][0].copy_(_dev(done))
            first[0] = False
        m.forward_sample(sl['obs'][t], sl['done'][t], v_out=sl['value'][t], action_out=sl['action'][t])
        sl['action'][t].copy_(_dev(act)); sl['reward'][t].copy_(_dev(rew)); sl['done'][t + 1].copy_(_dev(dpost))
        m.commit_transition()
        return sl['value'][t].cpu().numpy()
    return put


def _after_slots(m, obs):
    """The observation after the window's last step belongs in slot n_step (the library carries it into slot 0)."""
    m.rollout_slots()['obs'][m.n_step].copy_(_dev(obs))


def _grads(m):
    return m.unpack(m.grad_tensor().cpu().numpy())


def _returns(m):
    from deeprl_signal_control_amd import _lib
    Rs = np.zeros((m.n_step, m.E, m.n_agent), np.float32); Advs = np.zeros_like(Rs)
    _lib.check(m._L.tsc_model_get_returns(m._h, Rs.ctypes.data_as(C.c_void_p), Advs.ctypes.data_as(C.c_void_p)))
    return Rs, Advs


def _check_grads(m, o, ograds, tol, sel=None, slack=False, what=''):
    from tests.test_model_gpu import _grad_err
    g = _grads(m)
    sel = list(range(m.n_agent)) if sel is None else sel
    worst = 0.0
    for i, a in enumerate(sel):
        for k2 in (0, 1):
            for k, og in ograds[2 * i + k2].items():
                got, ref = g[2 * a + k2][k], og.numpy()
                if slack:                      # ambiguous samples: each one's own contribution to the entry is allowed on top
                    s = o.amb_slack[2 * i + k2][k].numpy()
                    d = np.abs(got - ref)
                    got = np.where(d <= s, ref, ref + np.sign(got - ref) * (d - s))
                err = _grad_err(o, 2 * i + k2, k, got, ref)
                worst = max(worst, err)
                assert err <= tol, '%s agent %d tower %d %s: |dg| / max|g| = %.2e > %.1e' % (what, a, k2, k, err, tol)
    return worst


def _check_params(m, o, sel=None, what=''):
    p, op = m.get_tower_params(), o.tower_params()
    sel = list(range(m.n_agent)) if sel is None else sel
    for i, a in enumerate(sel):
        for k2 in (0, 1):
            for k in op[2 * i + k2]:
                np.testing.assert_allclose(p[2 * a + k2][k], op[2 * i + k2][k], atol=3e-5, err_msg='%s param agent=%d %s' % (what, a, k))


# ---- 4: K = 1, lambda = 1 is the A2C update --------------------------------------------------------------------------------------
@pytest.mark.parametrize('agent,policy', [('ma2c', 'lstm'), ('ia2c', 'lstm'), ('ma2c', 'fc'), ('ia2c', 'fc')])
def test_one_epoch_lambda_one_is_the_a2c_update(agent, policy):
    """The same rollout through `algo = a2c` and `algo = ppo` (ppo_epochs 1, gae_lambda 1): Rs / Advs bit-identical, gradients
    within 2e-5 max|g| of each other and each within 2e-5 of the float64 oracle, the same parameters afterwards."""
    E, T = 24, 8
    scn, ma, o = _make(agent, policy, E, T, 5)
    mp = _vec(scn, agent, policy, E, T, 5, algo='ppo', ppo_epochs=1, gae_lambda=1.0)
    mp.reset()
    assert (ma.algo, ma.n_epoch, mp.algo, mp.n_epoch) == ('a2c', 1, 'ppo', 1)
    np.testing.assert_array_equal(ma.get_flat(), mp.get_flat())
    o.lam = 1.0
    obs, _ = fill(scn, o, E, T, np.random.RandomState(21), ma.cfg['reward_norm'], put=_put_copy(ma, mp), done_at=(3,))
    Rb = ma.forward(_dev(obs), False, 'v').clone()
    ma.compute_grads(Rb); mp.compute_grads(Rb)
    ograds, ostats = o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=0)
    (Ra, Aa), (Rp, Ap) = _returns(ma), _returns(mp)
    np.testing.assert_array_equal(Ra, Rp); np.testing.assert_array_equal(Aa, Ap)
    np.testing.assert_array_equal(Rp, o.Rs); np.testing.assert_array_equal(Ap, o.Advs)
    ga, gp = ma.grad_tensor().cpu().numpy().reshape(ma.G, -1), mp.grad_tensor().cpu().numpy().reshape(mp.G, -1)
    for t, (ta, tp) in enumerate(zip(ma.unpack(ga), mp.unpack(gp))):
        for k in ta:
            scale = max(float(np.abs(ta[k]).max()), 1e-30)
            assert float(np.abs(ta[k] - tp[k]).max()) <= 2e-5 * scale, (t, k)
    np.testing.assert_array_equal(ga == 0, gp == 0)
    wa = _check_grads(ma, o, ograds, 2e-5, what='a2c')
    wp = _check_grads(mp, o, ograds, 2e-5, what='ppo')
    print('%s %s: worst |dg| / max|g| vs oracle: a2c %.1e, ppo %.1e' % (agent, policy, wa, wp))
    sa, sp = ma.apply_grads(1.0, want_stats=True), mp.apply_grads(1.0, want_stats=True)
    assert sa.shape == (scn.n_agent, 4) and sp.shape == (scn.n_agent, 6)
    np.testing.assert_allclose(sp[:, 1:4], sa[:, 1:4], rtol=1e-5)                 # value / entropy loss, gradient norm
    np.testing.assert_allclose(sp[:, :3], ostats, rtol=2e-3, atol=1e-6)           # column 0: the surrogate, -mean(A) at ratio 1
    assert np.all(sp[:, 4] == 0) and np.abs(sp[:, 5]).max() == 0                  # nothing clipped, zero KL at epoch 0
    o.apply_grads(ograds, ma._cur_lr)
    _check_params(ma, o, what='a2c'); _check_params(mp, o, what='ppo')
    np.testing.assert_allclose(ma.get_flat(), mp.get_flat(), rtol=0, atol=1e-6)
    assert ma.cur_t == 0 and mp.cur_t == 0
    ma.close(); mp.close()


# ---- 5: GAE ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam', [0.9, 0.95])
def test_gae_matches_oracle(lam):
    """gae_kernel against PPOOracle.gae (float64 on both sides) at the rtol / atol of test_returns_match_reference_buffer_on_gpu,
    with terminal steps in the middle (step 4: every instance) and at the end of the window, and random ones."""
    E, T = 33, 12
    scn, m, o = _make('ma2c', 'lstm', E, T, 2, algo='ppo', gae_lambda=lam)
    obs, _ = fill(scn, o, E, T, np.random.RandomState(6), m.cfg['reward_norm'], put=_put_copy(m), done_at=(4, T - 1))
    Rb = m.forward(_dev(obs), False, 'v').clone()
    m.compute_grads(Rb, 0)
    o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=0, slack=False)
    Rs, Advs = _returns(m)
    print('lambda %.2f: max |dRs| %.2e, max |dAdvs| %.2e' % (lam, np.abs(Rs - o.Rs).max(), np.abs(Advs - o.Advs).max()))
    np.testing.assert_allclose(Rs, o.Rs, rtol=1e-6)
    np.testing.assert_allclose(Advs, o.Advs, rtol=1e-5, atol=1e-6)
    _, A1 = o.gae(np.stack(o.buf['rs']), np.stack(o.buf['vs']), np.stack(o.buf['dones'])[:, :, None] * np.ones((1, 1, scn.n_agent)),
                  Rb.cpu().numpy(), o.gamma, 1.0)
    assert np.abs(Advs - A1).max() > 1e-2                                          # and it is not the n-step estimator
    m.close()


# ---- 6: K = 3 with the clip active -------------------------------------------------------------------------------------------------
def _k3(agent, policy, E, T, seed, rseed, lr, sel=None, tol0=2e-5, p_done=0.1, layout=None, **cfg):
    scn, m, o = _make(agent, policy, E, T, seed, sel=sel, layout=layout, algo='ppo', ppo_epochs=3, reward_norm=K3_REWARD_NORM, lr_init=lr, **cfg)
    obs, _ = fill(scn, o, E, T, np.random.RandomState(rseed), K3_REWARD_NORM, put=_put_copy(m), sel=sel, p_done=p_done)
    Rb = m.forward(_dev(obs), False, 'v').clone()
    Rb_o = Rb.cpu().numpy() if sel is None else Rb.cpu().numpy()[:, sel]
    ids = list(range(scn.n_agent)) if sel is None else list(sel)
    for k in range(3):
        ograds, ostats = o.compute_grads(Rb_o, 0.01, epoch=k)
        clip, amb = k3_conditions(o, k)                                             # on the oracle alone, before the comparison
        m.compute_grads(Rb, k)
        worst = _check_grads(m, o, ograds, tol0 if k == 0 else 10 * tol0, sel=sel, slack=True, what='epoch %d' % k)
        stats = m.apply_grads(1.0, want_stats=True, epoch=k)
        ps = stats[ids, 4:]
        np.testing.assert_array_equal(stats[:, 4:], m.ppo_stats())
        onorm = o.apply_grads(ograds, lr, end_of_rollout=(k == 2))
        print('%s %s E=%d T=%d epoch %d: clipped %.3f (gpu %.3f), ambiguous %.4f, kl %.4f (gpu %.4f), worst |dg| / max|g| %.1e'
              % (agent, policy, E, T, k, clip, ps[:, 0].mean(), amb, o.approx_kl.mean(), ps[:, 1].mean(), worst))
        np.testing.assert_allclose(ps[:, 0], o.clip_share, rtol=2e-3, atol=o.amb_share.max() + 1e-12)
        np.testing.assert_allclose(ps[:, 1], o.approx_kl, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[ids, 1:3], ostats[:, 1:], rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(stats[ids, 3], onorm, rtol=2e-3)
        _check_params(m, o, sel=sel, what='epoch %d' % k)
        assert m.cur_t == (0 if k == 2 else T)
    m.close()


@pytest.mark.parametrize('agent,policy,E,T,seed,rseed,lr', K3_SMALL)
def test_k3_epochs_match_oracle(agent, policy, E, T, seed, rseed, lr):
    """Three epochs over one rollout, the oracle stepped with the same epochs: gradients (2e-5 at epoch 0, 2e-4 afterwards, plus
    the ambiguous samples' own contributions), parameters after every epoch (3e-5), clipped share and approximate KL.
    Chosen on the CPU (tests/ppo_oracle.py K3_SMALL, pinned by tests/test_ppo_oracle.py): init seed 5, rollout seed 7, E = 16,
    T = 8, lr 5e-2 (LSTM) / 5e-3 (FC).  Clipped share of all samples at epochs 1 / 2 on the oracle alone: MA2C LSTM 21.1 % /
    26.0 %, IA2C LSTM 16.3 % / 23.6 %, MA2C FC 26.3 % / 41.2 %, IA2C FC 13.8 % / 28.7 %; ambiguous samples at most 0.09 %."""
    _k3(agent, policy, E, T, seed, rseed, lr)


def test_k3_epochs_match_oracle_at_the_benchmarked_batch():
    """The same at large_grid MA2C, E = 1024, T = 120 (122 880 samples per agent; epoch 0 through the rollout's activation cache,
    epochs 1 - 2 through the training-shape re-forward) on three sampled agents -- the first, the centre and the last --
    like test_update_benchmarked_batch_E1024_T120: 1e-4 max|g| at epoch 0, 10 x that once the parameters carry an update's
    float32 rounding (the rule of _update_vs_oracle at this n_step).  Chosen on the CPU: init seed 5, rollout seed 7, p_done 0.05,
    lr 2e-2; on the oracle alone the clipped share of the three agents is 9.3 % / 57.6 % / 32.0 % at epoch 1 (33.0 % of all
    samples) and 19.2 % / 38.0 % / 18.9 % at epoch 2 (25.4 %), ambiguous samples at most 0.058 % (71 of an agent's 122 880).
    The worst |dg| / max|g| observed on the GPU at epochs 1 - 2 is not recorded here: this test has not yet run on one (the test
    prints it per epoch); until it has, whether the 10 x slack is needed or merely allowed is open."""
    _k3('ma2c', 'lstm', 1024, 120, 5, 7, 2e-2, sel=[0, 12, 24], tol0=1e-4, p_done=0.05)


# ---- 7: end-of-rollout bookkeeping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('agent,policy,zero_copy', [('ma2c', 'lstm', True), ('ma2c', 'lstm', False), ('ia2c', 'fc', True)])
def test_bookkeeping_moves_after_the_last_epoch_only(agent, policy, zero_copy):
    """A K = 3 update (through VecA2C.backward) whose rollout ends on a terminal step, then a second rollout: its epoch-0 gradients
    match the oracle's.  state_bw, done[0] or obs[0] moved before the last epoch would corrupt epochs 1 - 2 of the first update
    (parameters off); never moved, the second rollout starts from the wrong LSTM state / done / observation."""
    E, T, lr = 16, 8, 2e-2
    scn, m, o = _make(agent, policy, E, T, 5, algo='ppo', ppo_epochs=3, lr_init=lr)
    rng = np.random.RandomState(13)
    put = _put_slots(m) if zero_copy else _put_copy(m)
    obs, done = fill(scn, o, E, T, rng, m.cfg['reward_norm'], put=put, done_at=(T - 1,))
    if zero_copy:
        _after_slots(m, obs)
    Rb = torch.zeros(E, scn.n_agent, device='cuda')                               # terminal: no bootstrap
    stats = m.backward(Rb, want_stats=True)
    assert stats.shape == (scn.n_agent, 6) and m.cur_t == 0
    for k in range(3):
        g, _ = o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=k, slack=False)
        o.apply_grads(g, lr, end_of_rollout=(k == 2))
    _check_params(m, o, what='after K = 3')
    if zero_copy:                                                                 # the library carried slot T into slot 0
        sl = m.rollout_slots()
        np.testing.assert_array_equal(sl['obs'][0].cpu().numpy(), obs)
        np.testing.assert_array_equal(sl['done'][0].cpu().numpy(), done)
    obs2, _ = fill(scn, o, E, T, rng, m.cfg['reward_norm'], obs=obs, done=done, put=put)
    if zero_copy:
        _after_slots(m, obs2)
    Rb = m.forward(_dev(obs2), False, 'v').clone()
    m.compute_grads(Rb, 0)
    ograds, _ = o.compute_grads(Rb.cpu().numpy(), 0.01, epoch=0)
    np.testing.assert_array_equal(_returns(m)[1], o.Advs)                         # lambda 0.95, float64 on both sides ...
    worst = _check_grads(m, o, ograds, 2e-4, what='second rollout')               # ... parameters carry three updates' rounding
    print('%s %s zero_copy=%s: second rollout worst |dg| / max|g| %.1e' % (agent, policy, zero_copy, worst))
    m.close()


def test_epoch_without_epoch_zero_is_an_error():
    """The library refuses an epoch k > 0 unless epoch 0 ran on the same rollout: at the start, after the rollout's last apply,
    and after anything that invalidates what epoch 0 left behind -- an A2C tsc_model_compute_grads (Rs / Advs), tsc_model_reset
    (the start state), tsc_model_set_params (logp_old).  Out-of-range clip_eps / gae_lambda are refused too."""
    from deeprl_signal_control_amd import _lib
    scn, m, o = _make('ia2c', 'lstm', 4, 4, 1, algo='ppo', ppo_epochs=2)
    obs, _ = fill(scn, o, 4, 4, np.random.RandomState(0), m.cfg['reward_norm'], put=_put_copy(m))
    Rb = m.forward(_dev(obs), False, 'v').clone()
    L, h, rp = m._L, m._h, C.c_void_p(Rb.data_ptr())
    ppo = lambda k: L.tsc_model_compute_grads_ppo(h, rp, 0.01, 0.2, 0.95, k)       # noqa: E731

    def refused(k):
        return ppo(k) != 0 and 'without epoch 0' in _lib.lib().tsc_last_error().decode()
    assert refused(1)
    assert ppo(0) == 0 and L.tsc_model_apply_grads_ex(h, 1e-4, 1.0, None, 0) == 0 and ppo(1) == 0
    assert L.tsc_model_apply_grads_ex(h, 1e-4, 1.0, None, 1) == 0 and refused(1)   # the last epoch closed the rollout
    for spoil in (lambda: L.tsc_model_compute_grads(h, rp, 0.01), lambda: L.tsc_model_reset(h),
                  lambda: m.set_tower_params(m.get_tower_params())):
        assert ppo(0) == 0 and L.tsc_model_apply_grads_ex(h, 1e-4, 1.0, None, 0) == 0
        spoil()
        assert refused(1)
    assert L.tsc_model_compute_grads_ppo(h, rp, 0.01, 0.0, 0.95, 0) != 0 and 'clip_eps' in _lib.lib().tsc_last_error().decode()
    assert L.tsc_model_compute_grads_ppo(h, rp, 0.01, 0.2, 1.5, 0) != 0 and 'gae_lambda' in _lib.lib().tsc_last_error().decode()
    assert _lib.lib().tsc_version() >= 111
    m.close()


def test_vec_a2c_counts_the_epochs_itself():
    """compute_grads / apply_grads without an epoch argument (the two-call pattern of tests/test_tworank_gpu.py) under K = 3: the
    object runs epochs 0, 1, 2 in turn, closes the rollout after the third pair and refuses a new transition before that."""
    scn, m, o = _make('ia2c', 'fc', 4, 4, 1, algo='ppo', ppo_epochs=3)
    put = _put_copy(m)
    obs, _ = fill(scn, o, 4, 4, np.random.RandomState(0), m.cfg['reward_norm'], put=put)
    Rb = m.forward(_dev(obs), False, 'v').clone()
    for k in range(3):
        with pytest.raises(AssertionError, match='is due'):
            m.compute_grads(Rb, (k + 1) % 3)
        m.compute_grads(Rb)
        with pytest.raises(AssertionError, match='twice'):
            m.compute_grads(Rb)
        st = m.apply_grads(1.0, want_stats=True)
        assert (st[:, 5] == 0).all() == (k == 0)                                   # epoch 0 alone sits on the rollout's policy
        assert m.cur_t == (0 if k == 2 else 4)
        if k < 2:
            with pytest.raises(AssertionError, match='updates left'):
                m.add_transition(_dev(obs), False, m.action, torch.zeros(4, scn.n_agent, dtype=torch.float64, device='cuda'), m.v, m._false)
    fill(scn, o, 4, 4, np.random.RandomState(1), m.cfg['reward_norm'], put=put)    # the next rollout is accepted
    m.close()


def test_e1_adaptors_take_the_ppo_keys():
    """IA2C / MA2C (E = 1, lists of per-agent arrays) with algo = ppo: backward() runs the K epochs and closes the rollout; two
    rollouts in a row, the parameters move at each."""
    from deeprl_signal_control_amd.agents import IA2C, MA2C
    from deeprl_signal_control_amd.scenario import build_scenario
    for cls, agent in ((MA2C, 'ma2c'), (IA2C, 'ia2c')):
        scn = build_scenario('large_grid', agent)
        cfg = dict(batch_size=4, algo='ppo', ppo_epochs='3', ppo_clip='0.1', gae_lambda='0.9', lr_init=1e-2)
        args = (scn.n_s_ls, scn.n_a_ls, scn.n_w_ls) + ((scn.n_f_ls,) if agent == 'ma2c' else ())
        a = cls(*args, 1000, cfg, seed=2)
        assert (a.vec.algo, a.vec.n_epoch, a.vec.ppo_clip, a.vec.gae_lambda) == ('ppo', 3, 0.1, 0.9)
        rng = np.random.RandomState(3)
        a.reset()
        done, p_prev = True, a.vec.get_flat().copy()
        for it in range(2):
            for t in range(4):
                ob = [rng.rand(n) * 2 for n in scn.n_s_ls]
                pi, v = a.forward(ob, done, 'pv')
                act = [int(rng.randint(0, n)) for n in scn.n_a_ls]
                a.add_transition(ob, act, list(-rng.rand(scn.n_agent) * 4000), v, False)
                done = False
            R = a.forward([rng.rand(n) * 2 for n in scn.n_s_ls], False, 'v')
            a.backward(R)
            p = a.vec.get_flat()
            assert a.vec.cur_t == 0 and np.isfinite(p).all() and np.abs(p - p_prev).max() > 0
            assert np.abs(a.vec.ppo_stats()[:, 1]).max() > 0                       # the last epoch ran off the rollout's policy
            p_prev = p.copy()
        a.vec.close()


# ---- 8: replicas -----------------------------------------------------------------------------------------------------------------------
def test_multibatch_trainer_keeps_ppo_replicas_identical():
    """MultiBatchTrainer with algo = ppo, K = 3: the half-batches exchange every epoch's gradient, so parameters and RMSProp slots
    stay bit-identical over three rollouts (following test_multibatch_trainer_keeps_replicas_identical)."""
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_large_grid
    from deeprl_signal_control_amd.trainer import MultiBatchTrainer
    scn = build_large_grid('ma2c')
    E, T = 8, 6
    cfg = {'batch_size': T, 'reward_norm': 2000.0, 'algo': 'ppo', 'ppo_epochs': 3, 'lr_init': 5e-3}
    envs = [VecTrafficEnv(scn, E, seed=30 + 100 * b) for b in range(2)]
    models = [VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, 5, cfg, seed=3, name='ma2c') for b in range(2)]
    models[1].sample_seed = 51
    p0 = models[0].get_flat().copy()
    tr = MultiBatchTrainer(envs, models)
    for _ in range(3):
        tr.run_iteration()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(models[0].get_flat(), models[1].get_flat())
        np.testing.assert_array_equal(models[0].get_flat('ms'), models[1].get_flat('ms'))
        assert models[0].cur_t == 0 and models[1].cur_t == 0
    assert np.abs(models[0].get_flat() - p0).max() > 0
    assert np.abs(models[0].ppo_stats()[:, 1]).max() > 0                           # the last epoch ran off the rollout's policy
    for e in envs:
        e.close()
    for m in models:
        m.close()


def _rank_worker(rank, world, port, out):
    from tests.test_tworank_gpu import SEED0
    from deeprl_signal_control_amd.agents import VecA2C
    from deeprl_signal_control_amd.env import VecTrafficEnv
    from deeprl_signal_control_amd.scenario import build_scenario
    from deeprl_signal_control_amd.trainer import VecTrainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    E = 16
    scn = build_scenario('large_grid', 'ma2c')
    env = VecTrafficEnv(scn, E, device=0, seed=SEED0 + rank * E, seed_stride=E * world)
    model = VecA2C(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, scn.n_f_ls, E, scn.s_max, int(scn.green_tab.shape[1]),
                   dict(batch_size=120, algo='ppo', ppo_epochs=3, lr_init=5e-3), device=0, seed=1 + 7 * rank, name='ma2c')
    tr = VecTrainer(env, model)
    for it in range(3):
        _, stats = tr.run_iteration(want_stats=True)
        np.save(os.path.join(out, 'p_%d_%d.npy' % (it, rank)), model.get_flat('params'))
        np.save(os.path.join(out, 'ms_%d_%d.npy' % (it, rank)), model.get_flat('ms'))
        np.save(os.path.join(out, 'st_%d_%d.npy' % (it, rank)), stats)
    torch.distributed.destroy_process_group()


def test_two_ranks_one_gpu_ppo(tmp_path):
    """Two processes on one GPU over gloo (tests/test_tworank_gpu.py), algo = ppo with K = 3: an all-reduce per epoch inside
    VecA2C.backward; parameters and RMSProp slots bit-identical across the ranks after each of three rollouts."""
    import torch.multiprocessing as mp
    world, port = 2, 29300 + os.getpid() % 300
    out = str(tmp_path)
    mp.spawn(_rank_worker, args=(world, port, out), nprocs=world, join=True)
    ld = lambda n: np.load(os.path.join(out, n))                                   # noqa: E731
    for it in range(3):
        np.testing.assert_array_equal(ld('p_%d_0.npy' % it), ld('p_%d_1.npy' % it))
        np.testing.assert_array_equal(ld('ms_%d_0.npy' % it), ld('ms_%d_1.npy' % it))
        assert ld('st_%d_0.npy' % it).shape == (25, 6)
    assert not np.array_equal(ld('p_0_0.npy'), ld('p_2_0.npy'))
    assert not np.array_equal(ld('st_0_0.npy'), ld('st_0_1.npy'))                  # each rank reports its own shard's losses


# ---- 9: the default is untouched ---------------------------------------------------------------------------------------------------
# launches per kernel id of ONE update, cached-activation path, as on the commit before this feature (csrc/tsc_model.hip
# tsc_model_compute_grads + tsc_model_apply_grads: every ProfScope of the fused LSTM / FC update paths, once each)
A2C_UPDATE_LSTM = dict(returns=1, head_bwd=1, dwo_gemm=1, lstm_bwd=1, transpose_wx=1, dwx_gemm=1, dwh_gemm=1, dx1_gemm=1, dw1_gemm=1,
                       grad_norm=1, rmsprop=1)
A2C_UPDATE_FC = dict(returns=1, head_bwd=1, dwo_gemm=1, transpose_wx=1, dx1_gemm=1, dw1_gemm=1, grad_norm=1, rmsprop=1)


@pytest.mark.parametrize('policy,want', [('lstm', A2C_UPDATE_LSTM), ('fc', A2C_UPDATE_FC)])
def test_default_update_launches_what_it_did(policy, want):
    """No PPO key: one update launches exactly the kernels it launched before; the new ids exist, come after every old one, and
    stay at zero.  With algo = ppo the head pass and the advantage scan are the new ids and nothing else changes.
    tsc_profile_read exposes a launch COUNT per kernel id, not the order of the launches: counts are what is compared, against
    the tables above (each id of the fused update path once, as read from the code before this feature)."""
    from deeprl_signal_control_amd import _lib
    names = _lib.profile_names()
    assert names[-2:] == ['gae', 'head_bwd_ppo'] and names.index('demand') == len(names) - 3
    E, T = 16, 8
    for algo_cfg, expect in (({}, want), (dict(algo='ppo', ppo_epochs=1), None)):
        scn, m, o = _make('ia2c', policy, E, T, 5, **algo_cfg)
        obs, _ = fill(scn, o, E, T, np.random.RandomState(1), m.cfg['reward_norm'], put=_put_copy(m))
        Rb = m.forward(_dev(obs), False, 'v').clone()
        torch.cuda.synchronize()
        _lib.profile(enable=1, reset=True)
        try:
            m.backward(Rb)
            torch.cuda.synchronize()
            got = {k: c for k, (_, c) in _lib.profile().items()}
        finally:
            _lib.profile(enable=False)
            _lib.profile(reset=True)
        if expect is None:
            expect = dict(want); del expect['returns'], expect['head_bwd']; expect.update(gae=1, head_bwd_ppo=1)
        assert got == expect, got
        m.close()


# ---- learning ------------------------------------------------------------------------------------------------------------------------
def test_ma2c_ppo_mean_step_reward_improves():
    """tests/test_learning_gpu.py's run and trend criteria (18 episodes, E = 1024, lr 5e-3) with algo = ppo, four epochs."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import learning_curve
    rows, _ = learning_curve.run(18, 1024, lr=5e-3, algo='ppo', ppo_epochs=4)
    r = np.array([x['avg_reward'] for x in rows])
    print('ppo learning curve:', np.round(r, 1))
    assert np.isfinite(r).all() and r[0] < -400
    assert r[-4:].mean() > r[:4].mean() + 4.0, r
    assert np.all(np.diff(r[6:]) > -3.0), r
