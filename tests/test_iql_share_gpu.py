"""GPU tests of opt-in parameter sharing for the Q-learners (INTEGRATION.md "Parameter sharing"; include/tsc.h tsc_iql_set_sharing /
tsc_iql_get_sharing / tsc_iql_share_grads; csrc/tsc_share.h share_reduce_kernel, launched from tsc_iql_apply_grads).

  1  the reduce equals tests/test_share_host.py::share_mean bit for bit on the [A][stride] gradient buffer;
  2  two shared minibatch steps on the caller's draw against tests/iql_share_oracle.py's SharedOracleIQL, on the fused, the grouped and
     the IQL-LR route, the fused one again with every option armed; large_grid's 25 agents (12 + 9 + 4) for one step;
  3  members stay bit-identical over three steps, an agent alone in its class is untouched;
  4  two handles that stand in for two ranks stay identical;
  5  nothing changes while the key is off;
  6  arming and the refusals;
  7  checkpoints.

Tolerances are those of tests/iql_harness.py and no others: gradients |d| <= 2e-5 max|g| per tensor (hidden units on a ReLU kink
excepted as compare_grads does; a class mean carries the kink of any member), loss and clip norm rtol 1e-4, parameter steps by
tests/layouts.py::adam_step_bound (second moments preloaded with 1, as that bound requires).  Everything about the reduce and about
the members' equality is exact.  The layouts, seeds and data are tests/iql_share_oracle.py's; tests/test_iql_share_host.py states the
conditions the seeds meet.  The dueling head takes at most 7 actions per agent (tsc_iql_set_dueling), so the dueling cases run on the
eight agents of the 12-agent layout that have them (q160x8, classes [0..3, 0..3])."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import iql_harness as H
from tests import layouts as LY
from tests.iql_share_oracle import (ALL_ARMED, GRID_CASE, PARITY, PARITY_LR, PARITY_STEPS, PER_BETA, case_data, case_params, members_of,
                                    preload_second_moments, shared_oracle_for, spec_of)
from tests.test_share_gpu import _arbitrary, _bits
from tests.test_share_host import share_mean

pytestmark = pytest.mark.gpu
VP = C.c_void_p


def _handle(name, cfg, seed, E, cap, monkeypatch, share=1):
    spec = spec_of(name)
    monkeypatch.delenv('TSC_IQL_FUSED', raising=False)
    kw = dict(spec['cfg'], **cfg)
    if share:
        kw['share_params'] = 1
    lay, m = H.model(spec['layout'], 'iql', spec['model_type'], E, seed=seed, buffer_size=cap, reward_norm=LY.IQL_REWARD_NORM, **kw)
    assert bool(m.fused) == spec['fused'], name
    assert m.share == (spec['classes'] if share else None)
    return lay, m


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _feed(models, trans, oracle=None):
    for tr in trans:
        for m in models:
            m.add_transition(*[_dev(x) for x in tr])
        if oracle is not None:
            oracle.add_transition(*tr)


def _set_opt(m, m1, m2, t):
    m1, m2 = np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)
    H.check(m._L.tsc_iql_set_opt_state(m._h, m1.ctypes.data_as(VP), m2.ctypes.data_as(VP), t))


def _state(m):
    """name -> flat float32 array: parameters, both Adam moments and, on a handle with a target network, the frozen copy."""
    m1, m2, _ = m.get_opt_state()
    out = {'params': m.get_flat(), 'adam_m': m1, 'adam_v': m2}
    if m.target_update:
        out['target'] = m.get_target_flat()
    return out


def _members_identical(m, classes):
    A = len(classes)
    low = {}
    for what, flat in _state(m).items():
        rows = flat.reshape(A, -1)
        for a, c in enumerate(classes):
            np.testing.assert_array_equal(_bits(rows[a]), _bits(rows[low.setdefault(c, a)]), err_msg='%s of agents %d and %d' % (what, low[c], a))


# ---- 1: the reduce, exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,cfg', [('lr4', {}), ('q160x12', {}), ('solo', {}), ('lr65', {}), ('q160x8', dict(dueling=1))],
                         ids=['a_lr4', 'b_q160x12', 'c_solo', 'd_lr65', 'e_dueling'])
def test_reduce_equals_the_float64_restatement_bit_for_bit(name, cfg, monkeypatch):
    lay, m = _handle(name, cfg, 3, 1, 20, monkeypatch)
    classes, A = spec_of(name)['classes'], lay.n_agent
    assert m.get_sharing() == classes
    stride = m.layout.stride
    assert stride % 4 == 0 and m.n_param == A * stride
    if name == 'lr4':
        assert stride == 40                                 # 10 four-float columns: one partial workgroup
    if name.startswith('q160'):
        assert stride // 4 > 2 * 256 and (stride // 4) % 256 != 0          # several workgroups per class, the last one ragged
    g = _arbitrary(A, stride, np.random.RandomState(len(name) + stride))
    want = share_mean(g, classes)
    if A > 1:
        assert (_bits(want) != _bits(g)).any()
    m.grad_tensor().copy_(_dev(g.ravel()))
    m.share_grads()
    got = m.grad_tensor().cpu().numpy().reshape(A, stride)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, '%d entries differ, first (agent, offset) %r: got %r, want %r' % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    m.share_grads()                                         # a second pass over equal members: the mean of k equal values
    again = m.grad_tensor().cpu().numpy().reshape(A, stride)
    np.testing.assert_array_equal(_bits(again), _bits(share_mean(want, classes)))
    m.set_sharing(None)                                     # disarmed: a no-op
    assert m.share is None and m.get_sharing() == list(range(A))
    m.grad_tensor().copy_(_dev(g.ravel()))
    m.share_grads()
    np.testing.assert_array_equal(_bits(m.grad_tensor().cpu().numpy()), _bits(g.ravel()))
    m.close()


# ---- 2: update parity ------------------------------------------------------------------------------------------------------------------
def _kink_masks(m, o, idx, params_before, rows_before, classes):
    """Per agent (first-layer columns, any second-layer unit) on a ReLU kink as iql_harness.compare_grads finds them, joined over the
    agent's class: the class mean carries the kink of any member."""
    own = []
    for a in range(m.n_agent):
        q = o.qs[a]
        saved, q.p = q.p, params_before[a]
        own.append(H.kinks(o, [rows_before[a][e][s][0] for e in range(m.E) for s in idx[e, a]], a))
        q.p = saved
    out = []
    for a in range(m.n_agent):
        mates = [b for b in range(m.n_agent) if classes[b] == classes[a]]
        cols = None if own[a][0] is None else np.logical_or.reduce([own[b][0] for b in mates])
        out.append((cols, any(own[b][1] for b in mates)))
    return out


def _compare_mean(m, g, og, masks, what):
    """compare_grads's comparison -- |d| <= 2e-5 max|g| per tensor -- of the class-mean gradients, under the class's kinks."""
    for a in range(m.n_agent):
        cols, deep = masks[a]
        for k, ref in og[a].items():
            if deep and k not in ('q_w', 'q_b', 'v_w', 'v_b'):
                continue
            scale, err = max(np.abs(ref).max(), 1e-9), np.abs(g[a][k] - ref)
            if cols is not None and k.startswith(('fcw', 'fct')) and cols.any():
                sel = cols[:m.layout.n_fc0] if k.startswith('fcw') else cols[m.layout.n_fc0:]
                err = err[..., ~sel] if err.ndim == 2 else err[~sel]
            assert err.size == 0 or err.max() <= 2e-5 * scale, '%s agent %d %s: %.2e' % (what, a, k, err.max() / scale)


def _parity(name, cfg, seed, E, cap, steps, monkeypatch):
    lay, m = _handle(name, cfg, seed, E, cap, monkeypatch)
    classes, A, lr = spec_of(name)['classes'], lay.n_agent, PARITY_LR
    params = case_params(name, cfg, seed)
    if not cfg.get('dueling'):          # VecIQL's own initialisation is the rule case_params restates: the class's lowest member's draw
        np.testing.assert_array_equal(_bits(m.get_flat()), _bits(m.layout.pack(params)))
    m.set_agent_params(params)
    if m.target_update:                 # a frozen copy that disagrees, equal inside every class
        m.set_target_flat(m.layout.pack(case_params(name, cfg, seed, target=True)))
    _set_opt(m, np.zeros(m.n_param), np.ones(m.n_param), 0)
    _members_identical(m, classes)
    o = shared_oracle_for(m)
    assert o.classes == classes
    if m.target_update:
        o.set_target_params(m.layout.unpack(m.get_target_flat()))
    preload_second_moments(o)
    trans, idx, prio = case_data(name, seed, E, cap, steps)
    _feed([m], trans, o)
    if m.prioritized_replay:
        m.set_priorities(prio, np.maximum(m.get_priorities()[1], prio.max(2)))
        o.prio[:], o.qmax[:] = m.get_priorities()
        H.set_beta(m, PER_BETA)
    for step in range(steps):
        before = m.layout.unpack(m.get_flat())
        tgt_before = m.get_target_flat() if m.target_update else None
        d_idx = _dev(idx[step])
        H.check(m._L.tsc_iql_compute_grads_at(m._h, VP(d_idx.data_ptr())))
        m.update_step += 1
        raw = m.grad_tensor().cpu().numpy().copy()
        m.share_grads()
        shared = m.grad_tensor().cpu().numpy().copy()
        np.testing.assert_array_equal(_bits(shared.reshape(A, -1)), _bits(share_mean(raw.reshape(A, -1), classes)))
        stats = np.zeros((A, 2))
        H.check(m._L.tsc_iql_apply_grads(m._h, lr, 1.0, stats.ctypes.data_as(VP)))
        np.testing.assert_array_equal(_bits(m.grad_tensor().cpu().numpy()), _bits(shared))     # apply's own reduce met equal members
        obefore = [{k: v.numpy().copy() for k, v in q.p.items()} for q in o.qs]
        params_before, rows_before = H.snapshot(o)
        losses, norms, og = o.minibatch_step(lr, beta=PER_BETA, idx_given=idx[step])
        what = '%s step %d' % (name, step)
        # raw gradients, per member, before the reduce
        kinked = H.compare_grads(m, o, m.layout.unpack(raw), og, idx[step], params_before, rows_before, what + ' raw')
        masks = _kink_masks(m, o, idx[step], params_before, rows_before, classes)
        # the class-mean gradients behind share_grads
        _compare_mean(m, m.layout.unpack(shared), o.last_mean, masks, what + ' class mean')
        print('%s: agents on a ReLU kink %s; norms %s' % (what, sorted(kinked), np.round(stats[:, 1], 3)))
        np.testing.assert_allclose(stats[:, 0], losses, rtol=1e-4, atol=1e-9)       # the member's own loss
        np.testing.assert_allclose(stats[:, 1], norms, rtol=1e-4)                   # the class's norm
        for members in members_of(classes).values():
            assert len(set(stats[members, 1])) == 1 and len(set(stats[members, 0])) == len(members)
            rows = raw.reshape(A, -1)
            assert all((_bits(rows[a]) != _bits(rows[members[0]])).any() for a in members[1:])     # own rings, own gradients
        # parameters: Adam's step on the class mean
        after, oafter = m.layout.unpack(m.get_flat()), [{k: v.numpy().copy() for k, v in q.p.items()} for q in o.qs]
        worst = 0.0
        for a in range(A):
            if masks[a][1] or (masks[a][0] is not None and masks[a][0].any()):
                continue
            for k in before[a]:
                d_hip, d_orc = after[a][k].astype(np.float64) - before[a][k], oafter[a][k] - obefore[a][k]
                bound = LY.adam_step_bound(d_orc, before[a][k])
                worst = max(worst, float(np.abs(d_hip - d_orc).max()) / bound)
                assert np.abs(d_hip - d_orc).max() <= bound, '%s agent %d %s: %.2e > %.2e' % (what, a, k, np.abs(d_hip - d_orc).max(), bound)
        assert np.abs(m.get_flat() - m.layout.pack(before)).max() > 0
        print('%s: worst parameter-step error %.2f of its bound' % (what, worst))
        _members_identical(m, classes)
        if m.target_update:             # the frozen copy follows after every target_update-th Adam step, and only then
            want = m.get_flat() if (step + 1) % m.target_update == 0 else tgt_before
            np.testing.assert_array_equal(_bits(m.get_target_flat()), _bits(want))
        assert H.sync_oracle(m, o) == step + 1
        if m.prioritized_replay:
            o.prio[:], o.qmax[:] = m.get_priorities()
    m.close()


@pytest.mark.parametrize('name,cfg,seed', PARITY, ids=[n + ('_armed' if c else '') for n, c, _ in PARITY])
def test_shared_update_matches_the_shared_oracle(name, cfg, seed, monkeypatch):
    assert not cfg or cfg == ALL_ARMED
    _parity(name, cfg, seed, LY.IQL_E, LY.IQL_CAP, PARITY_STEPS, monkeypatch)


def test_shared_update_on_large_grid(monkeypatch):
    E, cap, seed = GRID_CASE
    assert sorted((spec_of('large_grid')['classes'].count(c) for c in set(spec_of('large_grid')['classes'])), reverse=True) == [12, 9, 4]
    _parity('large_grid', {}, seed, E, cap, 1, monkeypatch)


# ---- 3: the invariant ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['q160x5', 'q_small', 'lr4'])
def test_members_stay_bit_identical_and_a_singleton_is_untouched(name, monkeypatch):
    """Three minibatch steps of the library's own draw with target_update = 2: parameters, both Adam moments and the frozen copy of the
    members are bit-identical after every step; an agent alone in its class ends bit-identical to the same agent of an unshared handle
    fed the same rings and draws, a member of a class of two or more does not."""
    E, cap, seed = LY.IQL_E, LY.IQL_CAP, 5
    lay, ms = _handle(name, dict(target_update=2), seed, E, cap, monkeypatch)
    _, mu = _handle(name, dict(target_update=2), seed, E, cap, monkeypatch, share=0)
    classes, A = spec_of(name)['classes'], lay.n_agent
    singles = [a for a, c in enumerate(classes) if classes.count(c) == 1]
    shared = [a for a, c in enumerate(classes) if classes.count(c) > 1]
    assert singles and shared and ms.replay_seed == mu.replay_seed
    lows = sorted(set(min(a for a, c in enumerate(classes) if c == cc) for cc in set(classes)))
    p_s, p_u = ms.get_flat().reshape(A, -1), mu.get_flat().reshape(A, -1)
    np.testing.assert_array_equal(_bits(p_s[lows]), _bits(p_u[lows]))             # the lowest members' draws
    _members_identical(ms, classes)
    _feed([ms, mu], case_data(name, seed, E, cap)[0])
    for step in range(3):
        for m in (ms, mu):
            stats = m.minibatch_step(1e-3, want_stats=True)
            if m is ms:
                _members_identical(m, classes)
                for members in members_of(classes).values():
                    assert len(set(stats[members, 1])) == 1
        np.testing.assert_array_equal(H.batch(ms), H.batch(mu))
        same = (_bits(ms.get_target_flat()) == _bits(ms.get_flat())).all()
        assert same == (step == 1)                                                # theta- <- theta behind the second step only
    assert ms.get_opt_state()[2] == 3
    s, u = _state(ms), _state(mu)
    for what in s:
        rs, ru = s[what].reshape(A, -1), u[what].reshape(A, -1)
        for a in singles:
            np.testing.assert_array_equal(_bits(rs[a]), _bits(ru[a]), err_msg='%s of agent %d' % (what, a))
        for a in shared:
            assert (_bits(rs[a]) != _bits(ru[a])).any(), (what, a)
    ms.close(); mu.close()


# ---- 4: ranks --------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_identical(monkeypatch):
    """Two handles stand in for two ranks: own rings, the gradient buffers summed on the device and written to both (the all-reduce),
    apply_grads with grad_scale = 0.5.  The mean sits in apply, behind the sum: members and handles stay bit-identical."""
    name, E, cap, seed = 'q160x12', LY.IQL_E, LY.IQL_CAP, 5
    ranks = [_handle(name, dict(target_update=2), seed, E, cap, monkeypatch)[1] for _ in range(2)]
    classes = spec_of(name)['classes']
    for r, m in enumerate(ranks):
        _feed([m], case_data(name, seed + r, E, cap)[0])
    p0 = ranks[0].get_flat().copy()
    for step in range(3):
        for m in ranks:
            H.check(m._L.tsc_iql_compute_grads(m._h, m.replay_seed, m.update_step))
            m.update_step += 1
        g0, g1 = ranks[0].grad_tensor(), ranks[1].grad_tensor()
        assert not torch.equal(g0, g1)
        total = g0 + g1
        g0.copy_(total); g1.copy_(total)
        stats = []
        for m in ranks:
            stats.append(np.zeros((m.n_agent, 2)))
            H.check(m._L.tsc_iql_apply_grads(m._h, 1e-3, 0.5, stats[-1].ctypes.data_as(VP)))
        np.testing.assert_array_equal(stats[0][:, 1], stats[1][:, 1])
        s0, s1 = _state(ranks[0]), _state(ranks[1])
        for what in s0:
            np.testing.assert_array_equal(_bits(s0[what]), _bits(s1[what]), err_msg=what)
        for m in ranks:
            _members_identical(m, classes)
    assert np.abs(ranks[0].get_flat() - p0).max() > 0
    for m in ranks:
        m.close()


# ---- 5: off means off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['q160x5', 'q_small'])
def test_off_is_the_step_it_was(name, monkeypatch):
    """share_params = 0, a handle armed by the key and disarmed (and re-seeded) before the first step, a handle armed with every agent in
    its own class and a never-armed handle: bit-identical parameters, Adam moments and priorities over two steps of prioritized replay,
    and the same launches under every profile id of iql_harness.KERNELS.  (An armed handle does differ.)"""
    from deeprl_signal_control_amd import _lib
    E, cap, seed = LY.IQL_E, LY.IQL_CAP, 5
    cfg = dict(prioritized_replay=1)
    lay, never = _handle(name, cfg, seed, E, cap, monkeypatch, share=0)
    _, key0 = _handle(name, dict(cfg, share_params=0), seed, E, cap, monkeypatch, share=0)
    _, was = _handle(name, cfg, seed, E, cap, monkeypatch)
    _, single = _handle(name, cfg, seed, E, cap, monkeypatch, share=0)
    _, armed = _handle(name, cfg, seed, E, cap, monkeypatch)
    A = lay.n_agent
    was.set_sharing(None)
    was.init_params(seed)                                   # set_params + the zero moments of a fresh handle
    single.set_sharing(list(range(A)))
    assert never.share is None and key0.share is None and was.share is None and single.share == list(range(A))
    assert never.get_sharing() == key0.get_sharing() == was.get_sharing() == single.get_sharing() == list(range(A))
    models = [never, key0, was, single, armed]
    for m in models[1:4]:
        np.testing.assert_array_equal(_bits(m.get_flat()), _bits(never.get_flat()))
    _feed(models, case_data(name, seed, E, cap)[0])
    counts = []
    _lib.profile(enable=True)
    try:
        for m in models:
            _lib.profile(reset=True)
            for step in range(2):
                m.minibatch_step(1e-3)
            torch.cuda.synchronize()
            counts.append({k: H.launches(k) for k in H.KERNELS + ('iql_adam',)})
    finally:
        _lib.profile(enable=False)
        _lib.profile(reset=True)
    # (the fused learner counts under iql_grad, the grouped GEMMs under ids of their own)
    assert counts[0]['iql_per_sample'] > 0 and counts[0]['iql_per_update'] > 0 and counts[0]['iql_adam'] == 2, counts[0]
    assert (counts[0]['iql_grad'] > 0) == bool(never.fused), counts[0]
    assert all(c == counts[0] for c in counts[1:]), counts   # (armed too: the reduce runs inside the iql_adam scope, no id of its own)
    ref, ref_prio = _state(never), never.get_priorities()
    for m in models[1:4]:
        for what, flat in _state(m).items():
            np.testing.assert_array_equal(_bits(flat), _bits(ref[what]), err_msg=what)
        for got, want in zip(m.get_priorities(), ref_prio):
            np.testing.assert_array_equal(_bits(got), _bits(want))
    assert (_bits(armed.get_flat()) != _bits(ref['params'])).any()
    assert not any('share' in n for n in _lib.profile_names())
    for m in models:
        m.close()


# ---- 6: arming and refusals ------------------------------------------------------------------------------------------------------------
def _refused(call, *words):
    with pytest.raises(RuntimeError) as ex:
        call()
    assert all(w in str(ex.value) for w in words), str(ex.value)


def test_arming_copies_the_lowest_member_and_bad_classes_are_refused(monkeypatch):
    from deeprl_signal_control_amd import _lib
    assert _lib.lib().tsc_version() >= 124
    lay, m = _handle('lr4', dict(target_update=3), 3, 1, 20, monkeypatch, share=0)
    classes, A = spec_of('lr4')['classes'], lay.n_agent
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3] and m.share_sizes() == [1] * 4
    rng = np.random.RandomState(0)
    p0 = m.get_flat().reshape(A, -1).copy()
    m0, v0, t0 = [rng.rand(*p0.shape).astype(np.float32) + 0.5 for _ in range(3)]
    _set_opt(m, m0, v0, 7)
    m.set_target_flat(t0.ravel())
    assert (_bits(p0[0]) != _bits(p0[1])).any() and (_bits(p0[0]) != _bits(p0[3])).any()
    start = {'params': p0, 'adam_m': m0, 'adam_v': v0, 'target': t0}

    def unchanged(ref):
        for what, flat in _state(m).items():
            np.testing.assert_array_equal(_bits(flat), _bits(ref[what].ravel()), err_msg=what)

    # refusals leave the handle as it was: disarmed, nothing touched
    _refused(lambda: m.set_sharing([0, 0, 0, 0]), 'tsc_iql_set_sharing', 'agents 0 and 2', 'unequal (n_wave, n_wait, n_act)', '(3, 1, 2) vs (1, 1, 2)')
    _refused(lambda: m.set_sharing([0, 0, 2, 4]), 'agent(s) 3', 'id 4')
    _refused(lambda: m.set_sharing([-1, 0, 2, 7]), 'agent(s) 0 (id -1), 3 (id 7)')
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3]
    unchanged(start)

    m.set_sharing(classes)
    assert m.share == classes and m.get_sharing() == classes and m.share_sizes() == [3, 1] and m.get_opt_state()[2] == 7
    now = _state(m)
    for what, before in start.items():                      # parameters, both moments and the frozen copy: the lowest member's
        rows = now[what].reshape(A, -1)
        for a in (0, 1, 3):
            np.testing.assert_array_equal(_bits(rows[a]), _bits(before[0]), err_msg=what)
        np.testing.assert_array_equal(_bits(rows[2]), _bits(before[2]), err_msg=what)
    # host buffers whose members differ are refused by every setter, and nothing is uploaded
    held = {k: v.reshape(A, -1).copy() for k, v in now.items()}
    bad = held['params'].copy()
    bad[3, 17] += 1.0
    ok_m, ok_v = held['adam_m'], held['adam_v']
    _refused(lambda: H.check(m._L.tsc_iql_set_params(m._h, bad.ctypes.data_as(VP))), 'tsc_iql_set_params', 'agents 0 and 3', 'offset 17')
    _refused(lambda: _set_opt(m, bad, ok_v, 9), 'tsc_iql_set_opt_state', 'first moments', 'agents 0 and 3', 'offset 17')
    _refused(lambda: _set_opt(m, ok_m, bad, 9), 'tsc_iql_set_opt_state', 'second moments', 'agents 0 and 3')
    _refused(lambda: m.set_target_flat(bad.ravel()), 'tsc_iql_set_target_params', 'agents 0 and 3')
    bad1 = held['params'].copy()
    bad1[1, 0] -= 1.0
    _refused(lambda: H.check(m._L.tsc_iql_set_params(m._h, bad1.ctypes.data_as(VP))), 'agents 0 and 1', 'offset 0')      # the FIRST differing pair
    unchanged(held)
    assert m.get_opt_state()[2] == 7
    ok = held['params'].copy()
    ok[2, 17] += 1.0                                        # the singleton may hold anything
    ok[[0, 1, 3], 5] = 0.25                                 # and the members anything they agree on
    H.check(m._L.tsc_iql_set_params(m._h, ok.ctypes.data_as(VP)))
    np.testing.assert_array_equal(_bits(m.get_flat()), _bits(ok.ravel()))
    m.sync_target()                                         # copies theta: equal members by itself
    np.testing.assert_array_equal(_bits(m.get_target_flat()), _bits(ok.ravel()))
    # ids need not be lowest member indices: what was given comes back, the lowest member is still the source
    m.set_sharing([3, 3, 1, 3])
    assert m.get_sharing() == [3, 3, 1, 3] and m.share_sizes() == [3, 1]
    _refused(lambda: m.set_sharing([0, 0, 0, 0]), 'agents 0 and 2')
    assert m.get_sharing() == [3, 3, 1, 3]                  # a refused call leaves an armed handle armed as it was
    m.set_sharing(None)
    assert m.share is None and m.get_sharing() == [0, 1, 2, 3]
    np.testing.assert_array_equal(_bits(m.get_flat()), _bits(ok.ravel()))      # disarming leaves everything as it is
    H.check(m._L.tsc_iql_set_params(m._h, bad.ctypes.data_as(VP)))             # disarmed: any buffer again
    m.close()


def test_arming_order_does_not_matter(monkeypatch):
    """Sharing armed before or after tsc_iql_set_target / _set_dueling / _set_per / _set_return_steps: the same state, and the same state
    after a step on the same rings and draw."""
    name, E, cap, seed = 'q_small', LY.IQL_E, LY.IQL_CAP, 6
    classes = spec_of(name)['classes']
    lay, first = _handle(name, {}, seed, E, cap, monkeypatch, share=0)
    _, last = _handle(name, {}, seed, E, cap, monkeypatch, share=0)
    first.set_sharing(classes)
    for m in (first, last):
        H.set_target(m, 2, 1); H.set_dueling(m, 1); H.set_per(m, 1); H.set_steps(m, 3)
        m.target_update = 2             # (so that _state reads the frozen copy)
    last.set_sharing(classes)
    assert first.get_sharing() == last.get_sharing() == classes and H.get_dueling(first) == H.get_dueling(last) == 1
    trans, idx, _ = case_data(name, seed, E, cap)
    _feed([first, last], trans)
    for step in range(2):
        a, b = _state(first), _state(last)
        for what in a:
            np.testing.assert_array_equal(_bits(a[what]), _bits(b[what]), err_msg='%s before step %d' % (what, step))
        _members_identical(first, classes); _members_identical(last, classes)
        ga, sa = H.grads_at(first, _dev(idx[step]))
        gb, sb = H.grads_at(last, _dev(idx[step]))
        np.testing.assert_array_equal(_bits(ga), _bits(gb))
        np.testing.assert_array_equal(sa, sb)
    first.close(); last.close()


# ---- 7: checkpoints and the E = 1 adaptor ------------------------------------------------------------------------------------------------
def test_checkpoints_between_shared_and_unshared_models(tmp_path, monkeypatch):
    name, cfg = 'q_small', dict(target_update=2)
    classes = spec_of(name)['classes']
    mk = lambda seed, share=1: _handle(name, cfg, seed, 2, 20, monkeypatch, share=share)[1]      # noqa: E731
    path = lambda d: str(tmp_path / d)                                                          # noqa: E731
    a = mk(3)
    A = a.n_agent
    mom = np.random.RandomState(1).rand(2, A, a.layout.stride).astype(np.float32)
    mom[:, 3] = mom[:, 1]                                   # moments that are not the initial ones, equal inside the class (1, 3)
    _set_opt(a, mom[0], mom[1], 5)
    tgt = a.get_flat().reshape(A, -1) * np.float32(0.5)
    a.set_target_flat(tgt.ravel())
    a.save(path('shared'), 7)
    z = np.load(path('shared') + '/checkpoint-7.npz')
    assert [int(x) for x in z['share']] == classes
    b = mk(4)
    assert (_bits(a.get_flat()) != _bits(b.get_flat())).any()
    assert b.load(path('shared')) and b.share == classes
    sa, sb = _state(a), _state(b)
    for what in sa:
        np.testing.assert_array_equal(_bits(sb[what]), _bits(sa[what]), err_msg=what)
    assert b.get_opt_state()[2] == 5
    u = mk(4, share=0)                                      # a shared model's file into an unshared model: ordinary parameters
    assert u.load(path('shared')) and u.share is None
    np.testing.assert_array_equal(_bits(u.get_flat()), _bits(a.get_flat()))
    u.save(path('agree'), 1)                                # an unshared model writes no key; its members agree here
    assert 'share' not in np.load(path('agree') + '/checkpoint-1.npz').files
    c = mk(8)
    assert c.load(path('agree')) and c.share == classes
    np.testing.assert_array_equal(_bits(c.get_flat()), _bits(a.get_flat()))
    np.testing.assert_array_equal(_bits(c.get_target_flat()), _bits(a.get_target_flat()))
    # files whose members differ -- in the parameters, in a moment only, in the frozen copy only -- are refused, and nothing is uploaded
    v = mk(6, share=0)
    v.save(path('plain'), 7)
    assert 'share' not in np.load(path('plain') + '/checkpoint-7.npz').files
    odd = mom.copy()
    odd[1, 3, 11] += 1.0
    _set_opt(u, odd[0], odd[1], 5)
    u.save(path('moment'), 1)
    _set_opt(u, mom[0], mom[1], 5)
    tgt[3, 2] += 1.0
    u.set_target_flat(tgt.ravel())
    u.save(path('target'), 1)
    before = _state(b)
    for d, words in (('plain', 'the parameters of agents 1 and 3'), ('moment', 'the second Adam moments of agents 1 and 3'),
                     ('target', 'the target parameters of agents 1 and 3')):
        with pytest.raises(ValueError, match='does not fit this model.*' + words):
            b.load(path(d))
        for what, flat in _state(b).items():
            np.testing.assert_array_equal(_bits(flat), _bits(before[what]), err_msg=what)
        assert u.load(path(d))                              # the unshared model takes each of them
    for m in (a, b, c, u, v):
        m.close()


def test_e1_adaptor_takes_the_key():
    """IQL (E = 1) hands `share_params` through model_config (a string, as configparser delivers it), for both model types."""
    from deeprl_signal_control_amd.iql import IQL
    from deeprl_signal_control_amd.scenario import build_scenario
    for agent, mt in (('iqld', 'dqn'), ('iqll', 'lr')):
        scn = build_scenario('large_grid', agent)
        a = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20, share_params='1'), seed=2, model_type=mt)
        assert a.share_sizes() == a.vec.share_sizes() == [12, 9, 4] and a.share == a.vec.share
        _members_identical(a.vec, a.vec.share)
        a.vec.close()
        plain = IQL(scn.n_s_ls, scn.n_a_ls, scn.n_w_ls, 1000, dict(batch_size=20), seed=2, model_type=mt)
        assert plain.share is None and plain.share_sizes() == [1] * 25
        plain.vec.close()
