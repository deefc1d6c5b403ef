"""Host-side conditions of tests/test_regimes_gpu.py, on the oracles alone (no GPU, no library; nothing of a kernel is restated here).

The layouts of tests/layouts.py walk the learner's SHAPES and keep its VALUES where the initialisation puts them: every probability
between 0.06 and 0.6, every gradient norm below max_grad_norm.  The regimes of LY.REGIMES leave that corner on purpose -- the 1e-10 clamp
of log pi, exp underflow and exact zeros in the softmax, saturated gates, a per-agent clip factor that binds for some agents of a launch
and not for others, an exactly one-hot policy.  For every case the GPU module runs, on the very same draws, this module states:

  (a) the float32 restatement of the oracle (LY.f32_oracle_class) stays within HALF of the bound the GPU module uses -- gradients 2e-5
      max|g| in the first round and 2e-4 in the second, pi 2e-5, v value_bound -- so that a kernel keeps room for its own rounding;
  (b) `peaked` / `gates`: at least 5 % of the taken actions lie below the clamp and at least 5 % above, and no probability of any
      (sample, agent, action) has |ln(pi / 1e-10)| below the case's window w = 10 x the largest |d logit| between the restatement and
      float64, at least 1e-5: a correct float32 evaluation puts every probability on the oracle's side of the clamp;
  (c) `half_clip`: in each round an agent's norm lies below 0.99 x 40 and another's above 1.01 x 40, none in between; `peaked`: every
      agent above 1.01 x 40;
  (d) `gates`, LSTM: at least a tenth of the oracle's gate activations over (sample, unit, gate) lie outside (1e-3, 1 - 1e-3) (the
      candidate gate tanh as (1 + u) / 2).  The FcACPolicy has no gates: there the regime scales its ReLU layer and (d) does not apply;
  (e) no oracle gradient tensor has max|g| below 1e-5 (the relative measure means nothing there), and at most 4 hidden columns of a
      tower sit on a ReLU kink, as for the old layouts;
  (f) `onehot`: the restatement's pi is exactly 1.0 at the chosen action and below 1e-38 elsewhere on every sample.

The condition of tests/test_layouts_host.py that every action has a probability in (1e-4, 1 - 1e-4) on some sample (_open_heads) is NOT
required here: it exists because a saturated softmax passes any kernel that is compared on pi alone, and these cases are compared on what
saturation itself must produce -- the clamp branch's zeroed policy term in the gradients, the clip factor in the parameters, exact
zeros and exact ones.  (b) - (f) take its place.

Every test prints its figures: clamp share, window, norm range, gate share, the restatement's worst figure."""
import numpy as np
import pytest
import torch

from tests import layouts as LY
from tests.test_layouts_host import _a2c_pair, value_bound

LN_CLAMP = float(np.log(LY.CLAMP))
CLIP = 40.0                                     # A2C_DEFAULTS max_grad_norm


def _logits(o, dt):
    """The policy logits of the rollout in o's buffer under o's current parameters, through oracle.nets_oracle.tower -> list[A] of [T, E, n_a] float64."""
    from oracle.nets_oracle import t64, tower
    obs, dones = np.stack(o.buf['obs']), np.stack(o.buf['dones'])
    out = []
    with LY.oracle_dtype(dt), torch.no_grad():
        for a in range(o.A):
            lo, _ = tower(o.p[2 * a], o._ob(obs, a), t64(dones[:-1]), o.s_bw[2 * a], o.nw[a], o.nt[a], o.nf[a])
            out.append(lo.double().numpy())
    return out


def _logp(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _clamp_figures(o64, o32):
    """-> (share of the taken actions below the clamp, smallest |ln(pi / 1e-10)| over every (sample, agent, action), window w)."""
    l64, l32 = _logits(o64, torch.float64), _logits(o32, torch.float32)
    acts = np.stack(o64.buf['acts'])
    below = total = 0
    near, dl = np.inf, 0.0
    for a, (x, y) in enumerate(zip(l64, l32)):
        lp = _logp(x)
        near, dl = min(near, float(np.abs(lp - LN_CLAMP).min())), max(dl, float(np.abs(x - y).max()))
        taken = np.take_along_axis(lp, acts[:, :, a][..., None], -1)[..., 0]
        below, total = below + int((taken < LN_CLAMP).sum()), total + taken.size
    return below / total, near, max(10 * dl, 1e-5)


def _gate_share(o):
    """Share of the float64 oracle's gate activations of the rollout in its buffer, both towers, outside (1e-3, 1 - 1e-3)."""
    from oracle.nets_oracle import t64, tower_activations
    obs, dones = np.stack(o.buf['obs']), np.stack(o.buf['dones'])
    out = n = 0
    with torch.no_grad():
        for g in range(2 * o.A):
            a, s = g // 2, o.s_bw[g].clone()
            for t in range(obs.shape[0]):
                r = tower_activations(o.p[g], o._ob(obs[t], a), t64(dones[t]), s, o.nw[a], o.nt[a], o.nf[a])
                z = r['gates'].numpy().copy()
                z[:, 192:] = 0.5 * (1.0 + z[:, 192:])
                out, n = out + int(((z <= 1e-3) | (z >= 1 - 1e-3)).sum()), n + z.size
                s = torch.cat([r['c'], r['h']], 1)
    return out / n


def _regime_update(regime, name, policy, E, T, rounds=2):
    from tests.test_model_gpu import _grad_err
    lay, c, o64, o32 = _a2c_pair(name, policy, E, regime=regime)
    assert c['max_grad_norm'] == CLIP
    rng = np.random.RandomState(LY.regime_data_seed(regime, name, policy, E, T))
    hot = LY.onehot_action(lay)
    for it in range(rounds):
        pis32, vs32, vs64 = [], [], []           # fill_host returns the first oracle's pi: record the values and the second one's pi too
        f64, f32 = o64.forward, o32.forward
        o64.forward = lambda *a, **k: (lambda r: (vs64.append(r[1]), r)[1])(f64(*a, **k))
        o32.forward = lambda *a, **k: (lambda r: (pis32.append(r[0]), vs32.append(r[1]), r)[2])(f32(*a, **k))
        obs, done, pis = LY.fill_host(lay, [o64, o32], E, T, rng, c['reward_norm'])
        o64.forward, o32.forward = f64, f32
        dpi = max(np.abs(x - y).max() for s64, s32 in zip(pis, pis32) for x, y in zip(s64, s32))
        assert dpi <= 1e-5, 'round %d: float32 restatement |dpi| %.2e' % (it, dpi)
        for v64, v32 in zip(vs64, vs32):
            assert np.abs(v32 - v64).max() <= 0.5 * value_bound(v64)
        if regime == 'onehot':
            for s32 in pis32:
                for a, p in enumerate(s32):
                    assert (p[:, hot[a]] == 1.0).all() and (np.delete(p, hot[a], 1) < 1e-38).all(), (it, a)
        share, near, w = _clamp_figures(o64, o32)
        gate = _gate_share(o64) if policy == 'lstm' else float('nan')
        _, Rb = o64.forward(obs, np.zeros(E), 'v')
        o32.forward(obs, np.zeros(E), 'v')
        Rb = Rb.astype(np.float32)
        g64, _ = o64.compute_grads(Rb, 0.01)
        g32, _ = o32.compute_grads(Rb, 0.01)
        np.testing.assert_array_equal(o64.Rs, o32.Rs)
        worst, kinks = 0.0, 0
        for t, kc in enumerate(o64.kink_cols):
            n_kink = sum(int(cols.sum()) for cols in kc.values())
            kinks = max(kinks, n_kink)
            assert n_kink <= 4, 'round %d tower %d: %d hidden columns on a ReLU kink' % (it, t, n_kink)
            if regime == 'onehot' and t % 2 == 0:
                assert all(float(g.abs().max()) < 1e-30 for g in g64[t].values())   # the device's are exactly zero (GPU module)
                continue
            for k, og in g64[t].items():
                assert float(og.abs().max()) >= 1e-5, 'round %d tower %d %s: oracle max|g| %.1e' % (it, t, k, float(og.abs().max()))
                err = _grad_err(o64, t, k, g32[t][k].double().numpy(), og.numpy())
                worst = max(worst, err)
                assert err <= (1e-5 if it == 0 else 1e-4), 'round %d tower %d %s: float32 restatement |dg| / max|g| = %.2e' % (it, t, k, err)
        lr = LY.HALF_CLIP_LR if regime == 'half_clip' else 5e-4
        ms_before = [{k: v.numpy().copy() for k, v in m.items()} for m in o64.ms]
        norms = o64.apply_grads(g64, lr)
        o32.apply_grads(g32, lr)
        print('%s %s %s E=%d T=%d round %d: taken below the clamp %.3f, nearest |ln(pi / 1e-10)| %.2e (window %.1e), norms %.1f ... %.1f, '
              'gates saturated %.3f, restatement worst |dg| / max|g| %.1e, |dpi| %.1e, kink columns <= %d'
              % (regime, name, policy, E, T, it, share, near, w, norms.min(), norms.max(), gate, worst, dpi, kinks))
        if regime in ('peaked', 'gates'):
            assert 0.05 <= share <= 0.95, 'round %d: %.3f of the taken actions below the clamp' % (it, share)
        if regime != 'onehot':
            assert near >= w, 'round %d: a probability within %.2e of the clamp (window %.1e)' % (it, near, w)
        if regime == 'half_clip':
            assert (norms < 0.99 * CLIP).any() and (norms > 1.01 * CLIP).any() and not ((norms >= 0.99 * CLIP) & (norms <= 1.01 * CLIP)).any(), norms
            gap = LY.clip_step_gap([{k: v.numpy() for k, v in g.items()} for g in g64], ms_before, norms, CLIP, lr)
            print('    a clipped agent stepped with factor 1 moves a parameter by at least %.1e (100 x the parameter tolerance: 3.0e-03)' % gap)
            assert gap >= 100 * 3e-5, 'gap %.2e' % gap
        if regime == 'peaked':
            assert (norms > 1.01 * CLIP).all(), norms
        if regime == 'gates' and policy == 'lstm':
            assert gate >= 0.1, 'round %d: %.3f of the gate activations saturated' % (it, gate)


@pytest.mark.parametrize('regime,name,policy,E,T', LY.regime_cases())
def test_regime_update_conditions(regime, name, policy, E, T):
    _regime_update(regime, name, policy, E, T)


@pytest.mark.parametrize('regime,name,policy', LY.regime_forward_cases())
def test_regime_forward_conditions(regime, name, policy):
    """The forward cases: pi and v of the restatement within half the bounds; `onehot`: exactly one-hot."""
    E = LY.A2C_FORWARD_E
    lay, c, o64, o32 = _a2c_pair(name, policy, E, regime=regime)
    steps, boot = LY.forward_inputs(lay, E, LY.A2C_FORWARD_STEPS, np.random.RandomState(LY.data_seed(name, E)))
    hot, worst, pmin = LY.onehot_action(lay), 0.0, 1.0
    for obs, done in steps:
        pi, v = o64.forward(obs, done, 'pv')
        pi32, v32 = o32.forward(obs, done, 'pv')
        assert np.abs(v32 - v).max() <= 0.5 * value_bound(v)
        worst = max(worst, max(np.abs(a - b).max() for a, b in zip(pi, pi32)))
        pmin = min(pmin, min(float(p.min()) for p in pi))
        if regime == 'onehot':
            for a, p in enumerate(pi32):
                assert (p[:, hot[a]] == 1.0).all() and (np.delete(p, hot[a], 1) < 1e-38).all(), a
    assert worst <= 1e-5
    _, vb = o64.forward(boot, np.zeros(E), 'v')
    _, vb32 = o32.forward(boot, np.zeros(E), 'v')
    assert np.abs(vb32 - vb).max() <= 0.5 * value_bound(vb)
    print('%s %s %s: smallest oracle probability %.1e, float32 restatement |dpi| %.1e' % (regime, name, policy, pmin, worst))


def _ppo_pair(lr):
    """The PPO oracle of the GPU module's case and its float32 restatement, filled with the case's rollout -> (o64, o32, bootstrap values)."""
    from tests import ppo_oracle as PO
    spec = LY.A2C_LAYOUTS['head8']
    lay = spec['layout']
    E, T, seed, rseed, _ = LY.REGIME_PPO
    cfg = dict(spec['cfg'], reward_norm=PO.K3_REWARD_NORM)
    tw = LY.apply_regime(PO.make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=cfg, layout=lay).tower_params(), 'peaked', lay)
    o64 = PO.make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=cfg, layout=lay, towers=tw)
    saved, PO.PPOOracle = PO.PPOOracle, LY.f32_oracle_class(PO.PPOOracle)
    try:
        o32 = PO.make_oracle(None, 'ma2c', 'lstm', E, seed, cfg=cfg, layout=lay, towers=tw)
    finally:
        PO.PPOOracle = saved
    o64.reset(); o32.reset()
    obs, _ = PO.fill(lay, o64, E, T, np.random.RandomState(rseed), PO.K3_REWARD_NORM)
    PO.fill(lay, o32, E, T, np.random.RandomState(rseed), PO.K3_REWARD_NORM, put=lambda t, *a: o64.buf['vs'][t].astype(np.float32))
    _, Rb = o64.forward(obs, np.zeros(E), 'v')
    return o64, o32, Rb.astype(np.float32)


def test_ppo_peaked_conditions(lr=None):
    """The PPO case of the GPU module (head8, `peaked`, K = 2) on the oracle alone.  At both epochs at least 5 % of the taken actions sit
    below the clamp -- where they do at both, logp_old and logp are log 1e-10, the ratio is 1 and the sample's policy gradient is 0 -- and
    none within the window of it; at epoch 1 the clipped share lies in (5 %, 95 %); the restatement's |d logit| (a tenth of the window)
    stays below the relative 1e-4 within which tests/ppo_oracle.py calls a ratio ambiguous and grants its contribution as slack; with
    that slack the float32 restatement stays within half the gradient bounds, and no gradient tensor vanishes (conditions (a), (b),
    (e) of the module).  lr 5e-5: at 2e-4 and above the policy collapses within one epoch (KL 0.35 - 3.3), 1 - pi of a taken action
    cancels in float32 and the restatement itself leaves the bound (1.9e-4 at 2e-4, 7.7e-4 at 5e-4)."""
    from tests.test_model_gpu import _grad_err
    lr = LY.REGIME_PPO[4] if lr is None else lr
    o64, o32, Rb = _ppo_pair(lr)
    for k in range(2):
        share, near, w = _clamp_figures(o64, o32)
        g64, _ = o64.compute_grads(Rb, 0.01, epoch=k, slack=True)
        g32, _ = o32.compute_grads(Rb, 0.01, epoch=k, slack=False)
        clip, amb = float(o64.clip_share.mean()), float(o64.amb_share.mean())
        worst, gmin = 0.0, np.inf
        for t in range(len(g64)):
            assert sum(int(c.sum()) for c in o64.kink_cols[t].values()) <= 4
            for key, og in g64[t].items():
                gmin = min(gmin, float(og.abs().max()))
                d = (g32[t][key].double() - og).abs() - o64.amb_slack[t][key]
                worst = max(worst, _grad_err(o64, t, key, (og + d.clamp(min=0)).numpy(), og.numpy()))
        print('head8 peaked PPO lr %.0e epoch %d: taken below the clamp %.3f, nearest |ln(pi / 1e-10)| %.2e (window %.1e), clipped share %.3f, '
              'ambiguous %.4f, kl %.3f, smallest max|g| %.1e, restatement worst |dg| / max|g| %.1e'
              % (lr, k, share, near, w, clip, amb, o64.approx_kl.mean(), gmin, worst))
        assert 0.05 <= share <= 0.95 and near >= w and amb <= 0.005 and w <= 10 * 1e-4
        assert gmin >= 1e-5 and worst <= (1e-5 if k == 0 else 1e-4)
        if k == 1:
            assert 0.05 < clip < 0.95
        o64.apply_grads(g64, lr, end_of_rollout=(k == 1))
        o32.apply_grads(g32, lr, end_of_rollout=(k == 1))


# ---- the Q-learners -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LY.IQL_REGIME_LAYOUTS)
def test_iql_tied_conditions(name):
    """`tied`: on every row the GPU module evaluates -- the forward observations and every next observation that enters the rings -- the
    oracle's values of the two tied columns are bit-equal, they are the row's maximum by more than 1, and np.argmax (the first maximum)
    is the lower column j.  Rows are evaluated an instance batch (E = 5) at a time: over the 100 rows of a minibatch the float64 matmul
    blocks the head's columns and may round two identical columns an ulp apart, which is why the GPU module takes a* = j from the
    rule and not from the oracle's own argmax there."""
    from tests.test_layouts_host import _iql_pair
    lay, o64, _ = _iql_pair(name, 'tied')
    E = LY.IQL_E
    rng = np.random.RandomState(LY.data_seed(name, E))
    rows = [LY.rand_obs(lay, E, rng) for _ in range(3)]
    rows += [tr[3] for tr in LY.iql_transitions(lay, E, LY.IQL_CAP, np.random.RandomState(LY.data_seed(name, E, LY.IQL_CAP)), LY.IQL_REWARD_NORM)]
    for obs in rows:
        for a, q in enumerate(o64.forward(obs)):
            j, k = LY.tie_pair(a, lay.n_a_ls[a])
            assert np.array_equal(q[:, j], q[:, k]) and (np.argmax(q, 1) == j).all()
            rest = np.delete(q, [j, k], 1)
            assert rest.size == 0 or (rest.max(1) < q[:, j] - 1.0).all()


@pytest.mark.parametrize('name', LY.IQL_REGIME_LAYOUTS)
def test_iql_clip_conditions(name):
    """`clip`: in each of the three Adam steps an agent's norm lies below 0.99 x 40 and another's above 1.01 x 40, none in between
    (condition (c)), and for the most clipped agent a step taken with factor 1 differs from the clipped one by at least 100 x the bound
    the GPU module compares the step at (LY.adam_step_bound).  Second moments preloaded with 1, first moments 0, t = 0: Adam's own
    normalisation would otherwise hide a constant factor."""
    from tests.test_layouts_host import _iql_pair
    lay, o64, _ = _iql_pair(name, 'clip')
    E = LY.IQL_E
    for tr in LY.iql_transitions(lay, E, LY.IQL_CAP, np.random.RandomState(LY.data_seed(name, E, LY.IQL_CAP)), LY.IQL_REWARD_NORM):
        o64.add_transition(*tr)
    for q in o64.qs:
        q.v = {k: torch.ones_like(v) for k, v in q.p.items()}
    b1, b2, eps = 0.9, 0.999, 1e-8
    for step in range(LY.IQL_CLIP_STEPS):
        before = [({k: v.numpy().copy() for k, v in q.p.items()}, {k: v.numpy().copy() for k, v in q.m.items()},
                   {k: v.numpy().copy() for k, v in q.v.items()}) for q in o64.qs]
        _, norms, g = o64.minibatch_step(LY.IQL_CLIP_LR)
        assert (norms < 0.99 * CLIP).any() and (norms > 1.01 * CLIP).any() and not ((norms >= 0.99 * CLIP) & (norms <= 1.01 * CLIP)).any(), norms
        a = int(np.argmax(norms))
        p0, m0, v0 = before[a]
        t = step + 1
        lr_t = LY.IQL_CLIP_LR * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        ratio = 0.0
        for k in p0:
            d_true = o64.qs[a].p[k].numpy() - p0[k]
            m1, v1 = b1 * m0[k] + (1 - b1) * g[a][k], b2 * v0[k] + (1 - b2) * g[a][k] ** 2
            d_alt = -lr_t * m1 / (np.sqrt(v1) + eps)
            ratio = max(ratio, float(np.abs(d_alt - d_true).max()) / LY.adam_step_bound(d_true, p0[k]))
        print('%s clip step %d: norms %.1f ... %.1f; agent %d stepped with factor 1 is off by %.0f x the step bound' % (name, step, norms.min(), norms.max(), a, ratio))
        assert ratio >= 100
