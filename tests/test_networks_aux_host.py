"""The cases of tests/test_networks_aux_gpu.py on the host (no GPU, no library): the CPU oracle alone runs the very seeds, actions and
steps of networks.AUX, and what each GPU comparison rests on is stated as an assertion -- the flat walk of the pressure kernels goes
into its second round, pressures take both signs, greedy decisions are tied and clipped, every lane-data field is counted somewhere,
the last interval is the partial one, flow windows cover 4-second words partly.  A network that stops showing its condition (a
changed compiler, another seed) fails here, not silently on the GPU.  Every case prints the figures its conditions rest on."""
import numpy as np
import pytest

from tests import env_harness as H
from tests import networks as nw
from tests.env_rules import F, INTS, greedy_rule, hold_state, hold_update, lane_data_reference, loop_pressure


# ---- 0. the greedy tables of a scenario with laneless 'G' links ------------------------------------------------------------
def test_link62_greedy_tables_skip_links_without_a_lane():
    """link62's phase strings have 'G' on signal links no lane uses (link_lane -1): the tables build, every one of the 8 phases is
    a candidate, and the terms are the positions of the six used links' lanes alone."""
    scn = nw.NETWORKS['link62'].scenario()
    used = [0, 13, 31, 47, 61, 62]
    assert any(scn.green_tab[0, p, k] == ord('G') and scn.link_lane[0, k] < 0 for p in range(8) for k in range(63))
    n_cand, term, action = scn.greedy_controller_tables()
    assert n_cand.tolist() == [8] and action.tolist() == [list(range(8))]
    lanes = [int(x) for x in scn.agent_lanes[0, :scn.agent_nlane[0]]]
    assert len(lanes) == 6
    for p in range(8):
        want = []
        for k in used:                                          # link order, every lane once
            j = lanes.index(int(scn.link_lane[0, k]))
            if scn.phases[0][p][k] == 'G' and j not in want:
                want.append(j)
        got = [int(j) for j in term[0, p] if j >= 0]
        assert got == want, (p, got, want)
        assert (term[0, p, len(got):] == -1).all()
    assert sorted(set(term[term >= 0].tolist())) <= list(range(6))


def test_an_empty_candidate_has_flow_zero():
    """A phase whose 'G' links are all laneless is an empty candidate: flow 0.0, which loses to any vehicle and wins only by coming
    first among zeros."""
    scn = nw.merge4('zipper', phases0=('rrrr', 'GGrr', 'rrGG', 'GrGr'))
    n_cand, term, action = scn.greedy_controller_tables()
    assert n_cand[0] == 4 and (term[0, 0] == -1).all()
    tab = (term[0], action[0], n_cand[0])
    assert greedy_rule(tab, np.zeros(4)) == (0, [0.0, 0.0, 0.0, 0.0])
    assert greedy_rule(tab, np.array([0.0, 0.0, 0.2, 0.0]))[0] == 2


# ---- 1. the additions to tests/networks.py ------------------------------------------------------------------------------
def test_windows_has_every_kind_of_window():
    scn = nw.NETWORKS['windows'].scenario()
    fl = np.asarray(scn.flows, np.int64)
    table = (scn.episode_length_sec + 64 + 3) // 4 * 4
    assert (scn.control_interval_sec, scn.yellow_interval_sec, scn.episode_length_sec) == (1, 0, nw.WINDOWS_EPISODE) and table == 184
    b, en, vph, st = fl.T
    live = (vph > 0) & (en > b)
    assert {1, 2, 3} <= set((b[live] % 4).tolist()) and {1, 2, 3} <= set((en[live] % 4).tolist())
    assert ((en - b == 1) & (vph > 0)).any() and ((en == b) & (vph > 0)).any() and (vph == 0).any()
    assert ((en > table) & (b < table)).any() and (b > table).any()
    over = [(i, j) for i in range(len(fl)) for j in range(i + 1, len(fl)) if st[i] == st[j] and live[i] and live[j]
            and max(b[i], b[j]) < min(en[i], en[j])]
    assert len(over) >= 2 and nw.WINDOWS_PAIR in over
    a_, b_ = nw.WINDOWS_PAIR
    assert b[b_] == b[a_] + 1 and min(en[a_], en[b_]) - b[b_] == 2           # the pair shares two seconds; the second begins a second later
    assert not [j for j in range(len(fl)) if j not in nw.WINDOWS_PAIR and st[j] == st[a_] and b[j] < en[b_] and en[j] > b[a_]]
    assert np.bincount(scn.stream_entry_lane).max() == 2                    # two streams on one entry lane


def test_split_pieces_cuts_lanes_at_values_float32_does_not_hold():
    base = nw.NETWORKS['merge4_zipper'].scenario()
    scn = nw.aux_scenario('merge4_pieces')
    assert [len(ps) for ps in base.lane_pieces] == [1] * 6
    assert sorted(len(ps) for ps in scn.lane_pieces) == [1, 1, 1, 2, 3, 5]
    names = [nm for ps in scn.lane_pieces for nm, _, _ in ps]
    assert len(set(names)) == len(names) == 13
    tabs = scn.lane_data_slots()
    assert tabs['names'] == names and tabs['slot0'].tolist() == np.cumsum([0] + [len(ps) for ps in scn.lane_pieces]).tolist()
    cuts = sorted({c for cs in nw.MERGE4_CUTS.values() for c in cs})
    odd = [c for c in cuts if float(np.float32(c)) != c]
    assert {33.3, 61.7} <= set(odd)
    for l, ps in enumerate(scn.lane_pieces):
        assert abs(sum(p[2] for p in ps) - float(scn.lane_len[l])) < 1e-9
    # a slot's float32 start is the least float32 at or past the float64 start: a position compares with it as with the float64 cut
    s0 = np.concatenate([np.cumsum([0.0] + [p[2] for p in ps])[:-1] for ps in scn.lane_pieces])
    assert (tabs['start'].astype(np.float64) >= s0).all() and (np.nextafter(tabs['start'], np.float32(-np.inf)).astype(np.float64)[s0 > 0] < s0[s0 > 0]).all()
    assert base.lane_pieces is not scn.lane_pieces and scn.name == 'merge4_zipper_pieces'


def test_aux_table_runs_are_short():
    for fam, cases in nw.AUX.items():
        for c in (cases if isinstance(cases, list) else [cases]):
            net = nw.NETWORKS[c.net_name]
            assert 2 <= c.E <= 4 and nw.walk_steps(c) <= max(net.steps, nw.walk_steps(nw.Aux(c.key, c.net_name, c.E, None))), (fam, c)


# ---- 2. max pressure ------------------------------------------------------------------------------------------------------
def _pressure_figures(case):
    """Over the compared steps of a pressure case: most vehicles on the walked lanes, pressure range, whether the agents' actions
    differ within an instance and how many decisions are tied at the maximum, per measure."""
    scn, tb = case.scenario(), case.scenario().pressure_tables()
    fig = {m: dict(live=0, lo=0, hi=0, differ=False, ties=0, n=0) for m in ('count', 'queue')}
    for t, acts, pols, res, orc in nw.aux_run(case):
        if t < 0 or not case.compared(t):
            continue
        for o in orc:
            sn = o.ms.snapshot()
            for m, f in fig.items():
                act, prs = loop_pressure(scn, tb, sn, m)
                f['live'] = max(f['live'], int(sn['n'][tb['walk']].sum()))
                f['lo'], f['hi'] = min(f['lo'], int(prs.min())), max(f['hi'], int(prs.max()))
                f['differ'] |= len(set(act.tolist())) > 1
                for a in range(scn.n_agent):
                    row = prs[a, :int(scn.agent_nphase[a])]
                    f['ties'] += int((row == row.max()).sum() > 1)
                f['n'] += 1
    return scn, tb, fig


@pytest.mark.parametrize('case', nw.AUX['pressure'], ids=repr)
def test_pressure_cases_are_not_vacuous(case):
    scn, tb, fig = _pressure_figures(case)
    chunk = -(-len(tb['walk']) // 256)
    for m, f in fig.items():
        print('%s %s: %d walked lanes (chunk %d), %d movements, %d (agent, phase) pairs; %d compared states, most vehicles on the walked '
              'lanes %d, pressure in [%d, %d], actions differ %s, tied decisions %d'
              % (case, m, len(tb['walk']), chunk, len(tb['mov']), scn.n_agent * scn.green_tab.shape[1], f['n'], f['live'], f['lo'], f['hi'],
                 f['differ'], f['ties']))
        assert f['n'] >= 4 * case.E and (f['lo'] < 0 or f['hi'] > 0)
    if case.key in ('isolated_130', 'isolated_300', 'grid_x4'):
        assert chunk == {'isolated_130': 2, 'isolated_300': 3, 'grid_x4': 3}[case.key]
        assert fig['count']['live'] > 256                        # the second round of the flat walk
        assert fig['count']['lo'] < 0 < fig['count']['hi'] and fig['count']['differ']
    if case.key == 'isolated_300':
        assert scn.n_agent > 256 and scn.n_agent * scn.green_tab.shape[1] > 256
    if case.key == 'grid_x4':
        assert len(tb['mov']) > 4 * 256 and fig['queue']['lo'] < 0 < fig['queue']['hi'] and fig['queue']['differ']
    if case.key == 'link62':
        assert fig['count']['ties'] > 0                          # two phases tied at the maximum: the first must win


def test_hold_case_is_not_vacuous():
    """The hold run of the GPU module, oracle in the loop: the controller's own choices under min_green drive the traffic."""
    case = nw.AUX['hold']
    scn, tb, g = case.scenario(), case.scenario().pressure_tables(), case.min_green
    for t, acts, pols, res, orc in nw.aux_run(case):
        pass
    state = hold_state(case.E, scn.n_agent, g)
    cur, age, _ = state
    t, n_changes = 0, 0
    while t < case.least or not ((age < g) & (cur != 0)).any():
        assert t < case.most, 'no agent inside a hold on a phase other than 0'
        for e, o in enumerate(orc):
            p_star, _ = loop_pressure(scn, tb, o.ms.snapshot(), 'count')
            n_changes += hold_update(state, e, p_star, t, g)
        for e, o in enumerate(orc):
            o.step(list(cur[e]))
        t += 1
    print('hold on %s: %d control steps, %d phase changes of %d agents' % (case, t, n_changes, scn.n_agent))
    assert n_changes > 10 and scn.n_agent > 256 and (cur[:, 256:] != 0).any()


@pytest.mark.parametrize('case', nw.AUX['reward'], ids=repr)
def test_reward_cases_are_not_vacuous(case):
    from deeprl_signal_control_amd.trainer import pressure_reward
    scn, tb = case.scenario(), case.scenario().pressure_tables()
    live, lo, hi, n, gsum = 0, 0, 0, 0, 0.0
    for t, acts, pols, res, orc in nw.aux_run(case):
        if t < 0 or not case.compared(t):
            continue
        for o in orc:
            sn = o.ms.snapshot()
            _, g, P = pressure_reward(scn, sn, case.measure, train_mode=case.train_mode)
            live, lo, hi, n, gsum = max(live, int(sn['n'][tb['walk']].sum())), min(lo, int(P.min())), max(hi, int(P.max())), n + 1, gsum + g
    print('%s %s: %d compared states, most vehicles on the walked lanes %d, P in [%d, %d]' % (case, case.measure, n, live, lo, hi))
    assert n >= 4 * case.E and gsum < 0 and (lo < 0 or hi > 0)
    if case.measure == 'count':
        assert lo < 0 < hi                                       # both signs: the absolute value matters
    if case.key in ('isolated_130_ma2c', 'isolated_300'):
        assert live > 256
    if case.key == 'isolated_130_ma2c':
        assert scn.agent == 'ma2c' and all(len(nb) == 2 for nb in scn.neighbors)


# ---- 3. greedy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.AUX['greedy'], ids=repr)
def test_greedy_cases_are_not_vacuous(case):
    scn = case.scenario()
    n_cand, term, action = scn.greedy_controller_tables()
    clip = float(scn.clip_wave)
    ties, decisions, clipped, acts_seen = 0, 0, 0, set()
    for t, acts, pols, res, orc in nw.aux_run(case):
        obs = res if t < 0 else [r[0] for r in res]
        for e in range(case.E):
            for a in range(scn.n_agent):
                act, flows = greedy_rule((term[a], action[a], n_cand[a]), obs[e][a])
                ties += int(max(flows) > 0 and sum(f == max(flows) for f in flows) > 1)
                decisions += 1
                acts_seen.add(act)
                clipped += int((np.asarray(obs[e][a][:int(scn.agent_nlane[a])]) == clip).sum())
    print('%s: %d decisions, %d tied at a nonzero maximum, %d clipped wave entries, actions %s' % (case, decisions, ties, clipped, sorted(acts_seen)))
    assert ties > 0
    if case.net_name != 'merge4_zipper':         # (merge4's first phase is green for every lane: the first candidate always wins, by a
        assert len(acts_seen) > 1                #  tie or outright -- what these two runs pin is the tie and the clip; the exhaustive case has the rest)
    if case.key == 'merge4_n3':
        assert (scn.norm_wave, scn.clip_wave) == (3.0, 1.5) and clipped > 0


@pytest.mark.parametrize('norm,clip', nw.GREEDY_NORMS)
def test_greedy_enumeration_tells_float32_sums_from_the_float64_rule(norm, clip):
    scn, counts, ob32, want, naive64, naive32 = nw.greedy_exhaustive(norm, clip)
    print('norm_wave %g clip_wave %g: %d tuples, %d clipped entries; the float32 entries added in float64 pick another action in %d, '
          'added in float32 in %d; actions %s' % (norm, clip, len(counts), int((ob32 == np.float32(clip)).sum()), int((want != naive64).sum()),
                                                  int((want != naive32).sum()), np.bincount(want).tolist()))
    assert len(counts) == 9 ** 4 and clip < 8 / norm
    assert (want != naive64).any() and (ob32 == np.float32(clip)).any() and len(set(want.tolist())) == 4
    if norm == 5.0:
        i = counts.tolist().index([1, 2, 0, 3])                 # 3 / 5 against 1 / 5 + 2 / 5
        assert want[i] != naive32[i]


# ---- 4. the recording walks -----------------------------------------------------------------------------------------------
_walk_sums = {}


def _walk_reference(case):
    if case.key not in _walk_sums:
        scn = case.scenario()
        with H.walk_context(case):
            orc = H.WalkOracles(case)
            rng = np.random.RandomState(case.rng_seed)
            for _ in range(nw.walk_steps(case)):
                orc.step(H.uniform_actions(scn, rng, case.E))
        views = orc.views()
        _walk_sums[case.key] = {e: lane_data_reference(scn, v.snaps, case.period)[0] for e, v in views.items()}, views
    return _walk_sums[case.key]


@pytest.mark.parametrize('case', nw.AUX['walk'], ids=repr)
def test_walk_cases_are_not_vacuous(case):
    scn = case.scenario()
    sums, views = _walk_reference(case)
    tot = sum(s.sum(axis=(0, 2)) for s in sums.values())
    most = max(int(sn['n'].sum()) for v in views.values() for sn in v.snaps)
    print('%s: %d live lanes, %d slots, %d intervals of %d s; most vehicles %d; %s'
          % (case, scn.live_lane_prefix(), len(scn.lane_data_slots()['start']), next(iter(sums.values())).shape[0], case.period, most,
             ', '.join('%s %d' % (k, tot[F[k]]) for k in INTS)))
    for k in ('sampledSeconds', 'waitingTime', 'departed', 'arrived'):
        assert tot[F[k]] > 0, k
    T = int(scn.episode_length_sec)
    if case.steps is None:                                       # to the end of the episode
        assert all(len(v.snaps) == T for v in views.values())
    if case.key == 'isolated_130_200s':
        assert scn.live_lane_prefix() == 260 and T % case.period != 0 and most > 256
    if case.key == 'burst':
        assert tot[F['teleported']] > 0
    if case.key == 'merge4_pieces':
        assert tot[F['entered']] > 0 and tot[F['left']] == tot[F['entered']]
    if case.key == 'grid_x2':
        assert tot[F['laneChangedFrom']] > 0 and tot[F['laneChangedTo']] == tot[F['laneChangedFrom']]
    if case.key == 'ctrl8':
        assert (T, case.period, scn.control_interval_sec) == (500, 56, 8) and T == 8 * 56 + 52
        for s in sums.values():
            assert s.shape[0] == 9 and s[8, F['sampledSeconds']].sum() > 0          # the partial last interval holds samples
        assert nw.walk_steps(case) * 8 > T                       # ... and the last launch runs past the episode's end
    if case.key == 'ctrl1':
        assert scn.control_interval_sec == 1 and case.period == 7


def test_walk_family_counts_every_field():
    tot = np.zeros(len(INTS), np.int64)
    for case in nw.AUX['walk']:
        for s in _walk_reference(case)[0].values():
            tot += s.sum(axis=(0, 2))
    print('walk family: ' + ', '.join('%s %d' % (k, tot[F[k]]) for k in INTS))
    assert (tot > 0).all()


# ---- 5. per-instance demand -----------------------------------------------------------------------------------------------
def _partial_words(scn, vph):
    """Flow elements (rate > 0, inside the emission table) whose window begins / ends inside a 4-second word."""
    fl = np.asarray(scn.flows, np.int64)
    table = (scn.episode_length_sec + 64 + 3) // 4 * 4
    live = (np.asarray(vph) > 0) & (fl[:, 1] > fl[:, 0]) & (fl[:, 0] < table)
    return int((live & (fl[:, 0] % 4 != 0)).sum()), int((live & (fl[:, 1] % 4 != 0) & (fl[:, 1] < table)).sum())


def test_demand_columns_of_windows():
    case = nw.AUX['demand']
    scn = case.scenario()
    cols = nw.windows_columns(scn)
    assert cols.shape == (case.E, len(scn.flows)) and len({c.tobytes() for c in cols}) == case.E
    peaks = []
    for e, col in enumerate(cols):
        peak = nw.with_rates(scn, col).check_limits().peak_emission()
        begins, ends = _partial_words(scn, col)
        print('windows column %d: peak emission %d (flow %d, stream %d), words partly covered at %d begins and %d ends' % ((e,) + peak + (begins, ends)))
        assert peak[0] <= 255 and begins >= 1 and ends >= 1
        peaks.append(peak[0])
    assert peaks[1] == 255 and peaks[3] == 255 and peaks[2] >= 3
    a, b = nw.WINDOWS_PAIR
    bound = lambda col: sum(-(-int(col[f]) // 3600) for f in (a, b))
    assert bound(cols[1]) == 255 and bound(cols[3]) == 256      # column 3: only the per-second path of the host check can accept it
    col, flow, second = nw.windows_refused_column(scn)
    with pytest.raises(ValueError, match='emit 256 vehicles in one second'):
        nw.with_rates(scn, col).check_limits()
    assert flow == b and second == int(scn.flows[b, 0])


def test_demand_254_streams():
    case = nw.AUX['demand254']
    scn = case.scenario()
    assert scn.n_stream == 254 and len(scn.flows) == 254 and case.E == 3
    vph = nw.demand254_columns(scn, case.E)
    assert vph.shape == (3, 254) and len({c.tobytes() for c in vph}) == 3
    for col in vph:
        assert nw.with_rates(scn, col).check_limits().peak_emission()[0] <= 255
