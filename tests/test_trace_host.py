"""CPU side of the trajectory trace (tsc_env_trace, VecTrafficEnv.set_trace): the simulator-lane -> SUMO-lane tables of the three
scenarios (Scenario.lane_pieces / sumo_lane_pos), the decoding of the device's rows and the --trajectories flag."""
import re

import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import build_large_grid, build_real_net, build_small_grid

SCENARIOS = {'large_grid': lambda: build_large_grid('greedy'), 'real_net': lambda: build_real_net('greedy'),
             'small_grid': lambda: build_small_grid('greedy')}


def _sumo_lanes(name):
    """SUMO lane id -> length, from a source independent of the pieces: the uncontracted Monaco net; small_grid's edges
    (one lane each: <from>_<to>_0, whose length is what its cut pieces add up to)."""
    if name == 'real_net':
        raw = build_real_net('greedy', contract=False, sort_lanes=False)
        return {nm: float(ln) for nm, ln in zip(raw.lane_names, raw.lane_len)}
    scn = SCENARIOS[name]()
    out = {}
    for nm, ln in zip(scn.lane_names, scn.lane_len):
        base = re.sub(r'#\d+$', '', nm)
        out[base] = out.get(base, 0.0) + float(ln)
    return out


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_pieces_cover_every_lane(name):
    scn = SCENARIOS[name]()
    assert len(scn.lane_pieces) == scn.n_lane
    for l, ps in enumerate(scn.lane_pieces):
        assert ps, scn.lane_names[l]
        assert sum(p[2] for p in ps) == pytest.approx(float(scn.lane_len[l]), rel=1e-6, abs=1e-4), scn.lane_names[l]
        # the lane's own name is its last piece (the one that carries the signal and the detector)
        assert ps[-1][0] == re.sub(r'#\d+$', '', scn.lane_names[l]) if name == 'small_grid' else ps[-1][0] == scn.lane_names[l]


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_piece_names_are_sumo_lanes(name):
    scn = SCENARIOS[name]()
    sumo = _sumo_lanes(name)
    seen = {}
    for ps in scn.lane_pieces:
        for nm, start, ln in ps:
            assert nm in sumo, nm
            assert 0.0 <= start and start + ln <= sumo[nm] * (1 + 1e-6) + 1e-4, (nm, start, ln, sumo[nm])
            seen.setdefault(nm, []).append((start, ln))
            if name == 'small_grid':
                assert not re.search(r'_0#\d+$', nm), nm           # the simulator's cut pieces never leak out
    # every SUMO lane is covered exactly once, without gaps or overlaps
    assert set(seen) == set(sumo)
    for nm, parts in seen.items():
        parts.sort()
        assert parts[0][0] == 0.0
        for (s0, l0), (s1, _) in zip(parts, parts[1:]):
            assert s1 == pytest.approx(s0 + l0, abs=1e-3), nm
        assert parts[-1][0] + parts[-1][1] == pytest.approx(sumo[nm], rel=1e-6, abs=1e-3), nm
    if name == 'real_net':
        assert sum(len(ps) > 1 for ps in scn.lane_pieces) > 0       # contract_chains merged chains: their lengths are kept


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_sumo_lane_pos(name):
    scn = SCENARIOS[name]()
    sumo = _sumo_lanes(name)
    rng = np.random.RandomState(0)
    lane = rng.randint(0, scn.n_lane, 4000)
    x = rng.rand(4000) * scn.lane_len[lane]
    ids, pos = scn.sumo_lane_pos(lane, x)
    assert ids.shape == pos.shape == (4000,)
    for l, xi, nm, p in zip(lane, x, ids, pos):
        off = 0.0
        for pn, start, ln in scn.lane_pieces[l]:                   # the piece that holds x, by a plain walk
            if xi < off + ln or pn == scn.lane_pieces[l][-1][0] and start == scn.lane_pieces[l][-1][1]:
                break
            off += ln
        assert nm == pn
        assert start - 1e-6 <= p <= start + ln + 1e-6 and 0.0 <= p <= sumo[nm] + 1e-4
        assert p == pytest.approx(start + (xi - off), abs=1e-4)
    # ends of the lane: x = 0 is the first piece's start, x = lane length the last piece's end, beyond it stays there
    ids, pos = scn.sumo_lane_pos(np.arange(scn.n_lane), np.zeros(scn.n_lane))
    assert list(ids) == [ps[0][0] for ps in scn.lane_pieces] and np.allclose(pos, [ps[0][1] for ps in scn.lane_pieces])
    ids, pos = scn.sumo_lane_pos(np.arange(scn.n_lane), scn.lane_len.astype(np.float64) + 50.0)
    assert list(ids) == [ps[-1][0] for ps in scn.lane_pieces]
    assert np.allclose(pos, [ps[-1][1] + ps[-1][2] for ps in scn.lane_pieces])


def test_small_grid_cut_lane_positions():
    """A cut small_grid lane: the second piece of a 400 m edge continues the SUMO position where the first ends."""
    scn = build_small_grid('greedy')
    l0, l1 = scn.lane_names.index('nt1_nt6_0#0'), scn.lane_names.index('nt1_nt6_0')
    half = float(scn.lane_len[l0])
    ids, pos = scn.sumo_lane_pos([l0, l1, l1], [10.0, 10.0, half])
    assert list(ids) == ['nt1_nt6_0'] * 3
    assert np.allclose(pos, [10.0, half + 10.0, 2 * half])


def test_decode_trace():
    from deeprl_signal_control_amd.env import decode_trace
    scn = build_small_grid('greedy')
    counts = np.zeros(scn.episode_length_sec, np.int32)
    counts[0], counts[2] = 2, 1                                    # seconds 0 and 2 of the episode: time_sec 1 and 3
    lane = scn.lane_names.index('nt1_nt6_0')
    rows = np.zeros((3, 4), np.uint32)
    rows[:, 0] = [lane | 3 << 16, 0 | 7 << 16, lane | 3 << 16]
    rows[:, 1] = [0 | 0 << 16, 0 | 12 << 16, 0 | 0 << 16]
    rows[:, 2] = np.array([1.5, 20.0, 7.25], np.float32).view(np.uint32)
    rows[:, 3] = np.array([0.0, 13.0, 5.5], np.float32).view(np.uint32)
    d = decode_trace(scn, counts, rows)
    assert list(d['time_sec']) == [1, 1, 3]
    assert list(d['id']) == ['f_3.0', 'f_7.12', 'f_3.0']
    assert list(d['lane']) == ['nt1_nt6_0', scn.lane_pieces[0][0][0], 'nt1_nt6_0']
    half = float(scn.lane_len[lane])
    assert np.allclose(d['pos'], [half + 1.5, scn.lane_pieces[0][0][1] + 20.0, half + 7.25])
    assert list(d['speed']) == [0.0, 13.0, 5.5]
    assert list(d['sim_lane']) == [lane, 0, lane] and list(d['route']) == [3, 7, 3] and list(d['serial']) == [0, 12, 0]


@pytest.mark.parametrize('n,ok', [(0, True), (1, True), (2, True), (3, False), (-1, False)])
def test_trajectories_flag(n, ok, tmp_path):
    from deeprl_signal_control_amd import main as cli
    argv = ['--base-dir', str(tmp_path), 'evaluate', '--agents', 'greedy', '--evaluation-seeds', '10000,20000', '--trajectories', str(n)]
    if ok:
        assert cli.parse_args(argv).trajectories == n
    else:
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    assert cli.parse_args(['evaluate']).trajectories == 0
    assert cli.parse_args(['evaluate']).demo is False
