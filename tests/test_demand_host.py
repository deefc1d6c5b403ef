"""Per-instance traffic demand, host side (no GPU): the sampler that draws an episode's veh/h column from its seed
(scenario.DemandSampler), the [ENV_CONFIG] keys that configure it and `evaluate --demand-scales`."""
import numpy as np
import pytest

from deeprl_signal_control_amd.scenario import (DemandSampler, build_large_grid, build_real_net, build_scenario, build_small_grid,
                                                demand_kw, draw_stream_routes, permute_lanes)


def test_sampler_is_a_pure_function_of_the_seed():
    scn = build_large_grid('ma2c')
    a, b = DemandSampler(scn, (0.6, 0.8, 1.0, 1.2), 0.15), DemandSampler(scn, (0.6, 0.8, 1.0, 1.2), 0.15)
    draws = [a.draw(s) for s in range(100, 140)]
    for s, (sc, vph) in zip(range(100, 140), draws):
        sc2, vph2 = b.draw(s)
        sc3, vph3 = a.draw(s)                                   # ... not of the draws made before
        assert sc == sc2 == sc3 and sc in (0.6, 0.8, 1.0, 1.2)
        np.testing.assert_array_equal(vph, vph2)
        np.testing.assert_array_equal(vph, vph3)
        assert vph.dtype == np.int32 and vph.shape == (len(scn.flows),) and (vph >= 0).all()
    assert len({d[0] for d in draws}) == 4                      # every scale turns up in 40 episodes
    assert len({d[1].tobytes() for d in draws}) == 40           # and no two seeds share a column
    # jitter: every element within [1 - j, 1 + j] of its scale's column (truncated)
    for sc, vph in draws:
        col = a.column(sc)
        assert (vph <= np.floor(col * 1.15)).all() and (vph >= np.floor(col * 0.85)).all()


@pytest.mark.parametrize('build', [build_large_grid, build_real_net, build_small_grid])
def test_scale_one_without_jitter_is_the_scenario(build):
    scn = build('ma2c')
    s = DemandSampler(scn, (1.0,), 0.0)
    for seed in (0, 12, 99999):
        sc, vph = s.draw(seed)
        assert sc == 1.0
        np.testing.assert_array_equal(vph, scn.flows[:, 2])


@pytest.mark.parametrize('name,keys', [('large_grid', dict(peak_flow1=1100, peak_flow2=925)), ('real_net', dict(flow_rate=325))])
@pytest.mark.parametrize('scale', [0.5, 0.8, 1.2, 2.0])
def test_scale_is_build_scenario_with_scaled_keys(name, keys, scale):
    """The column of scale s is the rate column of the scenario built with the demand keys times s -- truncated after the
    scaling, like the reference generator's %d -- and nothing else of that scenario differs once its lanes are in the base's order."""
    scn = build_scenario(name, 'ma2c')
    want = build_scenario(name, 'ma2c', **{k: v * scale for k, v in keys.items()})
    got = DemandSampler(scn, (scale,)).column(scale)
    np.testing.assert_array_equal(got, want.flows[:, 2])
    np.testing.assert_array_equal(scn.flows[:, [0, 1, 3]], want.flows[:, [0, 1, 3]])
    assert not np.array_equal(got, scn.flows[:, 2])
    if name == 'large_grid':                                    # 1100 * 0.6 * 0.7 = 461.99.. -> 461: truncation, not rounding
        assert int(1100 * 0.6 * 0.7) == 461 and 461 in DemandSampler(scn, (1.0,)).column(1.0) and 462 not in scn.flows[:, 2]
        assert got[0] == int(1100 * scale * 0.6 * 0.4)


def test_small_grid_and_init_density_take_scales():
    scn = build_small_grid('ma2c')
    col = DemandSampler(scn, (2.0,)).column(2.0)
    np.testing.assert_array_equal(col, build_small_grid('ma2c', num_extra_car_per_hour=2000).flows[:, 2])
    scn = build_large_grid('ma2c', init_density=0.2)
    col = DemandSampler(scn, (0.5,)).column(0.5)
    np.testing.assert_array_equal(col, build_large_grid('ma2c', init_density=0.2, peak_flow1=550, peak_flow2=462.5).flows[:, 2])


def test_a_scale_that_changes_other_tables_is_refused():
    """The check that only the rates differ: a base scenario whose tables do not match what the builder gives (here: a lane
    made longer by hand) is refused, naming the table."""
    scn = build_large_grid('ma2c')
    scn.lane_len = scn.lane_len.copy()
    scn.lane_len[3] += 1.0
    with pytest.raises(ValueError, match='lane_len'):
        DemandSampler(scn, (0.8,))
    scn = build_large_grid('ma2c')                               # rates that are not the builder's: scaled columns would not be its multiples
    scn.flows = scn.flows.copy()
    scn.flows[5, 2] += 7
    with pytest.raises(ValueError, match='rates'):
        DemandSampler(scn, (0.8,))
    # ... and the base's lane order is the one that counts: a base in another order passes
    scn = build_large_grid('ma2c')
    scn = permute_lanes(scn, np.random.RandomState(0).permutation(scn.n_lane))
    DemandSampler(scn, (0.8, 1.2))


def test_stream_routes_do_not_move():
    """draw_stream_routes(seed) is what it was, sampler or not: the sampler has a RandomState of its own."""
    scn = build_large_grid('ma2c', init_density=0.2)
    before = [draw_stream_routes(scn, s) for s in range(20, 30)]
    smp = DemandSampler(scn, (0.6, 1.0, 1.4), 0.15)
    state = np.random.get_state()[1].copy()
    for s in range(20, 30):
        smp.draw(s)
        np.testing.assert_array_equal(draw_stream_routes(scn, s), before[s - 20])
    np.testing.assert_array_equal(np.random.get_state()[1], state)         # the global stream is not consumed either
    # and the sink draw of seed s is still RandomState(s).choice: not the sampler's stream
    rs = np.random.RandomState(21)
    m2 = np.nonzero(np.asarray(scn.stream_mode) == 2)[0]
    cand = scn.stream_choice[m2, 0, :, 0]
    K = int((cand[0] >= 0).sum())
    np.testing.assert_array_equal(before[1][m2], cand[np.arange(len(m2)), rs.choice(K, size=len(m2))])


def test_config_keys():
    from deeprl_signal_control_amd.env import demand_from_config, scenario_from_config
    base = dict(scenario='large_grid', agent='ma2c', seed='12', test_seeds='10000,20000')
    scn, _, _ = scenario_from_config(base)
    assert demand_from_config(base, scn) is None                 # both keys absent: nothing is constructed
    s = demand_from_config(dict(base, demand_scales='0.6,0.8,1.0,1.2', demand_jitter='0.15'), scn)
    assert s.scales == (0.6, 0.8, 1.0, 1.2) and s.jitter == 0.15
    s = demand_from_config(dict(base, demand_jitter='0.1'), scn)
    assert s.scales == (1.0,) and s.jitter == 0.1
    s = demand_from_config(dict(base, demand_scales='1.5'), scn)
    assert s.scales == (1.5,) and s.jitter == 0.0
    for bad, word in ((dict(demand_scales='0.8,0'), 'demand_scales'), (dict(demand_scales='-1'), 'demand_scales'),
                      (dict(demand_scales='a,b'), 'demand_scales'), (dict(demand_scales=''), 'demand_scales'),
                      (dict(demand_scales='nan'), 'demand_scales'),
                      (dict(demand_jitter='1.0'), 'demand_jitter'), (dict(demand_jitter='-0.1'), 'demand_jitter'),
                      (dict(demand_jitter='x'), 'demand_jitter')):
        with pytest.raises(ValueError, match=word):
            demand_from_config(dict(base, **bad), scn)
    # the scenario itself does not change with the keys
    scn2, _, _ = scenario_from_config(dict(base, demand_scales='0.6,1.2', demand_jitter='0.15'))
    np.testing.assert_array_equal(scn2.flows, scn.flows)
    assert demand_kw(None, None) is None


def test_evaluate_argument_parsing(capsys):
    from deeprl_signal_control_amd.main import parse_args
    a = parse_args(['evaluate', '--agents', 'greedy'])
    assert a.demand_scales is None
    a = parse_args(['evaluate', '--agents', 'greedy', '--demand-scales', '0.8,1.0,1.2', '--evaluation-seeds', '10000,20000'])
    assert a.demand_scales == [0.8, 1.0, 1.2]
    for bad in ('0', '0.8,-1', 'x', ''):
        with pytest.raises(SystemExit):
            parse_args(['evaluate', '--agents', 'greedy', '--demand-scales', bad])
        assert '--demand-scales' in capsys.readouterr().err
    with pytest.raises(SystemExit):                              # train takes the INI keys, not a flag
        parse_args(['train', '--demand-scales', '0.8'])


def test_eval_tables_get_a_demand_scale_column(tmp_path):
    """write_eval_tables with scales: every table carries the instance's scale; without, the files are what they were."""
    import pandas as pd
    from deeprl_signal_control_amd.main import write_eval_tables

    class Env:
        pass
    env = Env()
    env.scn, env.agent, env.E = type('S', (), {'name': 'large_grid'})(), 'greedy', 2
    env.control_data = [[{'time_sec': 5, 'reward': -1.0}], [{'time_sec': 5, 'reward': -2.0}]]
    env.traffic_data = [[{'time_sec': 1, 'number_total_car': 3}], [{'time_sec': 1, 'number_total_car': 4}]]
    env.trip_data = [[{'id': 'f_0.0', 'duration_sec': '10.00', 'wait_sec': '0.00'}], []]
    env.truncated_trip_data = [[], [{'id': 'f_1.0', 'duration_sec': '700.00', 'wait_sec': '600.00'}]]
    plain, scaled = str(tmp_path / 'a_'), str(tmp_path / 'b_')
    write_eval_tables(env, plain)
    write_eval_tables(env, scaled, [0.8, 1.2])
    for kind in ('control', 'traffic', 'trip', 'trip_truncated'):
        a = pd.read_csv(plain + 'large_grid_greedy_%s.csv' % kind, index_col=0)
        b = pd.read_csv(scaled + 'large_grid_greedy_%s.csv' % kind, index_col=0)
        assert 'demand_scale' not in a.columns and 'demand_scale' in b.columns
        pd.testing.assert_frame_equal(a, b.drop(columns='demand_scale'))
        for _, row in b.iterrows():
            assert row['demand_scale'] == [0.8, 1.2][int(row['episode']) - 1]
