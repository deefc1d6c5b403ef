"""Command line of the reference (main.py:21-48,82-230) on the MI355X path.

    python -m deeprl_signal_control_amd.main --base-dir DIR train --config-dir config/config_ma2c_large.ini
                                                                  [--test-mode no_test|in_train_test|after_train_test|all_test]
                                                                  [--envs E]
    python -m deeprl_signal_control_amd.main --base-dir DIR evaluate --agents ma2c,greedy,maxpressure,fixedtime,actuated,sotl
                                                                  [--evaluation-policy-type default|stochastic|deterministic]
                                                                  [--evaluation-seeds 10000,20000,...]
                                                                  [--trajectories N] [--lane-data PERIOD]
                                                                  [--demand-scales 0.8,1.0,1.2]

Same sub-commands, flags, INI sections ([MODEL_CONFIG] [TRAIN_CONFIG] [ENV_CONFIG], config/config_*.ini of the
reference are read unchanged) and on-disk layout as the reference: ``DIR/{log,data,model}`` with the config copied
into ``data/`` (main.py:84-87), ``data/train_reward.csv`` (utils.py:299-308), ``model/checkpoint-<step>``
(agents/models.py:83-108; an .npz here), and for ``evaluate``: ``DIR/<agent>/{data,model}`` in, ``DIR/eva_data/
<scenario>_<agent>_{control,traffic,trip}.csv`` out (main.py:158-222, utils.py:366-388, envs/env.py:534-542).
``--trajectories N`` also writes ``<scenario>_<agent>_fcd.csv``: every vehicle's SUMO lane, position and speed at every second
(SUMO's --fcd-output without coordinates) for the first N evaluation seeds, with an ``episode`` column.
``--lane-data PERIOD`` also writes ``<scenario>_<agent>_lanedata.csv``: per SUMO lane and PERIOD-second interval, SUMO's laneData
statistics (sampled vehicle-seconds, density, occupancy, waiting time, speed, travel time, vehicle counts) for every evaluation
seed.  PERIOD is a multiple of the control interval; 0 (the default) is off.
``--demand-scales S1,S2,...`` evaluates every seed under every demand scale (the scenario's demand keys times S, as
scenario.DemandSampler builds it) as one batched episode of seeds x scales instances -- episode numbers run over the seeds of the
first scale, then the second ... -- and adds a ``demand_scale`` column to every table.  Training draws its demand per episode from
``[ENV_CONFIG] demand_scales`` / ``demand_jitter``; the evaluation runs the nominal demand without the flag.

``greedy``, ``maxpressure`` (Varaiya 2013), ``fixedtime``, ``actuated`` (SUMO's gap-based actuated control) and ``sotl`` (self-organising
traffic lights, Gershenson 2005) are controllers without a learner: ``DIR/<name>/data/*.ini`` supplies the config ([ENV_CONFIG]
``pressure_measure = count | queue``, ``pressure_min_green = 1``, ``fixed_time_steps = 6``; ``actuated_min_green = 1``,
``actuated_max_green = 10``, ``actuated_gap_sec = 3.0``; ``sotl_min_green = 2``, ``sotl_theta = 20``, ``sotl_mu = 2``, ``sotl_omega = 25.0``
-- nominal values, not tuned), no checkpoint is read, and ``train`` refuses them.

What differs: ``--envs E`` trains on E parallel env instances per GPU (the reference has one); `total_step`,
`test_interval`, `log_interval` keep counting control steps of ONE instance, so a run is E times the experience.
The evaluation runs all evaluation seeds as one batched episode.  TensorBoard summaries and ``--demo`` (SUMO gui) have no
equivalent here.
"""
import argparse
import configparser
import logging
import os
import shutil
import sys
import time

import numpy as np


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--base-dir', type=str, required=False, default='./signal_control_results', help='experiment base dir')
    subparsers = parser.add_subparsers(dest='option', help='train or evaluate')
    sp = subparsers.add_parser('train', help='train a single agent under base dir')
    sp.add_argument('--test-mode', type=str, required=False, default='no_test',
                    choices=['no_test', 'in_train_test', 'after_train_test', 'all_test'], help='test mode during training')
    sp.add_argument('--config-dir', type=str, required=False, default='./config/config_ma2c_large.ini', help='experiment config path')
    sp.add_argument('--envs', type=int, default=1, help='parallel env instances on this GPU (the reference: 1)')
    sp.add_argument('--device', type=int, default=0)
    sp = subparsers.add_parser('evaluate', help='evaluate and compare agents under base dir')
    sp.add_argument('--agents', type=str, required=False, default='naive', help='agent folder names for evaluation, split by ,')
    sp.add_argument('--evaluation-policy-type', type=str, required=False, default='default',
                    help='inference policy type in evaluation: default, stochastic, or deterministic')
    sp.add_argument('--evaluation-seeds', type=str, required=False, default=','.join([str(i) for i in range(10000, 100001, 10000)]),
                    help='random seeds for evaluation, split by ,')
    sp.add_argument('--demo', action='store_true', help='accepted for compatibility (there is no gui)')
    sp.add_argument('--trajectories', type=int, default=0,
                    help='record per-second vehicle trajectories of the first N evaluation seeds (eva_data/<scenario>_<agent>_fcd.csv)')
    sp.add_argument('--lane-data', type=int, default=0, metavar='PERIOD',
                    help='record per-lane statistics over PERIOD-second intervals for every evaluation seed, a multiple of the '
                         'control interval (eva_data/<scenario>_<agent>_lanedata.csv); 0 = off')
    sp.add_argument('--demand-scales', type=str, default=None, metavar='S1,S2,...',
                    help='evaluate every seed under each of these multiples of the scenario\'s demand (one batched episode of seeds '
                         'x scales instances); every table gets a demand_scale column')
    sp.add_argument('--device', type=int, default=0)
    args = parser.parse_args(argv)
    if not args.option:
        parser.print_help()
        sys.exit(1)
    if args.option == 'evaluate':
        n_seeds = len([s for s in args.evaluation_seeds.split(',') if s]) if args.evaluation_seeds else 0
        if not 0 <= args.trajectories <= n_seeds:
            parser.error('--trajectories %d: must lie in [0, %d], the number of evaluation seeds' % (args.trajectories, n_seeds))
        if args.lane_data < 0:
            parser.error('--lane-data %d: must be 0 (off) or a positive multiple of the control interval' % args.lane_data)
        if args.demand_scales is not None:
            from .scenario import demand_kw
            try:
                args.demand_scales = list(demand_kw(args.demand_scales)[0])
            except ValueError as ex:
                parser.error('--%s' % str(ex).replace('_', '-', 1))
    return args


# ---- utils.py:19-67 ---------------------------------------------------------------------------------------------
def init_dir(base_dir, pathes=('log', 'data', 'model')):
    os.makedirs(base_dir, exist_ok=True)
    dirs = {}
    for path in pathes:
        cur = base_dir + '/%s/' % path
        os.makedirs(cur, exist_ok=True)
        dirs[path] = cur
    return dirs


def init_log(log_dir):
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', level=logging.INFO, force=True,
                        handlers=[logging.FileHandler('%s/%d.log' % (log_dir, time.time())), logging.StreamHandler()])


def init_test_flag(test_mode):
    return {'no_test': (False, False), 'in_train_test': (True, False), 'after_train_test': (False, True),
            'all_test': (True, True)}[test_mode]


def find_file(cur_dir, suffix='.ini'):
    for f in sorted(os.listdir(cur_dir)):
        if f.endswith(suffix):
            return cur_dir + '/' + f
    logging.error('Cannot find %s file' % suffix)
    return None


class GreedyPolicy:
    """LargeGridController / RealNetController / SmallGridController (envs/*_env.py) on the device obs tensor: the env's
    greedy kernel (VecTrafficEnv.greedy_actions -> tsc_env_greedy_actions) over the scenario's controller tables."""
    name = 'greedy'
    n_step = 1

    def __init__(self, env):
        self.env = env

    def forward(self, ob, *_a, **_k):
        return self.env.greedy_actions(ob)

    def reset(self):
        pass


class MaxPressurePolicy:
    """The max-pressure controller (Varaiya 2013) on the device's vehicle state: VecTrafficEnv.max_pressure_actions ->
    tsc_env_pressure_actions; [ENV_CONFIG] pressure_measure / pressure_min_green.  The observation is not read."""
    name = 'maxpressure'
    n_step = 1

    def __init__(self, env, measure='count', min_green=1):
        self.env, self.measure, self.min_green = env, measure, min_green

    def forward(self, ob, *_a, **_k):
        return self.env.max_pressure_actions(measure=self.measure, min_green=self.min_green)

    def reset(self):
        pass


class FixedTimePolicy:
    """A fixed-time cycle, [ENV_CONFIG] fixed_time_steps control steps per phase: VecTrafficEnv.fixed_time_actions ->
    tsc_env_fixed_time_actions."""
    name = 'fixedtime'
    n_step = 1

    def __init__(self, env, steps_per_phase=6):
        self.env, self.steps = env, steps_per_phase

    def forward(self, ob, *_a, **_k):
        return self.env.fixed_time_actions(self.steps)

    def reset(self):
        pass


class ActuatedPolicy:
    """Gap-based actuated control (SUMO's `actuated`) on the device's vehicle state: VecTrafficEnv.actuated_actions ->
    tsc_env_actuated_actions; [ENV_CONFIG] actuated_min_green / actuated_max_green / actuated_gap_sec.  The observation is not read."""
    name = 'actuated'
    n_step = 1

    def __init__(self, env, min_green=1, max_green=10, gap_sec=3.0):
        self.env, self.min_green, self.max_green, self.gap_sec = env, min_green, max_green, gap_sec

    def forward(self, ob, *_a, **_k):
        return self.env.actuated_actions(min_green=self.min_green, max_green=self.max_green, gap_sec=self.gap_sec)

    def reset(self):
        pass


class SotlPolicy:
    """Self-organising traffic lights (Gershenson 2005; Cools et al. 2008) on the device's vehicle state:
    VecTrafficEnv.sotl_actions -> tsc_env_actuated_actions; [ENV_CONFIG] sotl_min_green / sotl_theta / sotl_mu / sotl_omega."""
    name = 'sotl'
    n_step = 1

    def __init__(self, env, min_green=2, theta=20, mu=2, omega_m=25.0):
        self.env, self.min_green, self.theta, self.mu, self.omega_m = env, min_green, theta, mu, omega_m

    def forward(self, ob, *_a, **_k):
        return self.env.sotl_actions(min_green=self.min_green, theta=self.theta, mu=self.mu, omega_m=self.omega_m)

    def reset(self):
        pass


A2C_POLICIES = ('lstm', 'fc')


def a2c_policy(model_config):
    """[MODEL_CONFIG] policy = lstm | fc: the actor-critic net of IA2C / MA2C.  The key is the one the reference's
    config/config_greedy_large.ini:13 carries (and nothing there reads); absent means lstm, the policy the reference's
    agents/models.py builds.  fc is the feed-forward FcACPolicy (agents/policies.py:214-256), for MA2C its fingerprint
    variant FPFcACPolicy (agents/policies.py:259-282)."""
    policy = model_config.get('policy', 'lstm').strip()
    if policy not in A2C_POLICIES:
        raise ValueError('[MODEL_CONFIG] policy = %r: allowed values are %s' % (policy, ' | '.join(A2C_POLICIES)))
    return policy


def init_model(env, config, total_step, n_env, seed, device=0):
    """main.py:102-118: the learner for env.agent (IA2C / MA2C with the [MODEL_CONFIG] policy, a2c_policy)."""
    from .agents import VecA2C
    from .iql import VecIQL
    a_max = int(env.scn.green_tab.shape[1])
    if env.agent in ('ia2c', 'ma2c'):
        return VecA2C(env.n_s_ls, env.n_a_ls, env.n_w_ls, env.n_f_ls, n_env, env.scn.s_max, a_max, config['MODEL_CONFIG'],
                      total_step, device=device, seed=seed, name=env.agent, policy=a2c_policy(config['MODEL_CONFIG']))
    if env.agent in ('iqld', 'iqll'):
        return VecIQL(env.n_s_ls, env.n_a_ls, env.n_w_ls, n_env, env.scn.s_max, a_max, config['MODEL_CONFIG'], total_step,
                      device=device, seed=0, model_type='dqn' if env.agent == 'iqld' else 'lr')
    raise ValueError('agent %r has no learner (main.py:102-118 knows ia2c, ma2c, iqld, iqll)' % env.agent)


def car_following_label(scn):
    return 'krauss (sigma %g)' % scn.krauss_sigma if scn.car_following == 'krauss' else scn.car_following


def train(args):
    """main.py:82-155 + utils.py:255-308 (Trainer.run)."""
    from .env import VecTrafficEnv, demand_from_config, scenario_from_config
    from .trainer import Counter, VecTrainer
    dirs = init_dir(args.base_dir)
    init_log(dirs['log'])
    shutil.copy(args.config_dir, dirs['data'])
    config = configparser.ConfigParser()
    config.read(args.config_dir)
    in_test, post_test = init_test_flag(args.test_mode)
    from .env import CONTROLLERS
    if config['ENV_CONFIG'].get('agent') in CONTROLLERS:          # (before any work on the device)
        raise ValueError('agent %r has no learner to train (main.py:102-118 knows ia2c, ma2c, iqld, iqll); evaluate it with '
                         '`evaluate --agents %s`' % (config['ENV_CONFIG'].get('agent'), config['ENV_CONFIG'].get('agent')))
    scn, seed, test_seeds = scenario_from_config(config['ENV_CONFIG'])
    sampler = demand_from_config(config['ENV_CONFIG'], scn)
    env = VecTrafficEnv(scn, args.envs, device=args.device, seed=seed, test_seeds=test_seeds, demand=sampler)
    logging.info('Training: car following %s' % car_following_label(scn))
    if sampler is not None:
        logging.info('Training: per-instance demand, %s' % sampler.describe())
    logging.info('Training: s dim: %d, a dim %d, s dim ls: %r, a dim ls: %r' % (env.n_s, env.n_a, env.n_s_ls, env.n_a_ls))
    total_step = int(config.getfloat('TRAIN_CONFIG', 'total_step'))
    test_step = int(config.getfloat('TRAIN_CONFIG', 'test_interval'))
    log_step = int(config.getfloat('TRAIN_CONFIG', 'log_interval'))
    counter = Counter(total_step, test_step, log_step)
    model = init_model(env, config, total_step, args.envs, seed, args.device)
    if getattr(model, 'prioritized_replay', 0):
        logging.info('Training: prioritized replay, alpha %g, beta %g -> 1, eps %g' % (model.per_alpha, model.per_beta, model.per_eps))
    if getattr(model, 'dueling', 0):
        logging.info('Training: dueling head, Q = V + A - mean(A)')
    if getattr(model, 'return_steps', 1) > 1:
        logging.info('Training: %d-step returns' % model.return_steps)
    if getattr(model, 'share', None) is not None:
        sizes = model.share_sizes()
        logging.info('Training: parameter sharing, %d agents in %d classes of %s members'
                     % (model.n_agent, len(sizes), ' + '.join(str(n) for n in sizes)))
    trainer = VecTrainer(env, model, counter, log_rewards=True)
    data = trainer.run_training(run_test=in_test, output_path=dirs['data'])
    if post_test:                                               # Tester.run_offline (utils.py:324-338)
        rows = trainer.evaluate('default', step=counter.cur_step)
        data += rows
        logging.info('Offline testing: avg R: %.2f' % np.mean([r['avg_reward'] for r in rows]))
    write_reward_csv(data, dirs['data'] + 'train_reward.csv')
    logging.info('Training: save final model at step %d ...' % counter.cur_step)
    model.save(dirs['model'], counter.cur_step)
    env.close(); model.close()
    return data


def write_reward_csv(rows, path):
    """utils.py:307-308: pd.DataFrame(self.data).to_csv(...) (columns in pandas' alphabetical order of that era)."""
    import pandas as pd
    df = pd.DataFrame(rows)
    if len(df.columns):
        df = df[sorted(df.columns)]
    df.to_csv(path)


def evaluate_agent(agent_dir, output_dir, seeds, policy_type='default', device=0, trajectories=0, lane_data=0, demand_scales=None):
    """main.py:158-198 + Evaluator.run (utils.py:366-388): all evaluation seeds as ONE batched, recorded episode.  demand_scales:
    every seed under each of these demand scales (instance k * len(seeds) + i runs seed i at scale k); the tables then carry a
    demand_scale column."""
    from .env import CONTROLLERS, VecTrafficEnv, actuated_kw, check_lane_data_period, controller_kw, scenario_from_config
    from .trainer import VecTrainer
    agent = agent_dir.rstrip('/').split('/')[-1]
    if not os.path.isdir(agent_dir):
        logging.error('Evaluation: %s does not exist!' % agent)
        return None
    config_dir = find_file(agent_dir + '/data/')
    if not config_dir:
        return None
    config = configparser.ConfigParser()
    config.read(config_dir)
    if agent in CONTROLLERS:                  # the controllers share the greedy observation layout (none but greedy reads it)
        config['ENV_CONFIG']['agent'] = 'greedy'
        ctl = controller_kw(config['ENV_CONFIG']) if agent != 'greedy' else {}   # (refusals before any work on the device)
        if agent in ('actuated', 'sotl'):
            ctl = actuated_kw(config['ENV_CONFIG'])
    scn, seed, _ = scenario_from_config(config['ENV_CONFIG'])
    lane_data = check_lane_data_period(lane_data, scn.control_interval_sec)     # (before any work on the device)
    n_seed = len(seeds)
    scale_of = None
    if demand_scales:
        from .scenario import DemandSampler
        sampler = DemandSampler(scn, demand_scales)
        scale_of = [float(s_) for s_ in demand_scales for _ in seeds]
        seeds = list(seeds) * len(demand_scales)
    E = len(seeds)
    env = VecTrafficEnv(scn, E, device=device, seed=seed, test_seeds=seeds)
    env.agent = agent if agent in CONTROLLERS else env.agent                     # every table is named and labelled with it
    if scale_of is not None:
        env.set_demand(np.stack([sampler.column(s_) for s_ in scale_of]))
        logging.info('Evaluation: demand scales %s x %d seeds' % (','.join('%g' % s_ for s_ in demand_scales), n_seed))
    logging.info('Evaluation: car following %s' % car_following_label(scn))
    logging.info('Evaluation: s dim: %d, a dim %d, s dim ls: %r, a dim ls: %r' % (env.n_s, env.n_a, env.n_s_ls, env.n_a_ls))
    if agent == 'maxpressure':
        model = MaxPressurePolicy(env, ctl['pressure_measure'], ctl['pressure_min_green'])
        logging.info('Evaluation: max-pressure, measure %s, min green %d control steps' % (model.measure, model.min_green))
    elif agent == 'fixedtime':
        model = FixedTimePolicy(env, ctl['fixed_time_steps'])
        logging.info('Evaluation: fixed-time, %d control steps per phase' % model.steps)
    elif agent == 'actuated':
        model = ActuatedPolicy(env, ctl['actuated_min_green'], ctl['actuated_max_green'], ctl['actuated_gap_sec'])
        logging.info('Evaluation: actuated, green %d to %d control steps, gap %g s' % (model.min_green, model.max_green, model.gap_sec))
    elif agent == 'sotl':
        model = SotlPolicy(env, ctl['sotl_min_green'], ctl['sotl_theta'], ctl['sotl_mu'], ctl['sotl_omega'])
        logging.info('Evaluation: SOTL, min green %d control steps, theta %d, mu %d, omega %g m'
                     % (model.min_green, model.theta, model.mu, model.omega_m))
    elif agent != 'greedy':
        model = init_model(env, config, 0, E, seed, device)
        if not model.load(agent_dir + '/model/'):
            logging.error('Evaluation: no checkpoint under %s/model/' % agent_dir)
            return None
    else:
        model = GreedyPolicy(env)
    env.train_mode = False
    env.set_record(True)
    if trajectories:                 # the first N seeds, under every scale
        env.set_trace([k * n_seed + i for k in range(E // max(n_seed, 1)) for i in range(trajectories)])
    if lane_data:
        env.set_lane_data(lane_data)
    trainer = VecTrainer(env, model)
    mean, std = trainer.perform(np.arange(E), policy_type)
    env.collect_tripinfo()
    if trajectories:
        env.collect_trajectories()
    if lane_data:
        env.collect_lane_data()
    for e in range(E):
        logging.info('test %i, avg reward %.2f' % (e, mean[e]))
    write_eval_tables(env, output_dir, scale_of)
    env.close()
    if hasattr(model, 'close'):
        model.close()
    return mean, std


def write_eval_tables(env, output_dir, scale_of=None):
    """envs/env.py:534-542 over all evaluated instances: instance e is episode e + 1 (the reference runs the seeds one
    after the other and numbers them by cur_episode).  scale_of: the demand scale of every instance (evaluate --demand-scales), a
    demand_scale column of every table."""
    import pandas as pd

    def scaled(cols, e):
        return cols if scale_of is None else dict(cols, demand_scale=scale_of[e])
    for kind, per_env in (('control', env.control_data), ('traffic', env.traffic_data), ('trip', env.trip_data),
                          ('trip_truncated', getattr(env, 'truncated_trip_data', []))):
        rows = []
        for e, rs in enumerate(per_env):
            rows += [scaled(dict(r, episode=e + 1), e) for r in rs]
        if kind == 'trip_truncated':
            if not rows:
                continue
            # trips the teleport surrogate cut short (MICROSIM_SPEC.md rule 1): not in the trip table (SUMO's tripinfo would list them
            # later, with long durations), so averages over the trip table alone are biased low -- say so where it is read
            logging.info('Evaluation: %d trips truncated by the teleport surrogate (mean %.1f s in the network, %.1f s waiting) are in '
                         '%s_%s_trip_truncated.csv, not in the trip table' % (
                             len(rows), np.mean([float(r['duration_sec']) for r in rows]), np.mean([float(r['wait_sec']) for r in rows]),
                             env.scn.name, env.agent))
        df = pd.DataFrame(rows)
        if len(df.columns):
            df = df[sorted(df.columns)]
        df.to_csv(output_dir + ('%s_%s_%s.csv' % (env.scn.name, env.agent, kind)))
    if getattr(env, 'trace_instances', None):               # --trajectories: instance e is episode e + 1 here too
        from .env import FCD_COLUMNS
        df = pd.concat([pd.DataFrame(scaled(dict(env.trajectory_data[e], episode=e + 1), e)) for e in env.trace_instances], ignore_index=True)
        df[list(FCD_COLUMNS) + ['demand_scale'] * (scale_of is not None)].to_csv(output_dir + ('%s_%s_fcd.csv' % (env.scn.name, env.agent)))
    if getattr(env, 'lane_data', None):                     # --lane-data: every instance, episode e + 1
        from .env import lanedata_frame
        df = pd.concat([lanedata_frame(env.lane_data[e], e + 1) if scale_of is None else
                        lanedata_frame(env.lane_data[e], e + 1).assign(demand_scale=scale_of[e]) for e in range(env.E)], ignore_index=True)
        df.to_csv(output_dir + ('%s_%s_lanedata.csv' % (env.scn.name, env.agent)))


def evaluate(args):
    """main.py:201-222 (agents one after the other instead of one thread + SUMO port each)."""
    dirs = init_dir(args.base_dir, pathes=['eva_data', 'eva_log'])
    init_log(dirs['eva_log'])
    seeds = [int(s) for s in args.evaluation_seeds.split(',')] if args.evaluation_seeds else []
    logging.info('Evaluation: policy type: %s, random seeds: %s' % (args.evaluation_policy_type, seeds))
    out = {}
    for agent in args.agents.split(','):
        out[agent] = evaluate_agent(args.base_dir + '/' + agent, dirs['eva_data'], seeds, args.evaluation_policy_type, args.device,
                                    getattr(args, 'trajectories', 0), getattr(args, 'lane_data', 0), getattr(args, 'demand_scales', None))
    return out


def main(argv=None):
    args = parse_args(argv)
    return train(args) if args.option == 'train' else evaluate(args)


if __name__ == '__main__':
    main()
