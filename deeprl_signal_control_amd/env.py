"""Host-side env mirror of the reference's TrafficSimulator (envs/env.py:82-635) over the
HIP microsimulator (include/tsc.h, csrc/tsc_env.hip).

* ``VecTrafficEnv`` -- E parallel env instances on one GPU, torch tensors in/out
  (device memory only: no compute happens in torch).
* ``TrafficEnv`` -- E = 1 adaptor with the reference's exact duck-type
  (``reset/step/update_fingerprint/terminate`` and the attributes ``utils.Trainer`` and
  ``main.train`` read), so parity tests read like the reference's own
  scripts (envs/large_grid_env.py:261-286).

There is no CPU path: construction fails if libtsc.so is missing or no GPU is present.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .scenario import ACTUATED_RULES, LANE_CAP, OBJECTIVES, PRESSURE_MEASURES, Scenario, build_scenario

TRACE_ROW_CAP = 1 << 22           # default trajectory rows per traced instance (64 MiB; large_grid's busiest episodes need ~2 M)
FCD_COLUMNS = ('episode', 'time_sec', 'id', 'lane', 'pos', 'speed')
# tsc_env_read_lane_data's integer fields, in its order, under SUMO's laneData attribute names; the lanedata table's columns
LANEDATA_INTS = ('sampledSeconds', 'waitingTime', 'departed', 'arrived', 'entered', 'left', 'laneChangedFrom', 'laneChangedTo',
                 'teleported')
LANEDATA_COLUMNS = ('episode', 'begin', 'end', 'id', 'sampledSeconds', 'density', 'occupancy', 'waitingTime', 'speed', 'traveltime',
                    'departed', 'arrived', 'entered', 'left', 'laneChangedFrom', 'laneChangedTo', 'teleported')
VEHICLE_LENGTH = 5.0              # m (MICROSIM_SPEC.md; kLen of the kernels): SUMO's occupancy counts it


class VecTrafficEnv:
    """E instances of TrafficSimulator.  Seeds follow the reference's bookkeeping
    (envs/env.py:547-560): instance e starts at ``seed + e`` and every ``reset()`` in train
    mode advances its seed by ``seed_stride`` (1 for E = 1, like the reference).

    demand: a scenario.DemandSampler -- every ``reset()`` in train mode then draws each instance's veh/h column from its episode
    seed (set_demand); test mode runs the scenario's own demand unless set_demand is called by hand."""

    def __init__(self, scn: Scenario, n_env: int, device=0, seed=12, test_seeds=(10000, 20000),
                 seed_stride=None, resident=None, demand=None):
        if not torch.cuda.is_available():
            raise RuntimeError('VecTrafficEnv needs a GPU (MI355X); there is no CPU fallback')
        self.scn = scn
        self.E = int(n_env)
        self.device = torch.device('cuda', device) if not isinstance(device, torch.device) else device
        self.agent = scn.agent
        self.A, self.SMAX, self.AMAX = scn.n_agent, scn.s_max, int(scn.green_tab.shape[1])
        self.n_s_ls, self.n_a_ls = list(scn.n_s_ls), list(scn.n_a_ls)
        self.n_w_ls, self.n_f_ls = list(scn.n_w_ls), list(scn.n_f_ls)
        self.n_s, self.n_a = int(np.sum(self.n_s_ls)), int(np.prod(np.array(self.n_a_ls, dtype=object)))
        self.node_names = scn.node_names
        self.T = np.ceil(scn.episode_length_sec / scn.control_interval_sec)      # envs/env.py:89
        self.train_mode = True
        self.test_seeds = list(test_seeds)
        self.test_num = len(self.test_seeds)
        self.seeds = np.array([seed + e for e in range(self.E)], np.int64)
        self.seed_stride = self.E if seed_stride is None else seed_stride
        self.cur_episode = 0
        self.cur_sec = 0
        self.demand_sampler = demand
        self.demand_scale = np.ones(self.E)                   # the scales the sampler drew for the running episode
        self._sampled_demand = False                          # a sampled demand is installed (a test-mode reset takes it out)
        self._draws_routes = scn.stream_mode is not None and bool((np.asarray(scn.stream_mode) == 2).any())
        L = _lib.lib()
        self._L = L
        sc, self._keep = _lib.scenario_struct(scn)
        h = C.c_void_p()
        _lib.check(L.tsc_env_create(C.byref(sc), self.E, self.device.index or 0, C.byref(h)))
        self._h = h
        model = getattr(scn, 'car_following', 'idm')
        if model != 'idm':                  # (IDM handles never call it: they run exactly the kernels they always ran)
            car_following_kw(model, scn.krauss_sigma)
            _lib.check(L.tsc_env_set_car_following(h, CAR_FOLLOWING_MODELS.index(model), float(scn.krauss_sigma)))
        self.reward_pressure = None         # the measure of the armed pressure reward (set_reward_pressure), None = the built-in reward
        if scn.objective == 'pressure':     # (the other objectives never call it: they run exactly what they always ran)
            self.set_reward_pressure(scn.pressure_measure)
        if resident is not None:        # env instances sharing the device with these (other handles / ranks), these included
            _lib.check(L.tsc_env_set_resident_instances(h, int(resident)))
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream(self.device)
            _lib.check(L.tsc_env_set_stream(h, C.c_void_p(self.stream.cuda_stream)))
            d = self.device
            # obs / done ping-pong: step() writes the buffers the previous call did NOT return, so the
            # caller can still hand the previous (ob, done) to model.add_transition (utils.py:160-165)
            self._obs2 = [torch.zeros(self.E, self.A, self.SMAX, dtype=torch.float32, device=d) for _ in range(2)]
            self._done2 = [torch.zeros(self.E, dtype=torch.uint8, device=d) for _ in range(2)]
            self._flip = 0
            self.obs, self.done = self._obs2[0], self._done2[0]
            self.reward = torch.zeros(self.E, self.A, dtype=torch.float64, device=d)
            self.global_reward = torch.zeros(self.E, dtype=torch.float64, device=d)

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            self._L.tsc_env_destroy(self._h)
            self._h = None

    def terminate(self):
        """envs/env.py:563 closes the SUMO connection; the device-resident instances simply stay."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_stream(self, stream):
        self.stream = stream
        _lib.check(self._L.tsc_env_set_stream(self._h, C.c_void_p(stream.cuda_stream)))

    def set_demand(self, vph):
        """Per-instance traffic demand (tsc_env_set_demand): vph int [E, n_flow], the veh/h of flow element f for instance e in
        place of scn.flows[f, 2]; None returns to the scenario's own column.  Takes effect at the next reset() and stays in force
        until changed; a running episode is not touched.  Raises (and changes nothing) on a negative rate or one that makes a
        stream emit more than 255 vehicles in a second."""
        if vph is None:
            _lib.check(self._L.tsc_env_set_demand(self._h, None))
            return
        arr = np.asarray(vph)
        want = (self.E, len(self.scn.flows))
        if arr.shape != want or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError('set_demand: vph must be an integer array of shape [E, n_flow] = %r, got %s %r'
                             % (want, arr.dtype, arr.shape))
        if arr.size and (arr.min() < np.iinfo(np.int32).min or arr.max() > np.iinfo(np.int32).max):
            raise ValueError('set_demand: rates outside the int32 range')
        arr = np.ascontiguousarray(arr, np.int32)
        _lib.check(self._L.tsc_env_set_demand(self._h, arr.ctypes.data_as(C.POINTER(C.c_int32))))

    def demand(self):
        """The veh/h column in force since the last reset(), int32 [E, n_flow] (the scenario's own, repeated, without
        set_demand)."""
        out = np.zeros((self.E, len(self.scn.flows)), np.int32)
        _lib.check(self._L.tsc_env_demand(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def set_record(self, on, trip_cap=8192):
        """init_data(is_record=True) (envs/env.py:517-528): the following steps keep, per simulated second, the network
        statistics of _measure_traffic_step (:409-437), per control step the control log (:581-588) and a log of finished
        trips (:498-515), per env instance.  Uses the recording instantiation of the step kernel (plain lane walk)."""
        if on or getattr(self, '_rec_alloc', False):     # (a refusal -- the recording kernels' LDS need -- leaves the handle as it was)
            _lib.check(self._L.tsc_env_record(self._h, int(bool(on)), int(trip_cap)))
            self._rec_alloc = True
        self.is_record = bool(on)
        self.trip_cap = int(trip_cap)
        if self.is_record:
            K = self.scn.agent_lanes.shape[1]
            self._rec_ints = np.zeros((self.E, 8, 4), np.int64)
            self._rec_speed = np.zeros((self.E, 8), np.float64)
            self._rec_queue = np.zeros((self.E, 8, self.A * K), np.int32)
            self._ild_mask = (np.arange(K)[None, :] < np.asarray(self.scn.agent_nlane)[:, None]).ravel()
            self.traffic_data = [[] for _ in range(self.E)]
            self.control_data = [[] for _ in range(self.E)]
            self.trip_data = [[] for _ in range(self.E)]
            self.teleported_trips = [0] * self.E     # trips of the episode the teleport surrogate truncated (not in trip_data)
            self.truncated_trip_data = [[] for _ in range(self.E)]     # ... their rows (own table, see collect_tripinfo)

    def set_trace(self, instances, row_cap=TRACE_ROW_CAP):
        """Per-vehicle trajectories of the listed instances (SUMO's --fcd-output without coordinates, tsc_env_trace): from the next
        reset() on, every simulated second keeps each live vehicle's lane, position and speed.  Needs set_record(True); an empty
        list detaches the trace.  row_cap: rows kept per instance and episode (16 bytes each; collect_trajectories raises when an
        episode needed more)."""
        instances = [int(e) for e in instances]
        if instances and not getattr(self, 'is_record', False):
            raise ValueError('set_trace: recording is off -- call set_record(True) before set_trace (the trace rides on the '
                             'recording path)')
        if instances and int(row_cap) < 1:
            raise ValueError('set_trace: row_cap = %r must be >= 1' % row_cap)
        arr = np.ascontiguousarray(instances, np.int32)
        _lib.check(self._L.tsc_env_trace(self._h, len(arr), arr.ctypes.data_as(C.POINTER(C.c_int32)), int(row_cap)))
        self.trace_instances, self.trace_cap = instances, int(row_cap)
        self.trajectory_data = {e: None for e in instances}

    def collect_trajectories(self):
        """The traced instances' trajectories of the running episode (set_trace): {instance: dict of columns} with time_sec (the
        traffic table's convention: the end of simulated second t is t + 1), id (the trip table's f_<route>.<serial>), lane and pos
        (the SUMO lane and the position on it, Scenario.sumo_lane_pos) and speed, one row per live vehicle and second, in (second,
        simulator lane, queue position) order; also the simulator's own view of each row: sim_lane, x, route, serial.  Also kept for
        output_data."""
        T = int(self.scn.episode_length_sec)
        counts = np.zeros(T, np.int32)
        out = {}
        for k, e in enumerate(getattr(self, 'trace_instances', [])):
            n = C.c_int32()
            _lib.check(self._L.tsc_env_read_trace(self._h, k, counts.ctypes.data_as(C.POINTER(C.c_int32)), None, 0, C.byref(n)))
            if n.value > self.trace_cap:
                raise RuntimeError('instance %d: the episode needed %d trajectory rows, the trace holds %d: call set_trace(..., '
                                   'row_cap=%d) or larger' % (e, n.value, self.trace_cap, n.value))
            rows = np.zeros((n.value, 4), np.uint32)
            _lib.check(self._L.tsc_env_read_trace(self._h, k, counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(n)))
            out[e] = decode_trace(self.scn, counts, rows)
        self.trajectory_data = out
        return out

    def set_lane_data(self, period):
        """Per-lane traffic statistics of every instance over intervals of `period` seconds (SUMO's laneData / edgeData
        meandata, tsc_env_lane_data): from the next reset() on, the recording walk sums per SUMO lane and interval the sampled
        vehicle-seconds, halting vehicle-seconds, speeds and the departed / arrived / entered / left / lane-changing / teleported
        vehicles.  Needs set_record(True); `period` must be a positive multiple of control_interval_sec, 0
        detaches."""
        period = check_lane_data_period(period, self.scn.control_interval_sec)
        if period and not getattr(self, 'is_record', False):
            raise ValueError('set_lane_data: recording is off -- call set_record(True) before set_lane_data (the lane data rides '
                             'on the recording path)')
        tabs = self.scn.lane_data_slots()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self._L.tsc_env_lane_data(self._h, period, len(tabs['start']), tabs['slot0'].ctypes.data_as(ip),
                                             tabs['start'].ctypes.data_as(fp), tabs['sumo'].ctypes.data_as(ip)))
        self.lane_data_period, self._lane_slots = period, tabs
        self.lane_data = None

    def read_lane_data(self):
        """The raw sums since reset() (set_lane_data): ints int64 [E, n_interval, 9, n_slot] (LANEDATA_INTS order) and speed_sum
        float64 [E, n_interval, n_slot], per slot (a piece of a simulator lane, Scenario.lane_data_slots)."""
        if not getattr(self, 'lane_data_period', 0):
            raise RuntimeError('read_lane_data: no lane data armed (set_lane_data)')
        tabs = self._lane_slots
        n_int = -(-int(self.scn.episode_length_sec) // self.lane_data_period)
        ints = np.zeros((self.E, n_int, len(LANEDATA_INTS), len(tabs['start'])), np.int32)
        speed = np.zeros((self.E, n_int, len(tabs['start'])), np.float64)
        _lib.check(self._L.tsc_env_read_lane_data(self._h, ints.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  speed.ctypes.data_as(C.POINTER(C.c_double))))
        return ints.astype(np.int64), speed

    def collect_lane_data(self):
        """Every instance's lane data of the running episode (set_lane_data), merged onto SUMO lanes: {instance: dict of columns}
        with one row per (interval, SUMO lane), zeros included (merge_lane_data).  Also kept for output_data."""
        if not getattr(self, 'lane_data_period', 0):
            return {}
        ints, speed = self.read_lane_data()
        cols = merge_lane_data(self._lane_slots, self.lane_data_period, int(self.scn.episode_length_sec), ints, speed)
        self.lane_data = {e: {k: v[e] if isinstance(v, np.ndarray) and v.ndim == 2 else v for k, v in cols.items()}
                          for e in range(self.E)}
        return self.lane_data

    def counters(self):
        """Per-instance counters of the running episode: (arrived, teleported), int64 [E] each.  `arrived` is the episode sum
        of simulation.getArrivedNumber (envs/env.py:413); `teleported` counts the heads the teleport surrogate removed after
        --time-to-teleport seconds (envs/env.py:283-284; SUMO would move them on, so they are not arrivals)."""
        arr, tel = np.zeros(self.E, np.uint64), np.zeros(self.E, np.uint64)
        _lib.check(self._L.tsc_env_counters(self._h, arr.ctypes.data_as(C.c_void_p), tel.ctypes.data_as(C.c_void_p)))
        return arr.astype(np.int64), tel.astype(np.int64)

    def _record_step(self, action):
        """Append this control step's rows (reference dict keys; envs/env.py:429-437, :582-587)."""
        vp = C.c_void_p
        _lib.check(self._L.tsc_env_read_record(self._h, self._rec_ints.ctypes.data_as(vp), self._rec_speed.ctypes.data_as(vp),
                                               self._rec_queue.ctypes.data_as(vp)))
        ctrl = self.scn.control_interval_sec
        act = action.cpu().numpy()
        g = self.global_reward.cpu().numpy()
        for e in range(self.E):
            for q in range(ctrl):
                n, dep, arr, wsum = (int(x) for x in self._rec_ints[e, q])
                queues = self._rec_queue[e, q][self._ild_mask]
                self.traffic_data[e].append({'episode': self.cur_episode, 'time_sec': self.cur_sec - ctrl + q + 1,
                                             'number_total_car': n, 'number_departed_car': dep, 'number_arrived_car': arr,
                                             'avg_wait_sec': wsum / n if n > 0 else 0,
                                             'avg_speed_mps': self._rec_speed[e, q] / n if n > 0 else 0,
                                             'std_queue': np.std(queues), 'avg_queue': np.mean(queues)})
            self.control_data[e].append({'episode': self.cur_episode, 'time_sec': self.cur_sec, 'step': self.cur_sec / ctrl,
                                         'action': ','.join(['%d' % a for a in act[e]]), 'reward': g[e]})

    def collect_tripinfo(self):
        """envs/env.py:498-515: the finished trips of the episode just run, in (arrival, route, serial) order; ids are
        f_<route>.<serial within the route>, times formatted like SUMO's tripinfo attributes."""
        buf = np.zeros((8192, 6), np.int32)
        for e in range(self.E):
            cnt = C.c_int32()
            _lib.check(self._L.tsc_env_read_trips(self._h, e, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(cnt)))
            cap = getattr(self, 'trip_cap', len(buf))
            if cnt.value > cap:              # the kernel keeps the first trip_cap trips of an instance and counts the rest
                raise RuntimeError('instance %d finished %d trips, the trip log holds %d: call set_record(True, trip_cap=...) '
                                   'with a larger capacity' % (e, cnt.value, cap))
            if cnt.value > len(buf):
                buf = np.zeros((cnt.value, 6), np.int32)
                _lib.check(self._L.tsc_env_read_trips(self._h, e, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(cnt)))
            tr = buf[:cnt.value]
            # a negative arrival marks a trip the teleport surrogate truncated (include/tsc.h tsc_env_read_trips): SUMO's
            # tripinfo file only lists vehicles that arrived, so the reference's collect_tripinfo never sees such a row
            self.teleported_trips[e] += int((tr[:, 3] < 0).sum())
            # ... but SUMO would have teleported the vehicle on and listed it later with a LONG duration: leaving these rows
            # out drops the worst-delayed trips of the episode, so they are kept apart (a fourth table, *_trip_truncated.csv,
            # with the time in the network and the waiting accumulated up to the removal) -- any trip-time / wait average
            # over the trip table alone is biased low by them
            cut = tr[tr[:, 3] < 0]
            cut = cut[np.lexsort((cut[:, 1], cut[:, 0], -cut[:, 3]))]
            for r, ser, dep, arr, wsec, wcnt in cut:
                self.truncated_trip_data[e].append({'episode': self.cur_episode, 'id': 'f_%d.%d' % (r, ser), 'depart_sec': '%.2f' % dep,
                                                    'removed_sec': '%.2f' % (-arr), 'duration_sec': '%.2f' % (-arr - dep),
                                                    'wait_step': '%d' % wcnt, 'wait_sec': '%.2f' % wsec})
            tr = tr[tr[:, 3] >= 0]
            tr = tr[np.lexsort((tr[:, 1], tr[:, 0], tr[:, 3]))]
            for r, ser, dep, arr, wsec, wcnt in tr:
                self.trip_data[e].append({'episode': self.cur_episode, 'id': 'f_%d.%d' % (r, ser), 'depart_sec': '%.2f' % dep,
                                          'arrival_sec': '%.2f' % arr, 'duration_sec': '%.2f' % (arr - dep),
                                          'wait_step': '%d' % wcnt, 'wait_sec': '%.2f' % wsec})

    def output_data(self, output_path, e=0, name=None):
        """envs/env.py:534-542: <name>_<agent>_{control,traffic,trip}.csv with the reference's columns (pandas'
        alphabetical order, as in real_net_experimental_data/eva_data/)."""
        import pandas as pd
        name = name or self.scn.name
        for kind, rows in (('control', self.control_data[e]), ('traffic', self.traffic_data[e]), ('trip', self.trip_data[e]),
                           ('trip_truncated', self.truncated_trip_data[e])):
            if kind == 'trip_truncated' and not rows:
                continue                                    # the reference's three tables always; the fourth only when it has rows
            df = pd.DataFrame(rows)
            df = df[sorted(df.columns)] if len(df.columns) else df
            df.to_csv(output_path + ('%s_%s_%s.csv' % (name, self.agent, kind)))
        if e in getattr(self, 'trace_instances', []):         # set_trace: the trajectories, <name>_<agent>_fcd.csv
            tr = self.trajectory_data.get(e)
            if tr is None:
                tr = self.collect_trajectories()[e]
            pd.DataFrame(dict(tr, episode=self.cur_episode))[list(FCD_COLUMNS)].to_csv(output_path + ('%s_%s_fcd.csv' % (name, self.agent)))
        if getattr(self, 'lane_data_period', 0):               # set_lane_data: <name>_<agent>_lanedata.csv
            ld = self.lane_data if self.lane_data is not None else self.collect_lane_data()
            lanedata_frame(ld[e], self.cur_episode).to_csv(output_path + ('%s_%s_lanedata.csv' % (name, self.agent)))

    def live_vehicle_mean(self, steps, reset=True):
        """Window mean of the vehicles in the network per env instance over the last `steps` control steps."""
        v = C.c_double()
        _lib.check(self._L.tsc_env_live_sum(self._h, C.byref(v), int(reset)))
        return v.value / max(1, steps * self.E)

    # -- reference API, batched ------------------------------------------------------------
    def reset(self, test_ind=0, obs_out=None):
        """envs/env.py:544-561 -> obs float32 [E, A, SMAX] (written to obs_out if given)."""
        self.obs = self._obs2[self._flip] if obs_out is None else obs_out
        if self.train_mode:
            seeds = self.seeds.copy()
            self.seeds += self.seed_stride                      # `self.seed += 1`, env.py:560
        else:
            # test_ind: one index for every instance (the reference's perform(test_ind)), or one index per
            # instance so that all test seeds are evaluated in one batched episode
            ti = np.broadcast_to(np.asarray(test_ind, np.int64), (self.E,))
            seeds = np.asarray(self.test_seeds, np.int64)[ti]
            self.seeds += self.seed_stride                      # the reference bumps it in test mode too
        s32 = (seeds & 0xFFFFFFFF).astype(np.uint32)
        if self._draws_routes:           # what gen_rou_file(seed) draws per episode (large_grid init_density > 0: the sinks)
            from .scenario import draw_stream_routes
            routes = np.ascontiguousarray(np.stack([draw_stream_routes(self.scn, int(sd)) for sd in seeds]), np.int32)
            _lib.check(self._L.tsc_env_set_stream_routes(self._h, routes.ctypes.data_as(C.POINTER(C.c_int32))))
        if self.demand_sampler is not None:
            if self.train_mode:          # every instance's demand of this episode, from its seed
                draws = [self.demand_sampler.draw(int(sd)) for sd in seeds]
                self.demand_scale = np.array([d[0] for d in draws], np.float64)
                self.set_demand(np.stack([d[1] for d in draws]))
                self._sampled_demand = True
            elif self._sampled_demand:     # test episodes run the nominal demand
                self.demand_scale = np.ones(self.E)
                self.set_demand(None)
                self._sampled_demand = False
        _lib.check(self._L.tsc_env_reset(self._h, s32.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         C.c_void_p(self.obs.data_ptr())))
        self.cur_sec = 0
        self.cur_episode += 1
        self.lane_data = None                                   # (collect_lane_data: the sums start over)
        return self.obs

    def update_fingerprint(self, pi, zero_copy=False):
        """envs/env.py:633-635; pi float32 [E, A, AMAX] on the device.  zero_copy=True lets the env read
        `pi` in place at the next step() (the caller must not overwrite it before that)."""
        assert pi.dtype == torch.float32 and pi.is_contiguous() and tuple(pi.shape) == (self.E, self.A, self.AMAX)
        fn = self._L.tsc_env_bind_fingerprint if zero_copy else self._L.tsc_env_set_fingerprint
        _lib.check(fn(self._h, C.c_void_p(pi.data_ptr())))

    def greedy_actions(self, obs=None, out=None):
        """Controller.forward(obs) of the scenario's greedy controller (envs/large_grid_env.py:45-60,
        envs/real_net_env.py:78-111, envs/small_grid_env.py:40-55) for every instance, on the device (greedy_kernel,
        csrc/tsc_env.hip): obs float32 [E, A, SMAX] (default: the observation the env returned last) -> int32 [E, A]."""
        if not getattr(self, '_greedy_set', False):
            n_cand, term, action = self.scn.greedy_controller_tables()
            ip = C.POINTER(C.c_int32)
            n_cand, term, action = (np.ascontiguousarray(x, np.int32) for x in (n_cand, term, action))
            _lib.check(self._L.tsc_env_set_greedy(self._h, term.shape[1], term.shape[2], n_cand.ctypes.data_as(ip),
                                                  term.ctypes.data_as(ip), action.ctypes.data_as(ip)))
            self._greedy_set = True
        obs = self.obs if obs is None else obs
        assert obs.dtype == torch.float32 and obs.is_contiguous() and tuple(obs.shape) == (self.E, self.A, self.SMAX)
        if out is None:
            out = torch.empty(self.E, self.A, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (self.E, self.A)
        _lib.check(self._L.tsc_env_greedy_actions(self._h, C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def max_pressure_actions(self, out=None, measure='count', min_green=1, return_pressure=False):
        """The max-pressure controller's actions for every instance, from the vehicle state on the device (pressure_kernel,
        csrc/tsc_env.hip; the rule: INTEGRATION.md "Baseline controllers") -> int32 [E, A]; with return_pressure also the phase
        pressures int32 [E, A, AMAX] (padded phases 0).  measure 'count' | 'queue'; min_green >= 1 control steps a chosen phase is
        held at least.  Arms the tables at the first call and again when measure / min_green change (which frees the next
        decision, as reset() does).  ONE CALL PER CONTROL STEP: with min_green > 1 a call advances the hold state."""
        key = (measure, min_green)
        if getattr(self, '_pressure_key', None) != key:
            kw = pressure_kw(measure, min_green)
            tabs = self.scn.pressure_tables()
            ip = C.POINTER(C.c_int32)
            mov, lrm, served = (np.ascontiguousarray(tabs[k], np.int32) for k in ('mov', 'lane_route_mov', 'served'))
            _lib.check(self._L.tsc_env_set_pressure(self._h, PRESSURE_MEASURES.index(kw['pressure_measure']), kw['pressure_min_green'],
                                                    len(mov), mov.ctypes.data_as(ip), lrm.ctypes.data_as(ip), served.shape[2],
                                                    served.ctypes.data_as(ip)))
            self._pressure_key = key
        if out is None:
            out = torch.empty(self.E, self.A, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (self.E, self.A)
        prs = torch.empty(self.E, self.A, self.AMAX, dtype=torch.int32, device=self.device) if return_pressure else None
        _lib.check(self._L.tsc_env_pressure_actions(self._h, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(prs.data_ptr()) if return_pressure else None))
        return (out, prs) if return_pressure else out

    def _actuated(self, rule, key, tables_kw, params, out, return_counts):
        """actuated_actions / sotl_actions: arm (tsc_env_set_actuated) when the rule or a parameter changed, then one call of
        actuated_kernel.  params: (min_green, max_green, theta, mu)."""
        if getattr(self, '_actuated_key', None) != key:
            tabs = self.scn.actuated_tables(rule, **tables_kw)
            ip = C.POINTER(C.c_int32)
            mov, lrm, served = (np.ascontiguousarray(tabs[k], np.int32) for k in ('mov', 'lane_route_mov', 'served'))
            zone = np.ascontiguousarray(tabs['zone'], np.float32)
            _lib.check(self._L.tsc_env_set_actuated(self._h, ACTUATED_RULES.index(rule), *params, zone.ctypes.data_as(C.POINTER(C.c_float)),
                                                    len(mov), mov.ctypes.data_as(ip), lrm.ctypes.data_as(ip), served.shape[2],
                                                    served.ctypes.data_as(ip)))
            self._actuated_key = key
        if out is None:
            out = torch.empty(self.E, self.A, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (self.E, self.A)
        cnt = torch.empty(self.E, self.A, self.AMAX, 2, dtype=torch.int32, device=self.device) if return_counts else None
        _lib.check(self._L.tsc_env_actuated_actions(self._h, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(cnt.data_ptr()) if return_counts else None))
        return (out, cnt) if return_counts else out

    def actuated_actions(self, out=None, min_green=1, max_green=10, gap_sec=3.0, return_counts=False):
        """The gap-based actuated controller's actions (SUMO's `actuated`) for every instance, from the vehicle state on the device
        (actuated_kernel, csrc/tsc_env.hip; the rule: INTEGRATION.md "Baseline controllers") -> int32 [E, A]; with return_counts
        also int32 [E, A, AMAX, 2] = {call, dem} per phase (padded phases 0).  A green is extended while a vehicle is within gap_sec
        seconds (at the lane's speed limit) of the stop line, between min_green and max_green control steps; phases without demand
        are skipped.  The defaults are nominal, not tuned: gap_sec is SUMO's max-gap, max_green 50 s at a 5 s control interval.
        Arms the tables at the first call and again when a parameter changes or sotl_actions ran in between (the handle holds one
        of the two rules), which resets the state as reset() does.  ONE CALL PER CONTROL STEP: a call advances the state."""
        kw = actuated_kw(dict(actuated_min_green=min_green, actuated_max_green=max_green, actuated_gap_sec=gap_sec))
        g, G, gap = kw['actuated_min_green'], kw['actuated_max_green'], kw['actuated_gap_sec']
        return self._actuated('actuated', ('actuated', g, G, gap), dict(gap_sec=gap), (g, G, 0, 0), out, return_counts)

    def sotl_actions(self, out=None, min_green=2, theta=20, mu=2, omega_m=25.0, return_counts=False):
        """The self-organising traffic lights' actions (SOTL: Gershenson 2005, Cools et al. 2008) for every instance, as
        actuated_actions -> int32 [E, A]; with return_counts also int32 [E, A, AMAX, 2] = {call, red} per phase.  A phase is taken
        when the vehicles it kept waiting at red, summed over the control steps, reach theta, unless 1 .. mu vehicles are within
        omega_m metres of the stop line of the green phase.  The defaults are nominal, not tuned: of the order Cools et al. use."""
        kw = actuated_kw(dict(sotl_min_green=min_green, sotl_theta=theta, sotl_mu=mu, sotl_omega=omega_m))
        g, th, m, om = kw['sotl_min_green'], kw['sotl_theta'], kw['sotl_mu'], kw['sotl_omega']
        return self._actuated('sotl', ('sotl', g, th, m, om), dict(omega_m=om), (g, g, th, m), out, return_counts)

    def controller_state(self):
        """The state of the armed actuated / SOTL controller (tsc_env_actuated_state; synchronises): dict of int32 arrays cur [E, A],
        age [E, A] and kappa [E, A, AMAX] (all 0 under the gap rule)."""
        hold = np.zeros((self.E, self.A, 2), np.int32)
        kappa = np.zeros((self.E, self.A, self.AMAX), np.int32)
        ip = C.POINTER(C.c_int32)
        _lib.check(self._L.tsc_env_actuated_state(self._h, hold.ctypes.data_as(ip), kappa.ctypes.data_as(ip)))
        return dict(cur=hold[:, :, 0].copy(), age=hold[:, :, 1].copy(), kappa=kappa)

    def set_reward_pressure(self, measure):
        """The pressure reward (tsc_env_set_reward_pressure, pressure_reward_kernel; the rule: INTEGRATION.md "Pressure reward"):
        measure 'count' | 'queue' arms it -- from the next step() on, reward and global_reward are r[a] = -|P[a]| over the state the step
        left, shaped like the built-in reward, and reward_sum() sums its g from zero; None disarms, back to the scenario's built-in
        objective, whose reward_sum() starts over.  Neither sum spans the change: do not switch mid-episode if the sum matters.
        A scenario with objective = 'pressure' is armed at construction with its pressure_measure.  Independent of
        max_pressure_actions."""
        if measure is None:
            _lib.check(self._L.tsc_env_set_reward_pressure(self._h, -1, 0, None, None))
            self.reward_pressure = None
            return
        kw = pressure_kw(measure)
        tabs = self.scn.pressure_tables()
        ip = C.POINTER(C.c_int32)
        mov, lrm = (np.ascontiguousarray(tabs[k], np.int32) for k in ('mov', 'lane_route_mov'))
        _lib.check(self._L.tsc_env_set_reward_pressure(self._h, PRESSURE_MEASURES.index(kw['pressure_measure']), len(mov),
                                                       mov.ctypes.data_as(ip), lrm.ctypes.data_as(ip)))
        self.reward_pressure = kw['pressure_measure']

    def fixed_time_actions(self, steps_per_phase, out=None):
        """The fixed-time cycle for every instance (fixed_time_kernel): action[e, a] = (t // steps_per_phase) % n_phase[a] with t
        the control steps taken since reset() -> int32 [E, A]."""
        if out is None:
            out = torch.empty(self.E, self.A, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (self.E, self.A)
        _lib.check(self._L.tsc_env_fixed_time_actions(self._h, int(steps_per_phase), C.c_void_p(out.data_ptr())))
        return out

    def reward_sum(self, reset=False):
        """Sum of the global reward over instances and control steps since the accumulator was reset."""
        v = C.c_double()
        _lib.check(self._L.tsc_env_reward_sum(self._h, C.byref(v), int(reset)))
        return v.value

    def step(self, action, obs_out=None, reward_out=None, done_out=None):
        """envs/env.py:566-631; action int32 [E, A] on the device.  Returns the env's own
        output buffers (obs f32 [E,A,SMAX], reward f64 [E,A], done u8 [E], global f64 [E]);
        obs / done alternate between two buffers, reward / global are overwritten by the next call.
        obs_out / reward_out / done_out: write there instead (e.g. the learner's rollout slots, zero copy)."""
        assert action.dtype == torch.int32 and action.is_contiguous() and tuple(action.shape) == (self.E, self.A)
        self._flip ^= 1
        self.obs = self._obs2[self._flip] if obs_out is None else obs_out
        self.done = self._done2[self._flip] if done_out is None else done_out
        reward = self.reward if reward_out is None else reward_out
        _lib.check(self._L.tsc_env_step(self._h, C.c_void_p(action.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                        C.c_void_p(reward.data_ptr()),
                                        C.c_void_p(self.global_reward.data_ptr()),
                                        C.c_void_p(self.done.data_ptr()), int(self.train_mode)))
        self.cur_sec += self.scn.control_interval_sec
        if getattr(self, 'is_record', False):
            self._record_step(action)
        return self.obs, reward, self.done, self.global_reward

    # -- debug / parity ---------------------------------------------------------------------
    def step_plan(self):
        """What step() launches right now (tsc_env_step_plan): the step_kernel instantiation as `row` = (MAXT, HELP, REC, KF, SPEC)
        -- SPEC codes in include/tsc.h -- plus `threads` per workgroup and `lds_bytes`."""
        out = (C.c_int32 * 7)()
        _lib.check(self._L.tsc_env_step_plan(self._h, out))
        return dict(row=tuple(out[:5]), threads=out[5], lds_bytes=out[6])

    def get_state(self, e=0):
        NL, NR = self.scn.n_lane, self.scn.n_stream          # pending / serial are per insertion stream
        out = dict(n=np.zeros(NL, np.int32), x=np.zeros((NL, LANE_CAP), np.float32),
                   v=np.zeros((NL, LANE_CAP), np.float32), sf=np.zeros((NL, LANE_CAP), np.float32),
                   w=np.zeros((NL, LANE_CAP), np.int32), r=np.zeros((NL, LANE_CAP), np.int32),
                   pending=np.zeros(NR, np.int32), serial=np.zeros(NR, np.int32), t=np.zeros(1, np.int32))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self._L.tsc_env_get_state(
            self._h, e, out['n'].ctypes.data_as(ip), out['x'].ctypes.data_as(fp), out['v'].ctypes.data_as(fp),
            out['sf'].ctypes.data_as(fp), out['w'].ctypes.data_as(ip), out['r'].ctypes.data_as(ip),
            out['pending'].ctypes.data_as(ip), out['serial'].ctypes.data_as(ip), out['t'].ctypes.data_as(ip)))
        return out

    def car_following(self):
        """(model, sigma) in force since the last reset(): ('idm', 0.0) or ('krauss', sigma)."""
        m, sg = C.c_int32(), C.c_double()
        _lib.check(self._L.tsc_env_car_following(self._h, C.byref(m), C.byref(sg)))
        return CAR_FOLLOWING_MODELS[m.value], sg.value

    def mean_live_vehicles(self):
        v = C.c_double()
        _lib.check(self._L.tsc_env_live_vehicles(self._h, C.byref(v)))
        return v.value


def decode_trace(scn, counts, rows):
    """tsc_env_read_trace's output -> trajectory columns (VecTrafficEnv.collect_trajectories): counts [T] rows per simulated second,
    rows [n, 4] uint32 {lane | route << 16, depart | serial << 16, x bits, v bits}."""
    rows = np.asarray(rows, np.uint32).reshape(-1, 4)
    counts = np.asarray(counts, np.int64)
    n = len(rows)
    time_sec = np.repeat(np.arange(1, len(counts) + 1), counts)[:n]
    lane, route, serial = rows[:, 0] & 0xFFFF, rows[:, 0] >> 16, rows[:, 1] >> 16
    x, v = rows[:, 2].view(np.float32), rows[:, 3].view(np.float32)
    ids = np.array(['f_%d.%d' % (r, s) for r, s in zip(route.tolist(), serial.tolist())], dtype=object)
    sumo_lane, pos = scn.sumo_lane_pos(lane.astype(np.int64), x.astype(np.float64))
    return dict(time_sec=time_sec, id=ids, lane=sumo_lane, pos=pos, speed=v.astype(np.float64),
                sim_lane=lane.astype(np.int32), x=x, route=route.astype(np.int32), serial=serial.astype(np.int32))


def check_lane_data_period(period, control_interval_sec):
    """A lane-data period in seconds (set_lane_data, evaluate --lane-data): 0 = off, else a positive multiple of the control
    interval, so that one control step never straddles two intervals."""
    p = int(period)
    if p != period or p < 0 or p % int(control_interval_sec):
        raise ValueError('lane data period %r: must be 0 (off) or a positive multiple of the control interval (%d s)'
                         % (period, control_interval_sec))
    return p


def merge_lane_data(tabs, period, episode_sec, ints, speed):
    """Raw per-slot sums (VecTrafficEnv.read_lane_data: ints [E, n_interval, 9, n_slot], speed [E, n_interval, n_slot]) ->
    columns per SUMO lane (tabs: Scenario.lane_data_slots), rows in (interval, SUMO lane) order: begin, end, id, the integer
    columns of LANEDATA_INTS, speed_sum (a SUMO lane's slots added in slot order, i.e. (simulator lane, piece) order, from 0.0) and
    the derived columns of SUMO's laneData: density (vehicles / km), occupancy (%, vehicle length 5 m), speed (m/s) and traveltime
    (s), the last two NaN (an empty field) without samples or at speed 0.  Arrays [E, n_interval * n_sumo_lane]; begin / end / id
    are shared."""
    ints, speed = np.asarray(ints), np.asarray(speed, np.float64)
    E, n_int, _, n_slot = ints.shape
    names, sumo, length = tabs['names'], np.asarray(tabs['sumo']), np.asarray(tabs['length'], np.float64)
    n_sumo = len(names)
    m = np.zeros((n_sumo, n_slot), np.int64)
    m[sumo, np.arange(n_slot)] = 1
    isum = np.einsum('eifs,ns->eifn', ints.astype(np.int64), m)
    # the floats in slot order: a SUMO lane's k-th slot added in round k (a padding column of zeros for the shorter lists)
    order = [np.flatnonzero(sumo == j) for j in range(n_sumo)]
    depth = max(len(o) for o in order)
    pick = np.full((n_sumo, depth), n_slot, np.int64)
    for j, o in enumerate(order):
        pick[j, :len(o)] = o
    sp = np.concatenate([speed, np.zeros((E, n_int, 1))], axis=2)
    ssum = np.zeros((E, n_int, n_sumo))
    for k in range(depth):
        ssum = ssum + sp[:, :, pick[:, k]]
    begin = np.arange(n_int) * period
    end = np.minimum(begin + period, episode_sec)
    P = (end - begin).astype(np.float64)[None, :, None]
    L = length[None, None, :]
    samp = isum[:, :, 0, :].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where((samp > 0) & (ssum > 0), ssum / samp, np.nan)
        ttime = L / mean
    out = dict(begin=np.repeat(begin, n_sumo), end=np.repeat(end, n_sumo),
               id=np.array(list(names) * n_int, dtype=object),
               density=(samp / P / (L / 1000.0)).reshape(E, -1),
               occupancy=(100.0 * samp * VEHICLE_LENGTH / (P * L)).reshape(E, -1),
               speed=mean.reshape(E, -1), traveltime=ttime.reshape(E, -1), speed_sum=ssum.reshape(E, -1))
    for f, k in enumerate(LANEDATA_INTS):
        out[k] = isum[:, :, f, :].reshape(E, -1)
    return out


def lanedata_frame(cols, episode):
    """One instance's lane-data columns (VecTrafficEnv.collect_lane_data) -> the lanedata table (LANEDATA_COLUMNS)."""
    import pandas as pd
    n = len(cols['id'])
    return pd.DataFrame({k: (np.full(n, episode) if k == 'episode' else cols[k]) for k in LANEDATA_COLUMNS})


ENV_CONFIG_KEYS = dict(control_interval_sec=int, yellow_interval_sec=int, episode_length_sec=int, coop_gamma=float,
                       norm_wave=float, norm_wait=float, clip_wave=float, clip_wait=float, coef_wait=float,
                       objective=str, car_following=str, krauss_sigma=float)
DEMAND_CONFIG_KEYS = ('demand_scales', 'demand_jitter')
CAR_FOLLOWING_MODELS = ('idm', 'krauss')                 # include/tsc.h TSC_CF_IDM / TSC_CF_KRAUSS


def car_following_kw(model, sigma=None):
    """[ENV_CONFIG] car_following / krauss_sigma -> Scenario keywords.  A missing model means idm (MICROSIM_SPEC.md rule 3);
    krauss_sigma is SUMO's dawdling sigma in [0, 1] (default 0.5) and only means something under krauss."""
    model = 'idm' if model is None else str(model).strip()
    if model not in CAR_FOLLOWING_MODELS:
        raise ValueError('[ENV_CONFIG] car_following = %r: allowed values are %s' % (model, ' | '.join(CAR_FOLLOWING_MODELS)))
    kw = dict(car_following=model)
    if sigma is not None:
        sigma = float(sigma)
        if model != 'krauss':
            raise ValueError('[ENV_CONFIG] krauss_sigma = %r needs car_following = krauss (the %s model has no dawdling)' % (sigma, model))
        if not 0.0 <= sigma <= 1.0:
            raise ValueError('[ENV_CONFIG] krauss_sigma = %r: must lie in [0, 1]' % sigma)
        kw['krauss_sigma'] = sigma
    return kw


CONTROLLERS = ('greedy', 'maxpressure', 'fixedtime', 'actuated', 'sotl')     # evaluate --agents names that need no learner (main.py)


def pressure_kw(measure=None, min_green=None):
    """[ENV_CONFIG] pressure_measure = count | queue (default count) / pressure_min_green = 1 -> checked values."""
    measure = 'count' if measure is None else str(measure).strip()
    if measure not in PRESSURE_MEASURES:
        raise ValueError('[ENV_CONFIG] pressure_measure = %r: allowed values are %s' % (measure, ' | '.join(PRESSURE_MEASURES)))
    return dict(pressure_measure=measure, pressure_min_green=_positive_int('pressure_min_green', 1 if min_green is None else min_green))


def _positive_int(key, v):
    return _number(key, v, True, 1, False)


def objective_kw(objective=None, measure=None):
    """[ENV_CONFIG] objective = queue | wait | hybrid | pressure -> Scenario keywords; a missing key keeps the scenario's own default.
    Under pressure the measure is pressure_measure = count | queue (default count), the key the max-pressure controller reads, so one
    config trains and evaluates on the same measure."""
    kw = {}
    if objective is not None:
        objective = str(objective).strip()
        if objective not in OBJECTIVES:
            raise ValueError('[ENV_CONFIG] objective = %r: allowed values are %s' % (objective, ' | '.join(OBJECTIVES)))
        kw['objective'] = objective
    if measure is not None:
        kw['pressure_measure'] = pressure_kw(measure)['pressure_measure']
    return kw


def controller_kw(config):
    """The baseline controllers' keys of an [ENV_CONFIG] section (SectionProxy or dict of strings): pressure_measure = count | queue
    (default count), pressure_min_green = 1, fixed_time_steps = 6 (control steps per phase).  Unknown values are refused with the
    allowed ones named."""
    kw = pressure_kw(config.get('pressure_measure'), config.get('pressure_min_green'))
    steps = config.get('fixed_time_steps')
    kw['fixed_time_steps'] = _positive_int('fixed_time_steps', 6 if steps is None else steps)
    return kw


def _number(key, v, integer, least, strict):
    """[ENV_CONFIG] key = v as an int or a finite float, > least (strict) or >= least; refused with the key's name."""
    try:
        x = (int(str(v).strip()) if not isinstance(v, (int, np.integer)) else int(v)) if integer else float(v)
        ok = bool(np.isfinite(x)) and (x > least if strict else x >= least) and (not integer or x <= 1 << 30)   # (int32 on the device)
    except (TypeError, ValueError):
        x, ok = None, False
    if not ok:
        raise ValueError('[ENV_CONFIG] %s = %r: must be %s %s %g' % (key, v, 'an integer' if integer else 'a finite number',
                                                                     '>' if strict else '>=', least))
    return x


def actuated_kw(config):
    """The actuated and SOTL controllers' keys of an [ENV_CONFIG] section (SectionProxy or dict): actuated_min_green = 1,
    actuated_max_green = 10 (control steps), actuated_gap_sec = 3.0; sotl_min_green = 2, sotl_theta = 20 (vehicles x control steps),
    sotl_mu = 2, sotl_omega = 25.0 (metres) -> checked values.  The defaults are nominal, not tuned: the gap is SUMO's max-gap, the
    maximum green 50 s at a 5 s control interval; theta, mu and omega are of the order Cools et al. (2008) use.  Bad values are
    refused with the key's name."""
    def val(key, default, integer, least, strict=False):
        v = config.get(key)
        return _number(key, default if v is None else v, integer, least, strict)
    kw = dict(actuated_min_green=val('actuated_min_green', 1, True, 1), actuated_max_green=val('actuated_max_green', 10, True, 1),
              actuated_gap_sec=val('actuated_gap_sec', 3.0, False, 0, True),
              sotl_min_green=val('sotl_min_green', 2, True, 1), sotl_theta=val('sotl_theta', 20, True, 1),
              sotl_mu=val('sotl_mu', 2, True, 0), sotl_omega=val('sotl_omega', 25.0, False, 0, True))
    if kw['actuated_max_green'] < kw['actuated_min_green']:
        raise ValueError('[ENV_CONFIG] actuated_max_green = %d: must be >= actuated_min_green = %d'
                         % (kw['actuated_max_green'], kw['actuated_min_green']))
    return kw


SCENARIO_KEYS = {'large_grid': dict(peak_flow1=int, peak_flow2=int, init_density=float),
                 'real_net': dict(flow_rate=int), 'small_grid': dict(num_extra_car_per_hour=int)}


def scenario_from_config(config):
    """[ENV_CONFIG] section (configparser SectionProxy or dict of strings, config/config_*.ini) -> (Scenario, seed,
    test_seeds): the keys TrafficSimulator.__init__ and the scenario subclasses read (envs/env.py:83-110,
    envs/large_grid_env.py:64-68, envs/real_net_env.py:115-117, envs/small_grid_env.py:59-61).  `data_path` is
    accepted and ignored: nothing is generated on disk (the demand tables live on the device)."""
    get = config.get
    name, agent = get('scenario'), get('agent')
    kw = {}
    for k, typ in list(ENV_CONFIG_KEYS.items()) + list(SCENARIO_KEYS.get(name, {}).items()):
        v = get(k)
        if v is not None and k not in ('car_following', 'krauss_sigma', 'objective'):
            kw[k] = typ(float(v)) if typ is int else typ(v)
    kw.update(car_following_kw(get('car_following'), get('krauss_sigma')))
    kw.update(objective_kw(get('objective'), get('pressure_measure')))
    seed = int(get('seed'))
    test_seeds = tuple(int(x) for x in str(get('test_seeds')).split(','))
    return build_scenario(name, agent, **kw), seed, test_seeds


def demand_from_config(config, scn):
    """[ENV_CONFIG] demand_scales = 0.6,0.8,1.0,1.2 / demand_jitter = 0.15 -> the scenario.DemandSampler of a training run, or
    None with both keys absent (nothing is built then, and no demand call is ever made).  scales > 0, jitter in [0, 1)."""
    from .scenario import DemandSampler, demand_kw
    kw = demand_kw(config.get('demand_scales'), config.get('demand_jitter'))
    if kw is None:
        return None
    try:
        return DemandSampler(scn, *kw)
    except ValueError as ex:
        raise ValueError('[ENV_CONFIG] demand_scales / demand_jitter: %s' % ex) from None


class NodeView:
    """Read-only stand-in for envs/env.py:63-80 `Node`: what main.init_env hands to the greedy controllers
    (envs/real_net_env.py:78-111 reads lanes_in / ilds_in) and what the evaluation scripts print."""

    def __init__(self, scn, a):
        self.name = scn.node_names[a]
        self.control = False
        self.lanes_in = [scn.lane_names[l] for l in scn.link_lane[a, :scn.agent_nlink[a]]]
        self.ilds_in = [scn.lane_names[l] for l in scn.agent_lanes[a, :scn.agent_nlane[a]]]
        self.neighbor = [scn.node_names[j] for j in scn.neighbors[a]]
        self.n_a = int(scn.n_a_ls[a])
        self.num_state = int(scn.agent_nlane[a])
        self.num_fingerprint = int(scn.n_f_ls[a])
        self.phase_id = scn.extra.get('phase_ids', {}).get(self.name, scn.name)
        self.phases = list(scn.phases[a])


class TrafficEnv:
    """The reference's single-env duck-type (envs/env.py:544-635) on top of VecTrafficEnv(E=1):
    ``reset() -> list[A] of 1-D float arrays``, ``step(list[A] of int) -> (obs, reward ndarray,
    done bool, global_reward float)``.  Observations come back as float32 (the value the
    reference feeds to its nets, agents/policies.py:82,130); rewards stay float64.

    Constructed like the reference's env classes -- ``TrafficEnv(config['ENV_CONFIG'], port=0, output_path='',
    is_record=False, record_stat=False)`` (envs/large_grid_env.py:64-68) -- or from a compiled Scenario."""

    def __init__(self, config, port=0, output_path='', is_record=False, record_stat=False, device=0, seed=None,
                 test_seeds=None):
        if isinstance(config, Scenario):
            scn, cseed, ctest = config, 12, (10000, 20000)
        else:
            scn, cseed, ctest = scenario_from_config(config)
        seed = cseed if seed is None else seed
        test_seeds = ctest if test_seeds is None else test_seeds
        self.vec = VecTrafficEnv(scn, 1, device=device, seed=seed + port, test_seeds=test_seeds, seed_stride=1)
        self.scn = scn
        for k in ('agent', 'n_s_ls', 'n_a_ls', 'n_w_ls', 'n_f_ls', 'n_s', 'n_a', 'node_names', 'T'):
            setattr(self, k, getattr(self.vec, k))
        self.name = scn.name
        self.port = port
        self.nodes = {n: NodeView(scn, a) for a, n in enumerate(scn.node_names)}
        self.init_data(is_record, record_stat, output_path)

    test_num = property(lambda self: self.vec.test_num)
    test_seeds = property(lambda self: self.vec.test_seeds)

    def init_test_seeds(self, test_seeds):
        """envs/env.py:530-532."""
        self.vec.test_seeds = [int(s) for s in test_seeds]
        self.vec.test_num = len(self.vec.test_seeds)

    def init_data(self, is_record, record_stats, output_path):
        """envs/env.py:517-528."""
        self.is_record, self.record_stats, self.output_path = is_record, record_stats, output_path
        self.vec.set_record(bool(is_record))

    traffic_data = property(lambda self: self.vec.traffic_data[0])
    control_data = property(lambda self: self.vec.control_data[0])
    trip_data = property(lambda self: self.vec.trip_data[0])
    truncated_trip_data = property(lambda self: self.vec.truncated_trip_data[0])

    def collect_tripinfo(self):
        """envs/env.py:498-515 (call after the episode, like the reference's evaluation scripts)."""
        self.vec.collect_tripinfo()

    def output_data(self):
        """envs/env.py:534-542."""
        if not self.is_record:
            raise RuntimeError('Env: no record to output!')
        self.vec.output_data(self.output_path, 0, self.name)

    train_mode = property(lambda self: self.vec.train_mode,
                          lambda self, v: setattr(self.vec, 'train_mode', v))
    cur_episode = property(lambda self: self.vec.cur_episode)
    cur_sec = property(lambda self: self.vec.cur_sec)
    seed = property(lambda self: int(self.vec.seeds[0]))

    def _split(self, obs):
        o = obs[0].cpu().numpy()
        return [o[a, :n].copy() for a, n in enumerate(self.scn.obs_len)]

    def reset(self, gui=False, test_ind=0):
        return self._split(self.vec.reset(test_ind=test_ind))

    def update_fingerprint(self, policy):
        pi = np.zeros((1, self.vec.A, self.vec.AMAX), np.float32)
        for a, p in enumerate(policy):
            pi[0, a, :len(p)] = np.asarray(p, np.float32)
        self.vec.update_fingerprint(torch.from_numpy(pi).to(self.vec.device))

    def step(self, action):
        act = torch.tensor([[int(a) for a in action]], dtype=torch.int32, device=self.vec.device)
        obs, reward, done, g = self.vec.step(act)
        r = reward[0].cpu().numpy()
        if self.agent in ('a2c', 'greedy') and self.train_mode:
            r = float(r[0])                                    # scalar for greedy/a2c (envs/env.py:593-594)
        return self._split(obs), r, bool(done[0].item()), float(g[0].item())

    def step_plan(self):
        return self.vec.step_plan()

    def set_reward_pressure(self, measure):
        """VecTrafficEnv.set_reward_pressure: 'count' | 'queue' arms the pressure reward, None returns to the built-in one."""
        self.vec.set_reward_pressure(measure)

    def terminate(self):
        pass

    def close(self):
        self.vec.close()


def make_env(scenario='large_grid', agent='ma2c', n_env=None, **kw):
    """init_env (main.py:51-79) equivalent; n_env=None gives the reference's single-env type.  `scenario` may also be
    the [ENV_CONFIG] section itself (then `agent` and the other keys come from it)."""
    if not isinstance(scenario, str):
        scn, seed, test_seeds = scenario_from_config(scenario)
        kw.setdefault('seed', seed); kw.setdefault('test_seeds', test_seeds)
        return TrafficEnv(scn, **kw) if n_env is None else VecTrafficEnv(scn, n_env, **kw)
    scn_kw = {k: kw.pop(k) for k in list(kw)
              if k in Scenario.__dataclass_fields__ or k in ('peak_flow1', 'peak_flow2', 'sort_lanes')}
    scn = build_scenario(scenario, agent, **scn_kw)
    return TrafficEnv(scn, **kw) if n_env is None else VecTrafficEnv(scn, n_env, **kw)
