"""ctypes binding of oracle/libmicrosim.so (the CPU restatement of the microsim
spec, oracle/microsim.c).  TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, 'libmicrosim.so')
    src = os.path.join(_HERE, 'microsim.c')
    if force or not os.path.exists(so) or (os.path.exists(src) and
                                           os.path.getmtime(src) > os.path.getmtime(so)):
        subprocess.check_call(['make', '-C', _HERE, '-B', 'libmicrosim.so'],
                              stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.ms_create.restype = C.c_void_p
        L.ms_create.argtypes = [C.c_int] * 7 + [fp, fp, ip, ip, ip, ip, ip, ip, ip, ip, ip]
        L.ms_destroy.argtypes = [C.c_void_p]
        L.ms_reset.argtypes = [C.c_void_p, C.c_uint32]
        L.ms_set_links.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
        L.ms_step.argtypes = [C.c_void_p]
        L.ms_run.argtypes = [C.c_void_p, C.c_int]
        L.ms_lane_stats.argtypes = [C.c_void_p, C.c_int, C.c_float, ip, ip, ip]
        L.ms_lane_count.argtypes = [C.c_void_p, C.c_int]
        L.ms_lane_vehicles.argtypes = [C.c_void_p, C.c_int, fp, fp, ip, ip, ip, fp]
        L.ms_time.argtypes = [C.c_void_p]
        L.ms_totals.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.ms_stream_state.argtypes = [C.c_void_p, ip, ip]
        L.ms_check.argtypes = [C.c_void_p]
        L.ms_record.argtypes = [C.c_void_p, C.c_int]
        L.ms_trips.argtypes = [C.c_void_p, ip, C.c_int]
        L.ms_network_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.ms_set_streams.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, ip, fp, fp, ip, ip]
        L.ms_set_stream_routes.argtypes = [C.c_void_p, ip]
        L.ms_set_box.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_double]
        L.ms_box_count.argtypes = [C.c_void_p]
        L.ms_box_count.restype = C.c_int64
        L.ms_set_krauss.argtypes = [C.c_int, C.c_double]
        L.ms_set_lanechange.argtypes = [C.c_void_p, ip, ip, ip, C.c_double, C.c_double]
        L.ms_lanechange_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.ms_set_sibling.argtypes = [C.c_void_p, ip]
        L.ms_set_tables.argtypes = [C.c_void_p, ip, ip]
        _LIB = L
    return _LIB


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _i(a):
    return np.ascontiguousarray(a, np.int32)


class MicroSim:
    """One env instance of the CPU microsim over a compiled Scenario."""

    def __init__(self, scn, cap=None):
        from deeprl_signal_control_amd.scenario import LANE_CAP
        self.scn = scn
        self.cap = cap or LANE_CAP
        L = lib()
        self._keep = [_f(scn.lane_len), _f(scn.lane_vmax), _i(scn.lane_node),
                      _i(scn.lane_up), _i(scn.mv_next), _i(scn.mv_link), _i(scn.mv_yield), _i(scn.mv_prio),
                      _i(scn.mv_zip), _i(scn.route_entry_lane), _i(scn.flows)]
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        ptrs = [a.ctypes.data_as(fp if a.dtype == np.float32 else ip) for a in self._keep]
        self.kmax = int(scn.green_tab.shape[2])
        self.h = L.ms_create(scn.n_lane, scn.n_route, scn.n_agent, self.kmax, self.cap,
                             len(scn.flows), scn.teleport_sec, *ptrs)
        self.L = L
        if getattr(scn, 'lane_sib', None) is not None:          # rule 10 (the compiled tables already name the connection lanes)
            sib = _i(scn.lane_sib)
            self._keep.append(sib)
            L.ms_set_sibling(self.h, sib.ctypes.data_as(ip))
        scn.streams_ready()
        if scn.stream_entry_lane is not None:
            st = [_i(scn.stream_entry_lane), _f(scn.stream_origin), _f(scn.stream_limit), _i(scn.stream_mode), _i(scn.stream_choice)]
            self._keep += st
            L.ms_set_streams(self.h, scn.n_stream, int(scn.stream_choice.shape[1]), int(min(scn.choice_interval_sec, 1 << 30)),
                             int(scn.stream_choice.shape[2]), st[0].ctypes.data_as(ip), st[1].ctypes.data_as(fp),
                             st[2].ctypes.data_as(fp), st[3].ctypes.data_as(ip), st[4].ctypes.data_as(ip))

    def __del__(self):
        if getattr(self, 'h', None):
            self.L.ms_destroy(self.h)
            self.h = None

    def reset(self, seed, stream_routes=None):
        """stream_routes: this episode's routes of the mode-2 streams (scenario.draw_stream_routes), int32 [NS]."""
        if stream_routes is not None:
            r = _i(stream_routes)
            self.L.ms_set_stream_routes(self.h, r.ctypes.data_as(C.POINTER(C.c_int32)))
        self.L.ms_reset(self.h, int(seed) & 0xFFFFFFFF)

    def set_box(self, p):
        """EXPERIMENT (MICROSIM_SPEC.md, not the spec): a head with an open signal and a full target lane stands in the junction
        (with probability p, drawn per vehicle) and blocks its foe links (Scenario.link_foes); 0 switches it off."""
        foes = np.ascontiguousarray(self.scn.link_foes, np.uint32)
        assert foes.shape == (self.scn.n_agent, self.kmax)
        self.L.ms_set_box(self.h, foes.ctypes.data_as(C.POINTER(C.c_uint32)), float(p))

    def set_lanechange(self, gap_front=None, gap_back=2.0):
        """EXPERIMENT (MICROSIM_SPEC.md "lane changing", not the spec; large_grid only): hand-offs enter the lane the junction's
        connection leads to (large_grid/data/build_file.py:107-124: through and right turns lane 0 -> lane 0, a left turn
        from an avenue -> street lane 1) and a vehicle on the wrong lane of a two-lane street must change to its sibling lane
        inside the edge, gaps permitting (gap_front / gap_back metres + 1 s of the closing speed); None switches it off."""
        ip = C.POINTER(C.c_int32)
        if gap_front is None:
            self.L.ms_set_lanechange(self.h, None, None, None, 0.0, 0.0)
            return
        scn = self.scn
        names, NL, NR = scn.lane_names, scn.n_lane, scn.n_route
        idx = {n: i for i, n in enumerate(names)}
        sib = np.full(NL, -1, np.int32)
        for i, n in enumerate(names):
            base, k = n.rsplit('_', 1)
            sib[i] = idx.get(base + '_' + ('1' if k == '0' else '0'), -1)
        mv_next, mv_link = np.asarray(scn.mv_next).reshape(NL, NR), np.asarray(scn.mv_link).reshape(NL, NR)
        entry = mv_next.astype(np.int32).copy()
        feeders = [set(int(u) for u in np.asarray(scn.lane_up).reshape(NL, -1)[l] if u >= 0) for l in range(NL)]
        for l in range(NL):
            for r in range(NR):
                tl = int(mv_next[l, r])
                if tl < 0 or sib[tl] < 0:
                    continue
                left = scn.lane_node[l] >= 0 and mv_link[l, r] >= 0 and mv_link[l, r] % 3 == 2      # links: right, through, left per approach
                want = '1' if left else '0'
                el = tl if names[tl].endswith('_' + want) else int(sib[tl])
                entry[l, r] = el
                feeders[el].add(l)
        up = np.full((NL, 4), -1, np.int32)
        for l in range(NL):
            f = sorted(feeders[l])
            assert len(f) <= 4, (names[l], [names[x] for x in f])
            up[l, :len(f)] = f
        self._lc_keep = [sib, np.ascontiguousarray(entry, np.int32), up]
        self.L.ms_set_lanechange(self.h, sib.ctypes.data_as(ip), self._lc_keep[1].ctypes.data_as(ip), up.ctypes.data_as(ip),
                                 float(gap_front), float(gap_back))

    def set_rule10_from_needed_lane_tables(self):
        """Test hook (tools/sweep_lane_change.py): turn a scenario compiled WITHOUT rule 10 (hand-offs enter the lane the route
        needs) into its rule-10 form -- hand-offs enter the junction connection's lane, siblings feed each other first."""
        ip = C.POINTER(C.c_int32)
        scn = self.scn
        names, NL, NR = scn.lane_names, scn.n_lane, scn.n_route
        idx = {n: i for i, n in enumerate(names)}
        sib = np.full(NL, -1, np.int32)
        for i, n in enumerate(names):
            base, k = n.rsplit('_', 1)
            sib[i] = idx.get(base + '_' + ('1' if k == '0' else '0'), -1)
        mv_next, mv_link = np.asarray(scn.mv_next).reshape(NL, NR), np.asarray(scn.mv_link).reshape(NL, NR)
        entry = mv_next.astype(np.int32).copy()
        feeders = [[] for _ in range(NL)]
        for l in range(NL):
            for r in range(NR):
                tl = int(mv_next[l, r])
                if tl < 0:
                    continue
                el = tl
                if sib[tl] >= 0:
                    left = scn.lane_node[l] >= 0 and mv_link[l, r] >= 0 and mv_link[l, r] % 3 == 2
                    want = '1' if left else '0'
                    el = tl if names[tl].endswith('_' + want) else int(sib[tl])
                entry[l, r] = el
                if l not in feeders[el]:
                    feeders[el].append(l)
        up = np.full((NL, 4), -1, np.int32)
        for l in range(NL):
            f = ([int(sib[l])] if sib[l] >= 0 else []) + sorted(feeders[l])
            assert len(f) <= 4, (names[l], [names[x] for x in f])
            up[l, :len(f)] = f
        self._r10_keep = [sib, np.ascontiguousarray(entry, np.int32), up]
        self.L.ms_set_tables(self.h, self._r10_keep[1].ctypes.data_as(ip), up.ctypes.data_as(ip))
        self.L.ms_set_sibling(self.h, sib.ctypes.data_as(ip))

    def lanechange_counts(self):
        out = (C.c_int64 * 2)()
        self.L.ms_lanechange_counts(self.h, out)
        return dict(changes=out[0], blocked_seconds=out[1])

    def set_links(self, agent, chars):
        if isinstance(chars, str):
            chars = chars.encode()
        self.L.ms_set_links(self.h, agent, bytes(chars), len(chars))

    def step(self, n=1):
        self.L.ms_run(self.h, n)

    def lane_stats(self, lane, det_start=None):
        if det_start is None:
            det_start = float(self.scn.lane_det_start[lane])
        w, h, hw = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.ms_lane_stats(self.h, lane, det_start, C.byref(w), C.byref(h), C.byref(hw))
        return w.value, h.value, hw.value

    def lane_vehicles(self, lane):
        n = self.L.ms_lane_count(self.h, lane)
        x = np.zeros(self.cap, np.float32); v = np.zeros(self.cap, np.float32)
        sf = np.zeros(self.cap, np.float32)
        w = np.zeros(self.cap, np.int32); r = np.zeros(self.cap, np.int32); i = np.zeros(self.cap, np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self.L.ms_lane_vehicles(self.h, lane, x.ctypes.data_as(fp), v.ctypes.data_as(fp),
                                w.ctypes.data_as(ip), r.ctypes.data_as(ip), i.ctypes.data_as(ip),
                                sf.ctypes.data_as(fp))
        return dict(n=n, x=x[:n], v=v[:n], w=w[:n], r=r[:n], id=i[:n], sf=sf[:n])

    def snapshot(self):
        """Dense [NL, CAP] arrays (x, v, sf, w, r) + counts, for state-level parity checks."""
        NL, CAP = self.scn.n_lane, self.cap
        out = dict(n=np.zeros(NL, np.int32), x=np.zeros((NL, CAP), np.float32),
                   v=np.zeros((NL, CAP), np.float32), sf=np.zeros((NL, CAP), np.float32),
                   w=np.zeros((NL, CAP), np.int32), r=np.zeros((NL, CAP), np.int32))
        for l in range(NL):
            d = self.lane_vehicles(l)
            k = d['n']
            out['n'][l] = k
            for key in ('x', 'v', 'sf', 'w', 'r'):
                out[key][l, :k] = d[key]
        return out

    @property
    def time(self):
        return self.L.ms_time(self.h)

    def totals(self):
        out = (C.c_int64 * 8)()
        self.L.ms_totals(self.h, out)
        return dict(live=out[0], departed=out[1], arrived=out[2], sum_trip=out[3], pending=out[4],
                    step_departed=out[5], step_arrived=out[6], teleported=out[7])

    def stream_state(self):
        """(pending, serial) per insertion stream, int32 [NS] each: what VecTrafficEnv.get_state() calls 'pending' and 'serial'."""
        ip = C.POINTER(C.c_int32)
        pend, ser = np.zeros(self.scn.n_stream, np.int32), np.zeros(self.scn.n_stream, np.int32)
        self.L.ms_stream_state(self.h, pend.ctypes.data_as(ip), ser.ctypes.data_as(ip))
        return pend, ser

    def check(self):
        return self.L.ms_check(self.h)

    def record(self, max_trips=16384):
        """Keep a log of finished trips (the tripinfo file of the reference's evaluation runs)."""
        self.L.ms_record(self.h, int(max_trips))
        self._max_trips = int(max_trips)

    def trips(self):
        """[n, 6] int32: route, serial within the route, depart_sec, arrival_sec, waiting seconds, waiting count."""
        buf = np.zeros((getattr(self, '_max_trips', 0), 6), np.int32)
        n = self.L.ms_trips(self.h, buf.ctypes.data_as(C.POINTER(C.c_int32)), len(buf))
        return buf[:min(n, len(buf))]

    def network_stats(self):
        n, w, s = C.c_int64(), C.c_int64(), C.c_double()
        self.L.ms_network_stats(self.h, C.byref(n), C.byref(w), C.byref(s))
        return n.value, w.value, s.value
