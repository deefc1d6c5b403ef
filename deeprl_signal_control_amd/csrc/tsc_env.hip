// tsc_env.hip -- batched traffic microsimulator + reference env semantics on gfx950.
//
// Replaces, for E parallel env instances, the reference's TrafficSimulator.step/reset
// (envs/env.py:544-631) *including* the SUMO process behind its TraCI socket:
//   K1 signal FSM ............ envs/env.py:128-152,455-459 (tables from scenario.py)
//   K2 vehicle update ........ MICROSIM_SPEC.md (IDM + safe-speed clamp, lane queues)
//   K3 hand-off / insertion .. MICROSIM_SPEC.md (feeder gather, vehsPerHour flows)
//   K4 detectors ............. envs/env.py:325-407 (wave / halting / head-vehicle wait)
//   K5 observation gather .... envs/env.py:163-205,439-442 (float64 arithmetic, cast to f32)
//   K6 reward + shaping ...... envs/env.py:356-367,580,590-631 (float64, numpy sum order)
//
// Mapping: one workgroup per env instance: one thread per lane that a route can ever put a vehicle on (a
// prefix after load sorting, padded to a multiple of 64 = NLA) plus helper threads up to 256.  Vehicles live
// in HBM as one 16-byte record per slot {x, v, desired-speed factor, bits of (wait | route << 16)}, lane-major: S[E][NLP][CAP]
// (vslot) -- a lane's queue is contiguous, front first, so the flat phase (consecutive threads own consecutive queued vehicles
// of a lane; it is most of the kernel) reads and writes runs of up to 27 x 16 bytes with one load / one store per vehicle.
// Until round 5 the state was four slot-major arrays X / V / SF / M [CAP][NLP], coalesced for the lane threads' head walk
// instead: every flat-phase access instruction touched 64 cache lines (92.7 -> 86.3 us per control step at E = 1024 over
// whole episodes with lane-major arrays, -> 81.1 us with the records; PMC traffic per launch 159 -> 57 MB).
// Everything lanes need from *other* lanes
// (tail/head summaries, signal states, the per-step hand-off outbox, the route tables) is staged in LDS; one
// control step (2 yellow + 3 green simulated seconds, detectors, obs, reward) is a single launch.  Per
// simulated second: phase H (lane threads: the platoon that crosses and the first vehicle that stays), phase F (all
// threads: every other queued vehicle in a flat, load-balanced order -- car-following from the old state, the queue
// constraint as a segmented prefix-min scan on the wavefront's DPP path; its first half runs on the helper wavefronts
// WHILE the lane wavefronts are in phase H), phase B (gather + demand) (see step_kernel).
//
// Which kernel runs.  step_kernel<MAXT, HELP, REC, KF, SPEC> has one instantiation per row of kStepVariants (MAXT: workgroup
// bound; HELP: flat phase; REC: recording walk; KF: flat-phase vehicles per thread; SPEC: 0 runtime table dimensions, 1 / 2
// large_grid's / Monaco's as compile-time constants (kSpec), < 0 the kSpec* sentinels).  plan_step turns the handle's state into
// a row, a workgroup size and an LDS size (StepPlan; tsc_env_step_plan reports it) whenever an input changes -- create, record,
// trace, lane_data, set_resident_instances, reset -- and tsc_env_step only launches the plan.  The rules, first match wins:
//   recording on ........ <256 | 1024, false, true, 4 (Krauss: 1), S>: S = lane data (live from the reset after arming), else
//                         trace (from the call that attaches it), else none; IDM 0 / -2 / -4, Krauss -1 / -3 / -5
//   Krauss .............. <256 | 1024, HELP, false, KF, -1>: KF = TSC_ENV_KF only up to 256 threads with the flat phase, else 1
//   IDM, spec ........... <threads, true, false, kf, spec> when the scenario matches a kSpec row (not with TSC_ENV_SPEC=0 or
//                         kf 4), the flat phase is on, kf is 1 or 2 and threads is 256, 512 or 1024
//   IDM, runtime dims ... <256, true, false, kf, 0> up to 256 threads with the flat phase and kf 1 or 2; otherwise
//                         <256 | 1024, HELP, false, 4, 0>: every wider workgroup runs the 4-wide flat phase whatever kf says
// 256 | 1024 is by threads <= 256.  Threads: 256 with the flat phase when the live lanes fit (else NLA, the live lanes rounded
// up to 64; TSC_ENV_HELP=0: NLA); a spec handle follows the device's load (pick_workgroup: 1024 threads and kf 1 up to one instance
// per CU, 512 and kf 2 up to two, else 256 and kf 2 on large_grid / 1 on Monaco; tsc_env_set_resident_instances); a Krauss handle
// does not.  TSC_ENV_THREADS (a multiple of 64 in [NLA, 1024]) and TSC_ENV_KF (1 | 2 | 4) override either.  The recording rows keep
// that workgroup size.  Krauss is in force from the reset after tsc_env_set_car_following.  LDS is smem_bytes<KR, LD> of the
// handle's tables (at most kLdsMax); a setter whose effect waits for the reset checks the size it will need when it is called.
//
// Arithmetic is fp32 with one rounding per operation (-ffp-contract=off, IEEE div/sqrt) so the
// vehicle state is bit-identical to the CPU oracle; obs/reward are computed in float64 exactly
// like the reference's NumPy code.
#include "tsc_common.h"
#include "../../include/tsc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

constexpr float kLen = 5.0f, kS0 = 2.0f /* standstill gap (SUMO minGap 2.5 less the storage of its junction interiors, MICROSIM_SPEC.md) */,
                kAcc = 5.0f, kDec = 10.0f, kTHead = 1.0f;   // headway = SUMO's default tau
constexpr float kICab = 0.070710678f /* 1 / (2 sqrt(acc dec)): a multiply instead of an IEEE division */, kHalt = 0.1f, kYieldT = 3.0f, kYieldD = 10.0f;
constexpr int kCap = TSC_LANE_CAP, kMaxCross = TSC_MAX_CROSS, kMaxUp = TSC_MAX_UP;
// Element index of slot i of lane q in an instance's vehicle arrays X / V / SF / M (and R0 / R1).
#ifndef TSC_LANE_MAJOR
#define TSC_LANE_MAJOR 1
#endif
__host__ __device__ __forceinline__ int vslot(int i, int q, int NLP) { return TSC_LANE_MAJOR ? q * kCap + i : i * NLP + q; }

constexpr int kMaxEntry = 8;           // routes that may share one entry lane (small_grid: 6 paths leave np1_nt1)
// movement word of (lane, route):  [11:0] next lane (0xFFF = route ends here, 0xFFE = n/a)
//   [17:12] signal link (63 = none)   [29:18] lane this movement yields to (0xFFF = none)   [30] priority movement
__host__ __device__ __forceinline__ int mv_tl(int w) { const int t = w & 0xFFF; return t == 0xFFF ? -1 : t == 0xFFE ? -2 : t; }
__host__ __device__ __forceinline__ int mv_k(int w) { const int k = (w >> 12) & 0x3F; return k == 63 ? -1 : k; }
__host__ __device__ __forceinline__ int mv_yield(int w) { const int y = (w >> 18) & 0xFFF; return y == 0xFFF ? -1 : y; }
__host__ __device__ __forceinline__ bool mv_prio(int w) { return (w >> 30) & 1; }

// Trace fields (tsc_env_trace) sit where three flow / entry tables and the flow count were, which no kernel read: the layout and
// size of EnvDev, i.e. every kernel's arguments, stay those of the untraced build.
struct EnvDev {
    int NL, NLP, NR, A;
    int trace_cap;                 // rows per traced instance (tsc_env_trace)
    int KMAX, PMAX, LMAX, SMAX, NBR, E;
    int NS, KC;                    // insertion streams (= NR when every route is its own stream), route choices per stream
    int NU, NLA;                   // lanes that can ever hold a vehicle (prefix after load sorting), rounded up to wavefronts
    int help;                      // phase A1 enabled (step_kernel)
    const float *lane_len, *lane_vmax, *lane_det;
    const int *lane_node, *lane_up;
    const int *lane_sib;           // [NL] sibling lane of a two-lane street or -1; null = no lane changing (rule 10)
    const int *mv;                 // [NL*NR] packed movement word, see mv_* helpers
    const uint8_t *zip;            // [NL*NR] zipper-merge slot: rank | count << 4 (0 = none)
    const int *trace_slot;         // [E] trace buffer of an instance, -1 = untraced; null = no trace armed (tsc_env_trace)
    int *trace_cnt;                // [n_trace][1 + episode]: rows counted so far (dropped ones too: the cursor), then rows per second
    const int *sroute;             // [NS] route of a stream's vehicles (-1: drawn); null = the stream index itself
    const int *smode;              // [NS] 0 fixed, 1 per-vehicle draw from schoice, 2 per-instance route (iroute)
    const int *schoice;            // [NS][KC][2] (route, cumulative weight of 65536)
    const float *sorigin;          // [NS][2] the stretch of the entry lane vehicles are inserted on, or null (whole lane)
    int NI, ilen;                  // choice intervals per stream and their length in seconds
    int *iroute;                   // [E][NS] routes of the mode-2 streams of the running episode
    uint4 *trace_rows;             // [n_trace][trace_cap] one row per live vehicle and second: {lane | route << 16, R0, x, v}
    const uint32_t *lane_routes;   // [NL][2] the (<= kMaxEntry) routes whose entry lane this is, one byte each, 0xFF = none
    const uint8_t *emit_tab;       // [NS][emit_len] vehicles each stream's flows emit at second t (per instance: see emit_inst)
    int emit_len;
    float sigma;                   // Krauss dawdling in force (tsc_env_set_car_following; 0: none).  In the padding behind emit_len: the
                                   // offsets of the other fields are those of the IDM-only build
    const int *agent_lanes, *agent_nlane, *agent_nlink, *agent_nphase;
    const uint8_t *green_tab, *yellow_tab;
    const int *nbr, *obs_kind, *obs_src;
    const int *obs_ks;             // [A*SMAX] obs_kind << 16 | obs_src (one load per observation entry)
    int ctrl, yellow, episode, teleport, queue_cap, objective, agent_kind, realnet_scale;
    double coop_gamma, norm_wave, norm_wait, clip_wave, clip_wait, coef_wait;
    float4 *S;                     // [E][NLP][CAP] vehicle records {x, v, desired-speed factor, bits of (w | route << 16)}
    int *N;                        // [E][NLP]
    int *pending, *serial;         // [E][NS]
    int *tsec;
    uint32_t *seed;
    int *prev_action;              // [E][A]
    float *fp;                     // [E][A][PMAX]
    unsigned long long *arrived;   // [E] vehicles that reached the end of their route this episode
    unsigned long long *teleported; // [E] heads the teleport surrogate took out of the network (truncated trips, NOT arrivals)
    double *reward_acc;            // [E] running sum of the global reward (training-curve logging, utils.py:161,296-305)
    const float *fp_bound;         // zero-copy fingerprint source (tsc_env_bind_fingerprint) or null
    long long *dbg;                // optional: shader-clock stamps of workgroup 0 / thread 0 (tsc_env_debug_clock)
    const int *order;              // [E] instance of workgroup b (tsc_env_set_block_order / the load balancer); null = b
    // ---- evaluation recording (envs/env.py:409-437,498-515; tsc_env_record): off on the training path
    int rec;                       // per-second network statistics + trip log are being kept
    int trip_cap;                  // trip records per instance
    const float *lane_origin;      // [NL] start of the SUMO lane inside the compiled lane (lane.* getters count from here)
    uint32_t *R0, *R1;             // per vehicle, indexed like X: depart_sec | serial << 16 ; waiting seconds | waiting count << 16
                                   // (R0 also under Krauss: the serial within the insertion stream travels with the vehicle)
    long long *rec_int;            // [E][8 sec][4]: vehicles, departed, arrived, sum of waiting times
    double *rec_speed;             // [E][8 sec]: sum of speeds (per-lane partial sums added in lane order)
    int *rec_queue;                // [E][8 sec][A * LMAX]: halting vehicles on every incoming lane (whole SUMO lane)
    int *trips;                    // [E][trip_cap][6]: route, serial, depart, arrival, waiting seconds, waiting count
    int *n_trips;                  // [E]
    unsigned long long *live_acc;  // [E] sum over control steps of the vehicles in the network (window-mean V)
    // ---- greedy controllers (tsc_env_set_greedy / tsc_env_greedy_actions): candidate flows per agent
    int GC, GT;                    // candidates per agent (padded), terms per candidate (padded)
    const int *g_ncand;            // [A]
    const int8_t *g_term;          // [A][GC][GT] observation index of a term, -1 = end
    const int *g_action;           // [A][GC] action a winning candidate stands for
    // ---- lane data (tsc_env_lane_data; SUMO's laneData): per slot -- one (lane, SUMO lane it is a piece of) pair -- and interval,
    // kept by the recording walk of kSpecLaneData / kSpecKraussLaneData.  Behind every other field: the offsets of those stay put.
    int ld_period;                 // interval length in seconds (a multiple of ctrl: a launch lies in one interval)
    int ld_nslot;                  // slots of the lanes < NU (a prefix of the slot table)
    const int *ld_slot0;           // [NL + 1] first slot of every lane (its pieces in driving order)
    const float4 *ld_bound;        // [NU] where a lane's pieces 2..5 start on it: the smallest float position on the piece (INFINITY: none)
    const int *ld_sumo;            // [ld_nslot] SUMO lane of the slot (an index)
    int *ld_int;                   // [E][n_interval][kLdInts][ld_nslot] sums, see kLdSampled...
    double *ld_speed;              // [E][n_interval][ld_nslot] sums of speeds (per-second sums in slot order, added in second order)
    // ---- per-instance demand (tsc_env_set_demand): emit_tab then holds one [NS][emit_len] table per instance, emit_inst bytes
    // apart (demand_kernel writes them at the reset); 0 = every instance reads the scenario's one table.  Behind every other field.
    int emit_inst;
};
// Integer fields of the lane data, in the order of tsc_env_read_lane_data
enum { kLdSampled, kLdWaiting, kLdDeparted, kLdArrived, kLdEntered, kLdLeft, kLdLcFrom, kLdLcTo, kLdTeleported, kLdInts };
constexpr int kLdMaxPieces = 5;        // slots per lane (Monaco's longest contracted chain): the lookup is four compares, no loop

__device__ __forceinline__ uint32_t hash32(uint32_t seed, uint32_t route, uint32_t serial, uint32_t stream) {
    uint32_t h = seed * 0x9E3779B1u + route * 0x85EBCA77u + serial * 0xC2B2AE3Du + stream * 0x27D4EB2Fu;
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// Wavefront scans on the DPP data path (gfx9: row_shr within the four 16-lane rows, then row_bcast:15 into rows 1 / 3 and
// row_bcast:31 into rows 2 / 3): a cross-lane step is one VALU move instead of a ds_bpermute_b32 with its address arithmetic
// (~5 instructions and an LDS round trip each; the flat phase ran 14 of them per super-round).  Lanes without a source lane
// keep `ident`, the identity of the operator, so no lane test is needed.
#define TSC_DPP_I(ident, v, ctrl, rows) __builtin_amdgcn_update_dpp((ident), (v), (ctrl), (rows), 0xF, false)
#define TSC_DPP_F(ident, v, ctrl, rows) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ident), __float_as_int(v), (ctrl), (rows), 0xF, false))
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118, kDppBcast15 = 0x142, kDppBcast31 = 0x143,
              kDppWaveShr1 = 0x138;
// inclusive prefix sum over the wavefront
__device__ __forceinline__ int wave_scan_add(int v) {
    v += TSC_DPP_I(0, v, kDppShr1, 0xF); v += TSC_DPP_I(0, v, kDppShr2, 0xF);
    v += TSC_DPP_I(0, v, kDppShr4, 0xF); v += TSC_DPP_I(0, v, kDppShr8, 0xF);
    v += TSC_DPP_I(0, v, kDppBcast15, 0xA); v += TSC_DPP_I(0, v, kDppBcast31, 0xC);
    return v;
}
// inclusive prefix maximum over the wavefront (values >= 0)
__device__ __forceinline__ int wave_scan_max(int v) {
    v = max(v, TSC_DPP_I(0, v, kDppShr1, 0xF)); v = max(v, TSC_DPP_I(0, v, kDppShr2, 0xF));
    v = max(v, TSC_DPP_I(0, v, kDppShr4, 0xF)); v = max(v, TSC_DPP_I(0, v, kDppShr8, 0xF));
    v = max(v, TSC_DPP_I(0, v, kDppBcast15, 0xA)); v = max(v, TSC_DPP_I(0, v, kDppBcast31, 0xC));
    return v;
}
// segmented inclusive min-scan: (v, f) <- (f ? v : min(v, v_prev), f | f_prev); f = 1 marks the first lane of a segment
__device__ __forceinline__ void wave_seg_scan_min(float &v, int &f) {
#define TSC_SEG_STEP(ctrl, rows) do {                                     \
        const float ov = TSC_DPP_F(INFINITY, v, ctrl, rows);              \
        const int of = TSC_DPP_I(0, f, ctrl, rows);                       \
        v = f ? v : fminf(v, ov); f |= of; } while (0)
    TSC_SEG_STEP(kDppShr1, 0xF); TSC_SEG_STEP(kDppShr2, 0xF); TSC_SEG_STEP(kDppShr4, 0xF); TSC_SEG_STEP(kDppShr8, 0xF);
    TSC_SEG_STEP(kDppBcast15, 0xA); TSC_SEG_STEP(kDppBcast31, 0xC);
#undef TSC_SEG_STEP
}

// one car-following evaluation against one leader (MICROSIM_SPEC.md rule 3; KR: the Krauss alternative, v_des = min(v + a,
// v_safe, v0) with the same safe speed -- tsc_env_set_car_following)
template <bool KR = false>
__device__ __forceinline__ float follow(float v, float v0, bool has_lead, float g, float vl, float s0gap) {
    if constexpr (KR) {
        float vsafe = INFINITY;
        if (has_lead) {
            float gs = g - s0gap;
            if (gs < 0.0f) gs = 0.0f;
            vsafe = sqrtf((kDec * kDec + vl * vl) + (2.0f * kDec) * gs) - kDec;
        }
        float vn = v + kAcc;
        if (vn > vsafe) vn = vsafe;
        if (vn > v0) vn = v0;
        if (vn < 0.0f) vn = 0.0f;
        return vn;
    }
    float ratio = v / v0;
    float r2 = ratio * ratio;
    float acc = kAcc * (1.0f - r2 * r2);
    float vsafe = INFINITY;
    if (has_lead) {
        float sstar = (kS0 + v * kTHead) + (v * (v - vl)) * kICab;
        if (sstar < kS0) sstar = kS0;
        float s = g < 0.5f ? 0.5f : g;
        float q = sstar / s;
        acc = acc - kAcc * (q * q);
        float gs = g - s0gap;
        if (gs < 0.0f) gs = 0.0f;
        vsafe = sqrtf((kDec * kDec + vl * vl) + (2.0f * kDec) * gs) - kDec;
    }
    if (acc < -kDec) acc = -kDec;
    float vn = v + acc;
    if (vn > vsafe) vn = vsafe;
    if (vn > v0 && v <= v0) vn = v0;
    if (vn < 0.0f) vn = 0.0f;
    return vn;
}

// SUMO's dawdling (Krauss, sigma > 0): v' = v_des - (sigma * min(v_des, a)) * u, u uniform per vehicle (route, serial within its
// insertion stream) and second t, floored at 0 -- applied to the minimum over the leaders, before the queue clamp
__device__ __forceinline__ float dawdle(float vn, float sigma, uint32_t seed, uint32_t route, uint32_t serial, uint32_t t) {
    const float u = u01(hash32(seed ^ 0x9E3779B9u, route, serial, t));
    vn = vn - (sigma * (vn < kAcc ? vn : kAcc)) * u;
    if (vn < 0.0f) vn = 0.0f;
    return vn;
}

__device__ __forceinline__ bool sig_open(int tl, int k, int a, int w, float x, float v, float L,
                                         const uint8_t *link, int KMAX, int teleport) {
    if (tl == -1) return true;                      // route ends at the lane end
    if (tl < -1) return false;                      // route n/a on this lane: hold
    if (a < 0) return true;                         // uncontrolled junction: always open
    if (k < 0) return false;
    if (w >= teleport) return true;
    uint8_t st = link[a * KMAX + k];
    if (st == 'G' || st == 'g') return true;
    if (st == 'y') {
        float need = (v * v) / (2.0f * kDec);
        return (L - x) < need;
    }
    return false;
}

// Table dimensions of the reference's scenarios as compile-time constants (SPEC of step_kernel; matched against the
// scenario at create time): 1 = large_grid (5x5), 2 = real_net (Monaco, lane chains contracted)
struct SpecDims { int NLP, NLA, NU, NR, A, KMAX, PMAX, LMAX, NBR, ctrl, yellow, teleport; };
constexpr int kSpecKrauss = -1;        // SPEC of the Krauss instantiations (runtime dimensions, tsc_env_set_car_following)
constexpr int kSpecTrace = -2, kSpecKraussTrace = -3;   // the recording walk that also writes per-vehicle rows (tsc_env_trace): IDM / Krauss
constexpr int kSpecLaneData = -4, kSpecKraussLaneData = -5;   // ... that keeps the lane data (tsc_env_lane_data), the trace optional
constexpr SpecDims kSpec[3] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                               {192, 128, 88, 12, 25, 12, 5, 6, 4, 5, 2, 600},     // NU: 81 lanes carry vehicles (83 with lane changing); the rest stay empty
                               {192, 128, 113, 16, 28, 22, 6, 11, 5, 5, 2, 300}};

struct Smem {
    int *mv;                                   // [NU*NR]
    int *n; float *tx, *tv, *hx, *hv; uint32_t *hm;   // lane summaries [NLA]
    float *ox, *ov, *osf; uint32_t *om; int *oto;     // outbox [kMaxCross*NLA]
    int *nout;                                  // [NLA]
    int *wave, *halt, *hwait;                   // detectors [NLP]
    double *r;                                  // local rewards [A] (+1 for global)
    uint8_t *link_y, *link_g;                   // [A*KMAX]
    float *len, *vmax; int *node;               // lane length / speed limit / downstream agent [NLA]
    int *sib;                                   // sibling lane (rule 10) or -1 [NLA]
    int *pend, *ser; uint8_t *emit;             // per-stream insertion state [NS], emissions [NS*8]
    uint8_t *zip;                               // [NU*NR]
    uint32_t *up4;                              // [NLA] the lane's feeders, a byte each (0xFF = none): merge arbitration
    int *pre, *wtot;                            // wave-local inclusive scan of queued vehicles [NLA] (from phase H on: the lane's
                                                // first flat index), wave totals [16]
    uint8_t *mark; uint16_t *bound;             // flat phase: mark[k] = (lane & 63) + 1 where a lane's queued vehicles start at flat index
                                                // k (else 0) [NLA * (kCap - 1)]; bound[j] = lane + 1 of the owner of flat index 64 j
    int *nc; float *seed;                       // per lane: vehicles ahead of the first one that stays; its chain key [NLA]
    float *wtail, *hz;                          // wave tails of the chain scan [2][16]; old (x, v) across super-rounds [2]
    uint32_t *or0, *or1;                        // outbox of the trip records [kMaxCross*NLA]      (recording only)
    int *rq; double *rsp; long long *rint;      // per-lane halting [NLA], speed partial sums [NLA], counters [4]  (recording only)
    int *ldi; double *ldsp, *ldsec;             // lane data of the launch's interval [kLdInts][ld_nslot], speed sums [ld_nslot], this
                                                // second's speed sums [ld_nslot]                                   (LD only)
    float4 *ldb; int *ldsu;                     // copies of ld_bound [NU] / ld_sumo [ld_nslot]                     (LD only)
};

// One layout for the step and the reset kernel.
// KR: the Krauss kernels also hand the vehicles' R0 words over through the outbox (or0), recording or not.
// LD: the lane-data kernels (a recording walk: no flat phase) hold the lane data where the flat phase's arrays are otherwise.
template <bool KR = false, bool LD = false, class Take>
__host__ __device__ __forceinline__ void smem_layout(Smem &s, const EnvDev &P, Take take) {
    s.r = (double *)take(sizeof(double) * (P.A + 1));
    s.mv = (int *)take(sizeof(int) * P.NU * P.NR);
    s.n = (int *)take(4 * P.NLA); s.tx = (float *)take(4 * P.NLA); s.tv = (float *)take(4 * P.NLA);
    s.hx = (float *)take(4 * P.NLA); s.hv = (float *)take(4 * P.NLA); s.hm = (uint32_t *)take(4 * P.NLA);
    s.ox = (float *)take(4 * kMaxCross * P.NLA); s.ov = (float *)take(4 * kMaxCross * P.NLA);
    s.osf = (float *)take(4 * kMaxCross * P.NLA); s.om = (uint32_t *)take(4 * kMaxCross * P.NLA);
    s.oto = (int *)take(4 * kMaxCross * P.NLA);
    s.nout = (int *)take(4 * P.NLA);
    s.wave = (int *)take(4 * P.NLP); s.halt = (int *)take(4 * P.NLP); s.hwait = (int *)take(4 * P.NLP);
    s.link_y = (uint8_t *)take(P.A * P.KMAX); s.link_g = (uint8_t *)take(P.A * P.KMAX);
    s.len = (float *)take(4 * P.NLA); s.vmax = (float *)take(4 * P.NLA); s.node = (int *)take(4 * P.NLA);
    s.sib = (int *)take(4 * P.NLA);
    s.pend = (int *)take(4 * P.NS); s.ser = (int *)take(4 * P.NS); s.emit = (uint8_t *)take(8 * P.NS);
    s.zip = (uint8_t *)take((P.NU * P.NR + 3) / 4 * 4);
    s.up4 = (uint32_t *)take(4 * P.NLA);
    s.pre = (int *)take(4 * P.NLA); s.wtot = (int *)take(4 * 16);
    if constexpr (LD) {
        s.mark = nullptr; s.bound = nullptr; s.nc = nullptr; s.seed = nullptr; s.wtail = nullptr; s.hz = nullptr;
        s.ldi = (int *)take(4 * kLdInts * (size_t)P.ld_nslot); s.ldsp = (double *)take(8 * (size_t)P.ld_nslot);
        s.ldsec = (double *)take(8 * (size_t)P.ld_nslot); s.ldb = (float4 *)take(16 * (size_t)P.NU); s.ldsu = (int *)take(4 * (size_t)P.ld_nslot);
    } else {
        s.mark = (uint8_t *)take((size_t)P.NLA * (kCap - 1) + 8); s.bound = (uint16_t *)take(2 * ((size_t)P.NLA * (kCap - 1) / 64 + 8));
        s.nc = (int *)take(4 * P.NLA); s.seed = (float *)take(4 * P.NLA); s.wtail = (float *)take(4 * 32); s.hz = (float *)take(4 * 4);
    }
    if (P.rec) {
        s.or0 = (uint32_t *)take(4 * kMaxCross * P.NLA); s.or1 = (uint32_t *)take(4 * kMaxCross * P.NLA);
        s.rq = (int *)take(4 * P.NLA); s.rsp = (double *)take(8 * P.NLA); s.rint = (long long *)take(8 * 4);
    } else {
        s.or0 = s.or1 = nullptr; s.rq = nullptr; s.rsp = nullptr; s.rint = nullptr;
        if constexpr (KR) s.or0 = (uint32_t *)take(4 * kMaxCross * P.NLA);
    }
}

template <bool KR = false, bool LD = false>
__device__ __forceinline__ Smem carve(char *base, const EnvDev &P) {
    Smem s;
    char *p = base;
    smem_layout<KR, LD>(s, P, [&](size_t bytes) { char *q = p; p += (bytes + 15) & ~size_t(15); return q; });
    return s;
}

template <bool KR = false, bool LD = false>
size_t smem_bytes(const EnvDev &P) {
    Smem s;
    size_t tot = 0;
    smem_layout<KR, LD>(s, P, [&](size_t bytes) { tot += (bytes + 15) & ~size_t(15); return (char *)nullptr; });
    return tot;
}

// numpy's float64 pairwise sum (np.sum at envs/env.py:580), one block: n <= 128
__device__ __forceinline__ double np_sum_block(const double *a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
// ... and the whole sum: above 128 elements numpy halves recursively -- pw(a, n) = pw(a, n2) + pw(a + n2, n - n2) with n2 = n / 2
// rounded down to a multiple of 8 -- down to blocks.  The same walk without recursion: seg[2 d], seg[2 d + 1] are (offset, length)
// of the node at depth d of the path to the current block, left[d] the sum of that node's left half once the walk is in its right
// half.  A half is at most n / 2 + 8 long, so kNpSumDepth levels reach blocks for every n <= 2048, and tsc_env_create admits no
// more agents than that (2 n_agent <= kMaxCross * NLA <= 4096).  left / seg: kNpSumDepth entries / pairs of the caller's (LDS).
// Networks of more than 128 agents: tests/test_networks_gpu.py isolated_130 (one split), isolated_254 (a split inside the right half)
// and isolated_300 (the left half splits again: two levels down the left).
constexpr int kNpSumDepth = 8;
__device__ __forceinline__ double np_sum(const double *a, int n, double *left, int *seg) {
    if (n <= 128) return np_sum_block(a, n);
    int d = 0;
    unsigned right = 0u;                            // bit d: the node at depth d is a right half
    seg[0] = 0; seg[1] = n;
    for (;;) {
        while (seg[2 * d + 1] > 128 && d + 1 < kNpSumDepth) {       // down the left halves to a block
            int n2 = seg[2 * d + 1] / 2;
            n2 -= n2 % 8;
            seg[2 * d + 2] = seg[2 * d]; seg[2 * d + 3] = n2;
            ++d;
            right &= ~(1u << d);
        }
        double ret = np_sum_block(a + seg[2 * d], seg[2 * d + 1]);
        while (d > 0 && ((right >> d) & 1u)) { --d; ret = left[d] + ret; }      // a right half closes its parent
        if (d == 0) return ret;
        --d;                                        // a left half: keep its sum and go to the right half
        left[d] = ret;
        int n2 = seg[2 * d + 1] / 2;
        n2 -= n2 % 8;
        seg[2 * d + 2] = seg[2 * d] + n2; seg[2 * d + 3] = seg[2 * d + 1] - n2;
        ++d;
        right |= 1u << d;
    }
}

__device__ __forceinline__ double norm_clip(double x, double norm, double clip) {
    x = x / norm;                                   // envs/env.py:439-442
    if (clip < 0) return x;
    return fmin(fmax(x, 0.0), clip);
}

// K5: float32(state) for every agent of env e (envs/env.py:163-205)
__device__ void emit_obs(const EnvDev &P, const Smem &s, int e, float *obs) {
    const int tot = P.A * P.SMAX;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < tot; idx += blockDim.x) {
        int kind = P.obs_kind[idx], src = P.obs_src[idx];
        float o = 0.0f;
        if (kind == 1) o = (float)norm_clip((double)s.wave[src], P.norm_wave, P.clip_wave);
        else if (kind == 2) o = (float)(norm_clip((double)s.wave[src], P.norm_wave, P.clip_wave) * P.coop_gamma);
        else if (kind == 3) o = (float)norm_clip((double)s.hwait[src], P.norm_wait, P.clip_wait);
        else if (kind == 4) o = (P.fp_bound ? P.fp_bound : P.fp)[(size_t)e * P.A * P.PMAX + src];
        obs[(size_t)e * tot + idx] = o;
    }
}

__global__ void reset_kernel(EnvDev P, const uint32_t *seeds, float *obs) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    Smem s = carve(smem_raw, P);
    const int e = blockIdx.x, l = threadIdx.x;
    if (l < P.NLP) { P.N[(size_t)e * P.NLP + l] = 0; s.wave[l] = 0; s.hwait[l] = 0; }
    for (int r = l; r < P.NS; r += blockDim.x) {
        P.pending[(size_t)e * P.NS + r] = 0;
        P.serial[(size_t)e * P.NS + r] = 0;
    }
    for (int a = l; a < P.A; a += blockDim.x) {
        P.prev_action[(size_t)e * P.A + a] = 0;                    // envs/env.py:448
        int na = P.agent_nphase[a];
        float p = (float)(1.0 / (double)na);                       // envs/env.py:263-269
        for (int k = 0; k < P.PMAX; ++k) P.fp[((size_t)e * P.A + a) * P.PMAX + k] = k < na - 1 ? p : 0.0f;
    }
    if (l == 0) { P.tsec[e] = 0; P.seed[e] = seeds[e]; P.arrived[e] = 0ull; P.teleported[e] = 0ull; P.n_trips[e] = 0; }
    __syncthreads();
    emit_obs(P, s, e, obs);
}

// Per-instance demand (tsc_env_set_demand): the emission tables of all instances, [E][NS][emit_len] bytes, from each instance's
// veh/h column.  The flow elements' windows and streams are the scenario's (fl: {begin, end, flow index} per element, grouped by
// stream, off[r] .. off[r + 1] those of stream r); the counts follow tsc_env_create's integer rule: second t of an element that
// starts at b emits ceil((t - b + 1) vph / 3600) - ceil((t - b) vph / 3600).  One workgroup per (stream, instance), one thread
// per four seconds: five ceilings give the four counts, one 32-bit store writes them (emit_len is a multiple of 4).
__global__ void __launch_bounds__(256) demand_kernel(uint8_t *__restrict__ rows, const int *__restrict__ vph, const int *__restrict__ off,
                                                     const int *__restrict__ fl, int NS, int emit_len, int n_flow) {
    const int r = blockIdx.x, e = blockIdx.y;
    const int f0 = off[r], f1 = off[r + 1];
    uint32_t *row = (uint32_t *)(rows + ((size_t)e * NS + r) * emit_len);
    const int *rate = vph + (size_t)e * n_flow;
    for (int w = threadIdx.x; w < emit_len / 4; w += blockDim.x) {
        const int t0 = 4 * w;
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        for (int f = f0; f < f1; ++f) {
            const int b = fl[3 * f], en = fl[3 * f + 1];
            if (t0 + 4 <= b || t0 >= en) continue;
            const unsigned long long v = (unsigned long long)rate[fl[3 * f + 2]];
            // vehicles the element has emitted before second t: ceil(clamp(t - b, 0, en - b) v / 3600)
            unsigned long long cum[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                int tau = t0 + k - b;
                tau = tau < 0 ? 0 : tau > en - b ? en - b : tau;
                cum[k] = ((unsigned long long)tau * v + 3599ull) / 3600ull;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] += (uint32_t)(cum[k + 1] - cum[k]);
        }
        row[w] = c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24;       // (each <= 255: tsc_env_set_demand checked the column)
    }
}

__global__ void fingerprint_kernel(EnvDev P, const float *pi) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t tot = (size_t)P.E * P.A * P.PMAX;
    if (i < tot) P.fp[i] = pi[i];                                  // pi[:-1] is applied at gather time
}

// The reference's greedy controllers (LargeGridController envs/large_grid_env.py:45-60, RealNetController
// envs/real_net_env.py:78-111, SmallGridController envs/small_grid_env.py:40-55) are one rule over different tables: every
// candidate sums some of the agent's OWN wave entries in a fixed order, float64, starting from 0 -- `ob[0] + ob[3]`, `wave
// += ob[j]` per green link in link order, `ob[k]` alone -- and np.argmax keeps the FIRST maximum; the winner stands for an
// action (the phase itself, or small_grid's STATE_PHASE_MAP entry).  One thread per (instance, agent).
// The controllers see the env's float64 state, this kernel the float32 observation: a wave entry is a vehicle count over
// norm_wave, clipped (envs/env.py:439-442), so the count is recovered (rint(ob * norm_wave); exact for counts < 2^20) and
// the float64 value recomputed with the reference's operations -- ties between candidates then fall as they do in the
// reference (0.2 + 0.4 > 0.6 in float64, a tie on the float32 values).
__global__ void __launch_bounds__(256) greedy_kernel(EnvDev P, const float *__restrict__ obs, int *__restrict__ action) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.E * P.A) return;
    const int a = i % P.A;
    const float *ob = obs + (size_t)i * P.SMAX;
    const int8_t *term = P.g_term + (size_t)a * P.GC * P.GT;
    const float clipf = (float)P.clip_wave;
    double best = 0.0;
    int arg = 0;
    const int nc = P.g_ncand[a];
    for (int c = 0; c < nc; ++c) {
        double flow = 0.0;
        for (int k = 0; k < P.GT; ++k) {
            const int j = term[c * P.GT + k];
            if (j < 0) break;
            const float o = ob[j];
            double x = rint((double)o * P.norm_wave) / P.norm_wave;
            if (P.clip_wave >= 0.0 && (x > P.clip_wave || o == clipf)) x = P.clip_wave;
            flow += x;
        }
        if (c == 0 || flow > best) { best = flow; arg = c; }
    }
    action[i] = P.g_action[a * P.GC + arg];
}

// The movement tables that the max-pressure controller and the pressure reward each hold a set of (upload_movements).  Lanes are
// the scenario's (= the device's, load-sorted) lanes.
struct MovDev {
    int n_mov, n_walk;             // movements; lanes that appear in one, as its incoming or its downstream lane
    int measure;                   // TSC_PRESSURE_*
    const short *walk;             // [n_walk] the walked lanes, ascending
    const short *mov_of;           // [NL * NR] movement of (lane, route), -1 = none
    const short *mov_dn;           // [n_mov] index into walk of the movement's downstream lane
};

// Tables and state of the max-pressure controller (tsc_env_set_pressure), a kernel argument of their own: EnvDev -- every other
// kernel's argument -- keeps its layout and size.
struct PressDev {
    MovDev M;
    int min_green;                 // control steps a chosen phase is held at least
    const int *srv_off;            // [A * PMAX + 1] phase (a, p) serves the movements srv[srv_off[a * PMAX + p] .. srv_off[.. + 1])
    const short *srv;
    int *hold;                     // [E][A][2] {cur, age}: the phase being held and the control steps it has been
};
constexpr int kPressT = 256;       // threads per instance

// The flat walk of the controllers' kernels and the pressure reward (step (a) of pressure_kernel's comment), the one copy: fills
// start [n_walk + 1] for instance e from the counts of the lanes walk [n_walk], calling at_lane(w, n) once per walked lane (its index
// into walk, its clamped count), then at_record(w, lane, record) once per live record of those lanes.  `part` is [kPressT] scan
// scratch.  Every thread of the workgroup calls it; whatever LDS the caller zeroed before the call is zero for every at_record (a
// barrier lies between), and the callbacks' sums are complete when it returns (it ends on a barrier).
template <class LaneFn, class RecFn>
__device__ __forceinline__ void flat_walk(const EnvDev &P, const short *__restrict__ walk, int n_walk, int e, int *start, int *part,
                                          LaneFn at_lane, RecFn at_record) {
    const int t = threadIdx.x;
    const int *N = P.N + (size_t)e * P.NLP;
    const float4 *S = P.S + (size_t)e * kCap * P.NLP;
    // counts of this thread's run of walked lanes, their exclusive prefix sum over the workgroup
    const int chunk = (n_walk + kPressT - 1) / kPressT, w0 = t * chunk;
    int local = 0;
    for (int w = w0; w < w0 + chunk && w < n_walk; ++w) {
        const int n = N[walk[w]];
        local += n < 0 ? 0 : n > kCap ? kCap : n;
    }
    part[t] = local;
    __syncthreads();
    for (int d = 1; d < kPressT; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - local;
    for (int w = w0; w < w0 + chunk && w < n_walk; ++w) {
        int n = N[walk[w]];
        n = n < 0 ? 0 : n > kCap ? kCap : n;
        start[w] = run;
        at_lane(w, n);
        run += n;
    }
    if (t == kPressT - 1) start[n_walk] = part[t];
    __syncthreads();
    const int total = start[n_walk];
    for (int f = t; f < total; f += kPressT) {
        int lo = 0, hi = n_walk;               // the last walked lane whose first record is at or before f (empty lanes repeat a start)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (start[mid] <= f) lo = mid; else hi = mid;
        }
        const int lane = walk[lo];
        at_record(lo, lane, S[vslot(f - start[lo], lane, P.NLP)]);
    }
    __syncthreads();
}

// A record's movement: that of (its lane, the route in the upper half of its last word), -1 = none.
__device__ __forceinline__ int record_movement(const EnvDev &P, const short *__restrict__ mov_of, int lane, const float4 &rec) {
    const int route = (int)(__float_as_uint(rec.w) >> 16);
    return route < P.NR ? mov_of[lane * P.NR + route] : -1;
}

// flat_walk for pressure_kernel and pressure_reward_kernel: fills start / down / up for instance e from the live records of the
// walked lanes.
__device__ __forceinline__ void pressure_walk(const EnvDev &P, const MovDev &M, int e, int *start, int *down, int *up, int *part) {
    const bool queue = M.measure == TSC_PRESSURE_QUEUE;
    const short *__restrict__ mov_of = M.mov_of;
    for (int m = threadIdx.x; m < M.n_mov; m += kPressT) up[m] = 0;
    flat_walk(P, M.walk, M.n_walk, e, start, part,
              [=](int w, int n) { down[w] = queue ? 0 : n; },       // count: every vehicle of the lane
              [=, &P](int w, int lane, const float4 &rec) {
                  if (queue && !(rec.y < kHalt)) return;
                  const int mv = record_movement(P, mov_of, lane, rec);
                  if (mv >= 0) atomicAdd(&up[mv], 1);
                  if (queue) atomicAdd(&down[w], 1);
              });
}

// Max-pressure (Varaiya 2013), the rule of INTEGRATION.md "Baseline controllers": with q(vehicle) = 1 (count) or v < kHalt (queue),
// up(movement) = sum of q over the vehicles on its incoming lane whose route takes the movement, down(lane) = sum of q over ALL
// vehicles of the lane; the pressure of phase p is the int32 sum over the movements it serves of up - down(downstream lane); the
// action is the first maximum over p < n_phase, subject to the hold (min_green).  Integers only: the result is exact.
// One workgroup per instance.  (a) The live records of the walked lanes are visited in one flat (lane, slot) order -- exclusive
// prefix sum of the lanes' counts in LDS, a record's lane by binary search in it -- so a wavefront loads 64 consecutive live
// records, contiguous within a lane, and never a dead slot; the sums are LDS integer atomics (addition order cannot change an
// integer sum).  (b) One thread per (agent, phase) adds up its list.  (c) One thread per agent: argmax, hold, stores.
// Reads EnvDev, writes only action / pressure / Q.hold.  One call per control step: a call advances the hold state.
__global__ void __launch_bounds__(kPressT) pressure_kernel(EnvDev P, PressDev Q, int *__restrict__ action, int *__restrict__ pressure) {
    extern __shared__ int psm[];
    int *start = psm;                          // [n_walk + 1] flat index of a walked lane's first record
    int *down = start + Q.M.n_walk + 1;        // [n_walk]
    int *up = down + Q.M.n_walk;               // [n_mov]
    int *prs = up + Q.M.n_mov;                 // [A * PMAX]
    int *part = prs + P.A * P.PMAX;            // [kPressT] scan scratch
    const int e = blockIdx.x, t = threadIdx.x;
    pressure_walk(P, Q.M, e, start, down, up, part);
    for (int i = t; i < P.A * P.PMAX; i += kPressT) {
        int sum = 0;
        for (int j = Q.srv_off[i]; j < Q.srv_off[i + 1]; ++j) {
            const int mv = Q.srv[j];
            sum += up[mv] - down[Q.M.mov_dn[mv]];
        }
        prs[i] = sum;                          // (padded phases serve nothing: 0)
        if (pressure) pressure[(size_t)e * P.A * P.PMAX + i] = sum;
    }
    __syncthreads();
    for (int a = t; a < P.A; a += kPressT) {
        int2 *hold = (int2 *)Q.hold + (size_t)e * P.A + a;
        int2 h = *hold;                        // {cur, age}
        if (h.y < Q.min_green) h.y += 1;
        else {
            int arg = 0;
            for (int p = 1; p < P.agent_nphase[a]; ++p)
                if (prs[a * P.PMAX + p] > prs[a * P.PMAX + arg]) arg = p;
            if (arg != h.x) { h.x = arg; h.y = 1; }
            else h.y = Q.min_green;            // (held long enough: the count need not run on)
        }
        *hold = h;
        action[(size_t)e * P.A + a] = h.x;
    }
}

// Tables, parameters and state of the actuated and SOTL controllers (tsc_env_set_actuated), a kernel argument of their own like
// PressDev and independent of it.  The walk covers the movements' incoming lanes only: no downstream lane is read.
struct ActDev {
    int n_mov, n_walk;             // movements; their incoming lanes
    int rule;                      // TSC_ACTUATED_*
    int min_green, max_green;      // control steps (max_green: the gap rule's)
    int theta, mu;                 // SOTL: threshold (vehicles x control steps), the platoon that is not cut
    const short *walk;             // [n_walk] the incoming lanes, ascending
    const short *mov_of;           // [NL * NR] movement of (lane, route), -1 = none
    const float *zone;             // [NL] a vehicle within zone[l] of its lane's end is near (calls)
    const int *srv_off;            // [A * PMAX + 1] as PressDev's
    const short *srv;
    const unsigned *mask;          // [n_mov] bit p: phase p of the movement's agent serves it
    int *hold;                     // [E][A][2] {cur, age}
    int *kappa;                    // [E][A][PMAX] SOTL's integrated red-time demand
};

// Gap-based actuated control and SOTL, the rules of INTEGRATION.md "Baseline controllers".  One workgroup per instance.  (a) The
// flat walk over the incoming lanes: cnt(movement) = its vehicles, near(movement) = those with float32(lane_len - x) <= zone[lane] --
// one fp32 subtraction and a compare, nothing the compiler could contract.  (b) One thread per (agent, phase): call = sum of near,
// dem = sum of cnt over the served movements; under SOTL, in dem's place, red = the sum of cnt over those the agent's current phase
// does not serve too (phase_mask), and kappa's update with it: every kappa of an agent moves in parallel, not one after the other
// in its thread.  (c) One thread per agent: the rule, the stores.  Integers but for the compare: the result is exact.  Reads EnvDev, writes only action / counts / D.hold / D.kappa.  One call per control step.
__global__ void __launch_bounds__(kPressT) actuated_kernel(EnvDev P, ActDev D, int *__restrict__ action, int *__restrict__ counts) {
    extern __shared__ int asm_[];
    int *start = asm_;                         // [n_walk + 1] flat index of a walked lane's first record
    int *cnt = start + D.n_walk + 1;           // [n_mov]
    int *near = cnt + D.n_mov;                 // [n_mov]
    int *sums = near + D.n_mov;                // [A * PMAX][3] {call, dem | red, kappa}
    int *part = sums + 3 * P.A * P.PMAX;       // [kPressT] scan scratch
    const int e = blockIdx.x, t = threadIdx.x;
    const bool sotl = D.rule == TSC_ACTUATED_SOTL;
    const short *__restrict__ mov_of = D.mov_of;
    const float *__restrict__ zone = D.zone, *__restrict__ lane_len = P.lane_len;
    for (int m = t; m < 2 * D.n_mov; m += kPressT) cnt[m] = 0;     // (cnt and near)
    flat_walk(P, D.walk, D.n_walk, e, start, part, [](int, int) {},
              [=, &P](int, int lane, const float4 &rec) {
                  const int mv = record_movement(P, mov_of, lane, rec);
                  if (mv < 0) return;
                  atomicAdd(&cnt[mv], 1);
                  if (lane_len[lane] - rec.x <= zone[lane]) atomicAdd(&near[mv], 1);
              });
    const int2 *hold_e = (const int2 *)D.hold + (size_t)e * P.A;
    int *kappa_e = D.kappa + (size_t)e * P.A * P.PMAX;
    for (int i = t; i < P.A * P.PMAX; i += kPressT) {
        int call = 0, dem = 0;
        if (!sotl) {
            for (int j = D.srv_off[i]; j < D.srv_off[i + 1]; ++j) {
                const int mv = D.srv[j];
                call += near[mv];
                dem += cnt[mv];
            }
        } else {
            const int a = i / P.PMAX, cur = hold_e[a].x;
            const int k0 = kappa_e[i];
            for (int j = D.srv_off[i]; j < D.srv_off[i + 1]; ++j) {
                const int mv = D.srv[j];
                call += near[mv];
                dem += (D.mask[mv] >> cur) & 1u ? 0 : cnt[mv];
            }
            const int k = i - a * P.PMAX == cur ? 0 : k0 + dem;         // (padded phases serve nothing: theirs stays 0)
            kappa_e[i] = k; sums[3 * i + 2] = k;
        }
        sums[3 * i] = call; sums[3 * i + 1] = dem;             // (padded phases serve nothing: 0)
        if (counts) {
            int *c = counts + 2 * ((size_t)e * P.A * P.PMAX + i);
            c[0] = call; c[1] = dem;
        }
    }
    __syncthreads();
    for (int a = t; a < P.A; a += kPressT) {
        int2 *hold = (int2 *)D.hold + (size_t)e * P.A + a;
        int2 h = *hold;                        // {cur, age}
        const int n = P.agent_nphase[a];
        const int *s = sums + 3 * a * P.PMAX;
        if (!sotl) {
            if (h.y < D.min_green) h.y += 1;
            else if (h.y < D.max_green && s[3 * h.x] > 0) h.y += 1;            // the extension
            else {
                int q = -1;                    // the first phase after cur, cyclically, with demand
                for (int d = 1; d < n && q < 0; ++d) {
                    const int p = h.x + d < n ? h.x + d : h.x + d - n;
                    if (s[3 * p + 1] > 0) q = p;
                }
                if (q < 0) h.y = h.y + 1 < D.max_green ? h.y + 1 : D.max_green;
                else { h.x = q; h.y = 1; }
            }
        } else {
            int q = -1, best = 0;              // the FIRST maximum of the updated kappa over p != cur
            for (int p = 0; p < n; ++p) {
                const int k = s[3 * p + 2];
                if (p != h.x && (q < 0 || k > best)) { q = p; best = k; }
            }
            const int call = s[3 * h.x];
            if (h.y < D.min_green || (call > 0 && call <= D.mu) || q < 0 || best < D.theta) h.y = h.y < (1 << 30) ? h.y + 1 : 1 << 30;
            else { h.x = q; h.y = 1; kappa_e[a * P.PMAX + q] = 0; }
        }
        *hold = h;
        action[(size_t)e * P.A + a] = h.x;
    }
}

// The reward shaping of envs/env.py:580,:590-631, float64: r is [A + 1], the agents' local rewards and then their sum g.  Thread
// `first` of `stride` stores the returned reward of agents first, first + stride, ...  (The same loop ends step_kernel's K6.)
__device__ __forceinline__ void shape_rewards(const EnvDev &P, const double *r, int e, double *reward, int train_mode, int first, int stride) {
    for (int a = first; a < P.A; a += stride) {
        const double g = r[P.A];
        double out;
        if (!train_mode) {
            out = r[a];
        } else if (P.agent_kind == TSC_AGENT_GREEDY) {
            out = g;
        } else if (P.agent_kind == TSC_AGENT_GLOBAL) {
            out = P.realnet_scale ? g / (double)(P.A * 20) : g;
        } else {
            double cur = r[a];
            int deg = 0;
            for (int j = 0; j < P.NBR; ++j) {
                const int nb = P.nbr[a * P.NBR + j];
                if (nb < 0) break;
                cur += P.coop_gamma * r[nb];
                ++deg;
            }
            out = P.realnet_scale ? cur / (double)((1 + deg) * 20) : cur;
        }
        reward[(size_t)e * P.A + a] = out;
    }
}

// Tables and accumulator of the pressure reward (tsc_env_set_reward_pressure), a kernel argument of their own like PressDev and
// independent of it: the controller and the reward may be armed with different measures, or one without the other.
struct PressRewDev {
    MovDev M;
    const int *agt_off;            // [A + 1] agent a owns the movements agt_mov[agt_off[a] .. agt_off[a + 1])
    const short *agt_mov;
    double *acc;                   // [E] running sum of the global pressure reward (tsc_env_reward_sum while armed)
};

// The pressure reward, the rule of INTEGRATION.md "Pressure reward": P[a] = int32 sum over the agent's movements of up - down(downstream
// lane) on the state step_kernel left, r[a] = -|P[a]|, g = sum of r; the returned reward is shaped as step_kernel shapes its own
// (K6).  Runs behind step_kernel on the same stream and overwrites reward / greward; reads EnvDev, writes nothing else but R.acc.
// One workgroup per instance: the walk of pressure_kernel, then one thread per agent sums its movements, one thread forms g, one
// thread per agent shapes and stores.  r and g are integers in float64: no order of addition can change them.
__global__ void __launch_bounds__(kPressT) pressure_reward_kernel(EnvDev P, PressRewDev R, double *__restrict__ reward,
                                                                  double *__restrict__ greward, int train_mode) {
    extern __shared__ __attribute__((aligned(16))) char prw_raw[];
    double *r = (double *)prw_raw;             // [A + 1] local rewards, then g
    int *start = (int *)(r + P.A + 1);         // [n_walk + 1]
    int *down = start + R.M.n_walk + 1;        // [n_walk]
    int *up = down + R.M.n_walk;               // [n_mov]
    int *part = up + R.M.n_mov;                // [kPressT]
    const int e = blockIdx.x, t = threadIdx.x;
    pressure_walk(P, R.M, e, start, down, up, part);
    for (int a = t; a < P.A; a += kPressT) {
        int sum = 0;
        for (int j = R.agt_off[a]; j < R.agt_off[a + 1]; ++j) {
            const int mv = R.agt_mov[j];
            sum += up[mv] - down[R.M.mov_dn[mv]];
        }
        r[a] = (double)(sum < 0 ? sum : -sum);
    }
    __syncthreads();
    if (t == 0) {
        double g = 0.0;
        for (int a = 0; a < P.A; ++a) g += r[a];
        r[P.A] = g; greward[e] = g; R.acc[e] += g;
    }
    __syncthreads();
    shape_rewards(P, r, e, reward, train_mode, t, kPressT);
}

// Fixed-time cycle: phase (t / steps) % n_phase at control step t = tsec / control interval.  One thread per (instance, agent).
__global__ void __launch_bounds__(256) fixed_time_kernel(EnvDev P, int steps, int *__restrict__ action) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.E * P.A) return;
    const int t = P.tsec[i / P.A] / P.ctrl;
    action[i] = (t / steps) % P.agent_nphase[i % P.A];
}

// Work decomposition of one workgroup (= one env instance):
//   * lane threads (l < NLA) own one lane each: the head walk (phase H), the gather (phase B);
//   * with HELP, phase F evaluates the car-following law of every queued vehicle behind the first one that stays with
//     ALL threads of the workgroup, KF vehicles per thread in a flat, load-balanced order (prefix sum over the lane
//     counts; the lane of a flat index from byte marks + a wavefront prefix maximum).  A queued vehicle that is not the head of a platoon crossing in this very
//     second cannot cross, so its new speed depends only on OLD state (itself, the vehicle ahead, the signal):
//     min(follow(leader), follow(stop line) if the link is closed).  The walk then only applies the clamps and
//     the bookkeeping (~50 instructions per vehicle instead of ~500); heads and vehicles right behind a vehicle
//     that crossed this second are still evaluated inline.  Lanes are very unevenly loaded (a wavefront walks as
//     long as its fullest lane while most of its 64 threads idle), so this halves the VALU work of the kernel.
// Register budget: the 256-thread instantiation is capped at 128 VGPRs (4 waves / SIMD).  With 155 VGPRs the
// grid fits the chip with no slack, and whenever another kernel ran in between (i.e. always, in the training
// loop) XCD 0 admitted ~30 workgroups one full round late -> 178 us became 316 us per step
// (tools/bench_env.py, tsc_env_debug_clock).  Since the scalar side stopped spilling into VGPR lanes (below) no instantiation
// needs scratch under the cap: the benchmarked one takes 88 VGPRs (122 before, two of them full of spilled scalars), the
// runtime-dimension ones 99 - 128 (128 and 284 - 424 B of scratch before).
// SPEC 1: the table dimensions of the reference's large_grid are compile-time constants (LDS offsets and index products
// fold into immediates: the kernel holds > 100 scalar values otherwise and reloads the spilled ones with v_readlane)
// SPEC = kSpecKrauss (tsc_env_set_car_following): runtime table dimensions and the Krauss car following with SUMO's dawdling
// instead of rule 3's IDM (KR); the vehicles' R0 words (depart | serial << 16) then travel with them on every path (SER), recording
// or not.  (A sentinel of SPEC rather than one more template parameter: the IDM kernels keep their symbols and their code.)
// SPEC = kSpecTrace / kSpecKraussTrace (tsc_env_trace, recording walk only): after every simulated second a workgroup whose instance
// is traced writes one row per live vehicle, in (lane, slot) order, behind its running cursor (TR; see the end of the second loop).
// SPEC = kSpecLaneData / kSpecKraussLaneData (tsc_env_lane_data, recording walk only): the same, the trace optional (null
// trace_slot: none), and the lane thread also keeps its slots' lane data (LD): it finds every vehicle's slot at the end of the
// second from its position, and counts the vehicles, the halting ones, the speeds and the events on it; a hand-off carries the
// vehicle's old slot in the upper half of its outbox target, so that the gathering thread counts `entered` / `laneChangedTo` on
// its own slot and `left` / `laneChangedFrom` (LDS atomics) on the source's.  The interval's sums stay in LDS for the launch.
// Scalar registers.  The kernel's arguments are ~100 dwords of kernarg memory, the compiler loads them 8 or 16 dwords at a time at
// kernel entry, and what the second loop or the epilogue reads of them then stays live -- in whole 16-dword tuples -- across the
// loop, where 106 SGPRs do not hold it: the surplus lives in VGPR lanes (v_writelane / v_readlane, a VALU slot and wait states
// each, in a VALU-bound kernel, and the VGPRs count against the 128).  So the prologue alone reads the parameters themselves; the
// second loop and the epilogue read the kernarg segment again through an opaque copy of its address (step_args: a scalar load
// where the value is used, served by the scalar cache), values the compiler would compute once in front of the loop and then
// spill (the `!= 0xFF` masks of the entry-route bytes and their hash products, the lane tests of the flat phase and of publish)
// are formed from opaque copies inside it, and a specialised row knows its workgroup size at compile time (BD).  Per-second
// loop of <256, true, false, 2, 1>: 138 v_readlane_b32 and 4482 instructions before, none and 4361 now; no specialised
// instantiation reloads a scalar inside the loop (tools/kernel_regs.py prints the counts; profiles/env_scalar_bench.json).
struct StepArgs {                           // the kernarg segment of step_kernel: its parameters in order
    EnvDev P; const int *action; float *obs; double *reward, *greward; uint8_t *done; int train_mode;
};
using StepArgsPtr = const __attribute__((address_space(4))) StepArgs *;
__device__ __forceinline__ StepArgsPtr step_args() {
    StepArgsPtr k = (StepArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));             // opaque: what is read through it is loaded behind this point
    return k;
}
// compile-time table dimensions over the runtime ones
template <int SPEC>
__device__ __forceinline__ void spec_dims(EnvDev &P) {
    if constexpr (SPEC > 0) {
        constexpr SpecDims D = kSpec[SPEC];
        P.NLP = D.NLP; P.NLA = D.NLA; P.NU = D.NU; P.NR = D.NR; P.A = D.A; P.KMAX = D.KMAX;
        P.PMAX = D.PMAX; P.LMAX = D.LMAX; P.NBR = D.NBR; P.ctrl = D.ctrl; P.yellow = D.yellow; P.teleport = D.teleport;
        P.NS = D.NR;                            // the reference's configurations: every route is its own stream
    }
}
template <int MAXT, bool HELP, bool REC = false, int KF = 4, int SPEC = 0>      // REC: evaluation recording (plain walk only); KF: vehicles per thread and super-round of the flat phase
__global__ void __launch_bounds__(MAXT, MAXT <= 512 ? 4 : 1)      // (HIP: the second figure is wavefronts per SIMD) 128 VGPRs whatever the workgroup size
step_kernel(EnvDev P, const int *__restrict__ action, float *__restrict__ obs, double *__restrict__ reward,
            double *__restrict__ greward, uint8_t *__restrict__ done, int train_mode) {
    constexpr bool KR = SPEC == kSpecKrauss || SPEC == kSpecKraussTrace || SPEC == kSpecKraussLaneData;
    constexpr bool LD = SPEC == kSpecLaneData || SPEC == kSpecKraussLaneData;
    constexpr bool TR = SPEC == kSpecTrace || SPEC == kSpecKraussTrace || LD;
    constexpr bool SER = REC || KR;         // R0 (depart | serial << 16) is kept per slot
    static_assert(!TR || (REC && !HELP), "the trace rides on the recording walk");
    static_assert(offsetof(StepArgs, action) == (sizeof(EnvDev) + 7) / 8 * 8, "StepArgs mirrors the parameter list");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    spec_dims<SPEC>(P);
    const int BD = SPEC > 0 ? MAXT : (int)blockDim.x;       // (plan_step launches a specialised row with exactly its MAXT threads)
    Smem s = carve<KR, LD>(smem_raw, P);
    const int e = P.order ? P.order[blockIdx.x] : (int)blockIdx.x, l = threadIdx.x, NLP = P.NLP, NLA = P.NLA, NR = P.NR, NS = P.NS;
    const bool lane = l < P.NU;             // lanes >= NU are never entered by any route: always empty
    const bool lthr = l < NLA;              // threads >= NLA only help in phase A1 and in the strided loops
    const bool stamp = blockIdx.x == 0 && threadIdx.x == 0;         // (whether stamps are on is read at each stamp: TSC_STAMP)
    int nstamp = 0;
    // A measurement build (-DTSC_ENV_PHASE_SUMS, tools/build_variant.sh) also lets every workgroup's thread 0 sum its shader-clock
    // cycles per kind of phase (tsc_env_debug_clock enable == 3): bucket 0 prologue + epilogue, 1 head walk, 2 flat phase, 3 gather +
    // demand, 4 the barriers between them.  Not in the product build: the sums live in registers over the whole kernel (25 spilled
    // dwords in the benchmarked instantiation).
#ifdef TSC_ENV_PHASE_SUMS
    const bool wsum = P.dbg && threadIdx.x == 0;
    long long pacc_[5] = {0, 0, 0, 0, 0}, wprev = 0;
    int wk = 0;
#define TSC_STAMP() do { if (stamp && nstamp < 62) { long long *d_ = step_args()->P.dbg; if (d_) d_[nstamp++] = clock64(); }   \
        if (wsum) { const long long now_ = clock64();                                                                    \
            if (wk > 0) { const int d_ = wk - 1, r_ = (d_ - 1) % 6;                                                       \
                const int b_ = (d_ == 0 || d_ > 30) ? 0 : (r_ == 0 ? 1 : r_ == 2 ? 2 : r_ == 4 ? 3 : 4); pacc_[b_] += now_ - wprev; } \
            wprev = now_; ++wk; } } while (0)
#else
#define TSC_STAMP() do { if (stamp && nstamp < 62) { long long *d_ = step_args()->P.dbg; if (d_) d_[nstamp++] = clock64(); } } while (0)
#endif
    TSC_STAMP();
    if (P.dbg && threadIdx.x == 0) P.dbg[64 + 2 * blockIdx.x] = wall_clock64();
    float4 *S = P.S + (size_t)e * kCap * NLP;
    static_assert(!(HELP && REC), "recording uses the plain walk");
    uint32_t *R0 = SER ? P.R0 + (size_t)e * kCap * NLP : nullptr, *R1 = REC ? P.R1 + (size_t)e * kCap * NLP : nullptr;
    const float origin = REC && lane ? P.lane_origin[l] : 0.0f;
    if (REC && l < 4) s.rint[l] = 0;
    int tslot = -1, tcur = 0;               // TR: this instance's trace buffer (-1: untraced, the same for the whole workgroup), its cursor
    if constexpr (TR) {
        tslot = (LD && !P.trace_slot) ? -1 : P.trace_slot[e];
        if (tslot >= 0) tcur = P.trace_cnt[(size_t)tslot * (P.episode + 1)];
    }

    // ---- prologue.  Everything is requested in two levels -- first all loads that depend on nothing, then (under
    // the table copies) the ones that need a first-level value -- and unconditionally (lane index clamped), so
    // that the prologue costs a few memory round trips instead of one per table.
    const int lc = lane ? l : P.NU - 1;                                  // clamped lane for the loads
    const bool ag = l < P.A;
    const int ac = ag ? l : P.A - 1;
    // level 1
    const int act = action[(size_t)e * P.A + ac];
    const int prev = P.prev_action[(size_t)e * P.A + ac];
    int n = P.N[(size_t)e * NLP + lc];
    float L_ = P.lane_len[lc], vmax_ = P.lane_vmax[lc], det = P.lane_det[lc];
    int my_node = P.lane_node[lc];
    int up0 = P.lane_up[lc * kMaxUp], up1 = P.lane_up[lc * kMaxUp + 1], up2 = P.lane_up[lc * kMaxUp + 2], up3 = P.lane_up[lc * kMaxUp + 3];
    uint32_t myr_lo = P.lane_routes[lc * 2], myr_hi = P.lane_routes[lc * 2 + 1];     // entry routes, a byte each
    int t = P.tsec[e];
    const uint32_t seed = P.seed[e];
    const int rc = l < NS ? l : NS - 1;
    const int pend0 = P.pending[(size_t)e * NS + rc], ser0 = P.serial[(size_t)e * NS + rc];
    const uint8_t *const emit_tab = P.emit_tab + (size_t)e * P.emit_inst;    // the instance's own table under tsc_env_set_demand
    if (!lane) {
        n = 0; L_ = 1.0f; vmax_ = 1.0f; det = 0.0f; my_node = -1; up0 = up1 = up2 = up3 = -1;
        myr_lo = myr_hi = 0xFFFFFFFFu;
    }
    // table copies: four (clamped, unconditional) loads in flight per thread and round instead of one
    auto copy_words = [&](uint32_t *dst, const uint32_t *src, int count) {
        for (int base = l; base < count; base += 4 * BD) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = base + u * BD; w[u] = src[i < count ? i : count - 1]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = base + u * BD; if (i < count) dst[i] = w[u]; }
        }
    };
    // Round 6: the first 8 / 4 words per thread of the two tables are REQUESTED here, next to the level-1 loads, and stored behind the
    // level-2 requests (one memory round trip for both tables instead of one per 4-word round: three on large_grid -- the workgroup is a
    // latency chain, 64 us alone on a CU against 80 us with three neighbours, so a round trip is ~ 1 % of the step); what does not fit
    // (no reference scenario; tests/test_networks_gpu.py grid_x2, grid_x4) takes the loop.
    constexpr int kTW = 8, kTZ = 4;
    const int n_mv = P.NU * NR, n_zip = (P.NU * NR + 3) / 4;                            // zip padded to 4 B
    uint32_t tw[kTW], tz[kTZ];
#pragma unroll
    for (int u = 0; u < kTW; ++u) { const int i = l + u * BD; tw[u] = ((const uint32_t *)P.mv)[i < n_mv ? i : n_mv - 1]; }
#pragma unroll
    for (int u = 0; u < kTZ; ++u) { const int i = l + u * BD; tz[u] = ((const uint32_t *)P.zip)[i < n_zip ? i : n_zip - 1]; }
    // level 2 (needs n / act / t), issued before the remaining LDS fills
    float hx = 0, hv = 0, hsf = 0, tx = 0, tv = 0; uint32_t hm = 0;      // head record (slot 0) / tail of my lane, kept in registers
    {
        const int nl = n > 0 ? n - 1 : 0;
        const int s0 = vslot(0, lc, NLP), sl = vslot(nl, lc, NLP);
        const float4 a0 = S[s0];
        const float2 al = *(const float2 *)(S + sl);
        if (n > 0) { hx = a0.x; hv = a0.y; hsf = a0.z; hm = __float_as_uint(a0.w); tx = al.x; tv = al.y; }
    }
#pragma unroll
    for (int u = 0; u < kTW; ++u) { const int i = l + u * BD; if (i < n_mv) ((uint32_t *)s.mv)[i] = tw[u]; }
#pragma unroll
    for (int u = 0; u < kTZ; ++u) { const int i = l + u * BD; if (i < n_zip) ((uint32_t *)s.zip)[i] = tz[u]; }
    if (n_mv > kTW * BD) copy_words((uint32_t *)s.mv + kTW * BD, (const uint32_t *)P.mv + kTW * BD, n_mv - kTW * BD);
    if (n_zip > kTZ * BD) copy_words((uint32_t *)s.zip + kTZ * BD, (const uint32_t *)P.zip + kTZ * BD, n_zip - kTZ * BD);
    // K1: signal FSM (envs/env.py:128-152) -> link chars for the yellow and the green interval
    if (ag) {
        P.prev_action[(size_t)e * P.A + l] = act;
        const uint8_t *g = P.green_tab + ((size_t)l * P.PMAX + act) * P.KMAX;
        const uint8_t *y = (prev < 0 || prev == act) ? g : P.yellow_tab + (((size_t)l * P.PMAX + prev) * P.PMAX + act) * P.KMAX;
        for (int k = 0; k < P.KMAX; ++k) { s.link_y[l * P.KMAX + k] = y[k]; s.link_g[l * P.KMAX + k] = g[k]; }
    }
    // per-route insertion state and this step's emissions live in LDS for the duration of the launch
    if (l < NS) {
        s.pend[l] = pend0; s.ser[l] = ser0;
        for (int q = 0; q < 8; ++q) s.emit[l * 8 + q] = q < P.ctrl ? emit_tab[(size_t)l * P.emit_len + t + q] : 0;
    }
    for (int r = BD + l; r < NS; r += BD) {              // more streams than threads (tests/test_networks_gpu.py few_threads)
        s.pend[r] = P.pending[(size_t)e * NS + r]; s.ser[r] = P.serial[(size_t)e * NS + r];
        for (int q = 0; q < 8; ++q) s.emit[r * 8 + q] = q < P.ctrl ? emit_tab[(size_t)r * P.emit_len + t + q] : 0;
    }
    for (int a2 = BD + l; a2 < P.A; a2 += BD) {          // more agents than threads (few_threads as well: its live junctions are agents 70 .. 99)
        const int act2 = action[(size_t)e * P.A + a2], prev2 = P.prev_action[(size_t)e * P.A + a2];
        P.prev_action[(size_t)e * P.A + a2] = act2;
        const uint8_t *g = P.green_tab + ((size_t)a2 * P.PMAX + act2) * P.KMAX;
        const uint8_t *y = (prev2 < 0 || prev2 == act2) ? g : P.yellow_tab + (((size_t)a2 * P.PMAX + prev2) * P.PMAX + act2) * P.KMAX;
        for (int k = 0; k < P.KMAX; ++k) { s.link_y[a2 * P.KMAX + k] = y[k]; s.link_g[a2 * P.KMAX + k] = g[k]; }
    }
    for (int q = l; q < NLA; q += BD) {
        const bool in = q < P.NU;
        s.len[q] = in ? P.lane_len[q] : 1.0f; s.node[q] = in ? P.lane_node[q] : -1; s.vmax[q] = in ? P.lane_vmax[q] : 1.0f;
        int sbq = (in && P.lane_sib) ? P.lane_sib[q] : -1;
        s.sib[q] = sbq < P.NU ? sbq : -1;               // (a sibling no route ever reaches has no rows here and is never needed)
    }
    for (int q = l; q < NLP; q += BD) { s.wave[q] = 0; s.halt[q] = 0; s.hwait[q] = 0; }
    if constexpr (HELP) {                           // flat-phase marks: all clear (a second sets and clears its own)
        uint32_t *mk = (uint32_t *)s.mark;
        for (int q = l; q < (NLA * (kCap - 1) + 8) / 4; q += BD) mk[q] = 0u;
    }
    // publishes a lane's summary for the next second; with HELP also the wave-local inclusive scan of the number
    // of queued vehicles (slots >= 1) that phase A1 distributes over the workgroup
    auto publish = [&]() {
        if (!lthr) return;
        s.n[l] = n; s.hx[l] = hx; s.hv[l] = hv; s.hm[l] = hm; s.tx[l] = tx; s.tv[l] = tv;
        if constexpr (HELP) {
            const int inc = wave_scan_add(n > 1 ? n - 1 : 0);
            s.pre[l] = inc;
            int l6 = l & 63;
            asm volatile("" : "+v"(l6));            // (opaque: a mask of this call, not of the launch)
            if (l6 == 63) s.wtot[l >> 6] = inc;
        }
    };
    publish();
    if (lthr) {
        auto b8 = [&](int u) { return (uint32_t)((u >= 0 && u < 255 && u < P.NU) ? u : 0xFF); };
        s.up4[l] = b8(up0) | b8(up1) << 8 | b8(up2) << 16 | b8(up3) << 24;
        s.nout[l] = 0;
    }
    // LD: the sums of the interval this launch lies in, into LDS (stored back once, behind the last second); my lane's slots
    const int nds = LD ? P.ld_nslot : 0;
    const bool ldon = LD && t < P.episode;
    int *ld_gi = nullptr; double *ld_gs = nullptr;
    int ld_k0 = 0, ld_k1 = 0;
    if constexpr (LD) {
        if (ldon) {
            const int nint = (P.episode + P.ld_period - 1) / P.ld_period;
            const size_t row = (size_t)e * nint + t / P.ld_period;
            ld_gi = P.ld_int + row * kLdInts * nds; ld_gs = P.ld_speed + row * nds;
            if (lane) { ld_k0 = P.ld_slot0[l]; ld_k1 = P.ld_slot0[l + 1]; }
            copy_words((uint32_t *)s.ldi, (const uint32_t *)ld_gi, kLdInts * nds);          // (four loads in flight per thread)
            copy_words((uint32_t *)s.ldsp, (const uint32_t *)ld_gs, 2 * nds);
            copy_words((uint32_t *)s.ldsu, (const uint32_t *)P.ld_sumo, nds);
            copy_words((uint32_t *)s.ldb, (const uint32_t *)P.ld_bound, 4 * P.NU);
            for (int i = l; i < nds; i += BD) s.ldsec[i] = 0.0;
        }
    }
    // the slot of position x on my lane: the last piece that starts at or before x (the first one for any x before it).  A lane of
    // one piece (every lane of large_grid) has it without a look; otherwise four compares against the lane's piece starts.
    auto ld_slot = [&](float x) {
        if (ld_k1 == ld_k0 + 1) return ld_k0;
        const float4 b = s.ldb[l];
        return ld_k0 + (int)(x >= b.x) + (int)(x >= b.y) + (int)(x >= b.z) + (int)(x >= b.w);
    };
    unsigned arrived = 0, tele = 0;
    __syncthreads();
    TSC_STAMP();

    int d_wave = 0, d_halt = 0;                     // detector counts, taken during the last simulated second
#pragma unroll 1
    for (int sub = 0; sub < P.ctrl; ++sub, ++t) {
        const uint8_t *link = sub < P.yellow ? s.link_y : s.link_g;
        const bool last = sub == P.ctrl - 1;
        // ================= phase H (K2): the platoon that crosses in this second and the first vehicle that stays,
        // from the OLD state (without HELP: the whole lane, sequentially) =================
        int kept = 0, nsent = 0;
        bool has_first = false;                        // HELP: the first stayer is written in phase B (its old slot is
        float fxn = 0.0f, fvn = 0.0f, fsf = 0.0f;      // still read by the flat phase)
        uint32_t fmeta = 0u, fr0 = 0u;
        int i0 = 0;
        // recording: this lane's share of the per-second network statistics (envs/env.py:409-437)
        int rq_halt = 0, rq_wait = 0, rq_arr = 0, rq_dep = 0;
        double rq_speed = 0.0;
        auto tally = [&](float xn, float vn, uint32_t nmeta) {
            if constexpr (REC) {
                rq_wait += (int)(nmeta & 0xFFFFu);
                rq_speed += (double)vn;
                if (vn < kHalt && xn >= origin) ++rq_halt;
            }
        };
        // LD: a vehicle of my lane at the end of this second, at xn with speed vn -> its slot, where it is counted.  The counts and
        // the speed sum of the slot the last vehicle was on stay in registers (a lane's vehicles come in queue order, so its slot
        // changes at most once per piece); a change of slot moves them to LDS, and the speed sum continues from the new slot's
        // partial sum of this second, so the sum is the one of the slot's speeds in queue order whatever the order of slots.
        // The run starts on the lane's first slot with a sum of 0.0 (what every slot's sum of the second starts from): on a lane of one
        // piece the slot never changes, and the walk never touches LDS for it.
        const bool ldsec = ldon && t < P.episode;
        int ld_cur = ld_k0, ld_ns = 0, ld_nw = 0;
        double ld_acc = 0.0;
        auto ld_flush = [&]() {
            s.ldsec[ld_cur] = ld_acc;
            s.ldi[kLdSampled * nds + ld_cur] += ld_ns; s.ldi[kLdWaiting * nds + ld_cur] += ld_nw;
            ld_ns = 0; ld_nw = 0;
        };
        auto ld_sample = [&](float xn, float vn) {
            const int k = ld_slot(xn);
            if (k != ld_cur) { ld_flush(); ld_cur = k; ld_acc = s.ldsec[k]; }
            ++ld_ns;
            if (vn < kHalt) ++ld_nw;
            ld_acc += (double)vn;
            return k;
        };
        if constexpr (HELP) {
            // flat order of the queued vehicles (slots >= 1) of the instance, lane after lane: this lane's first flat index P0
            // (wave-local inclusive scan from publish() + the totals of the lane wavefronts before mine), a mark at P0 and the
            // owner of the one multiple of 64 its <= 27 vehicles can cover -- what the flat phase needs to turn a flat index
            // into (lane, slot) with one LDS read, a wavefront max-scan and one more read (a 6-step binary search per vehicle
            // before round 4)
            if (lthr) {
                const int c = n > 1 ? n - 1 : 0;
                int P0 = s.pre[l] - c;
                int lw = l >> 6;
                asm volatile("" : "+v"(lw));                // (opaque: the loop's entry test would be a mask held, and spilled, for the launch)
                for (int w = 0; w < NLA / 64 - 1; ++w) P0 += w < lw ? s.wtot[w] : 0;
                s.pre[l] = P0;
                if (c > 0) {
                    s.mark[P0] = (uint8_t)((l & 63) + 1);
                    const int m64 = (P0 + c - 1) & ~63;
                    if (m64 >= P0) s.bound[m64 >> 6] = (uint16_t)(l + 1);
                }
            }
            // From here on the lane wavefronts walk their heads (phase H) while every other wavefront already starts the flat
            // phase's first half (locate, load, car-following: old state only) -- the two only meet at the barrier in front of
            // the chain keys (round 4; before, all helper wavefronts idled through phase H).
            __syncthreads();
        }
        if (lane) {
            // lane constants from LDS per phase (HELP): two registers less across the flat phase than holding them for the launch
            const float L = HELP ? s.len[l] : L_, vmax = HELP ? s.vmax[l] : vmax_;
            int ncross = 0;
            bool all_crossed = true;
            float pnx = INFINITY, pox = 0.0f, pov = 0.0f;
            float K = INFINITY;                            // plain walk: running min of the chain keys (MICROSIM_SPEC.md rule 4)
            // a vehicle that stays on the lane: compact it to slot `kept`, refresh the summary, count detectors
            auto keep = [&](float xn, float vn, float sf, uint32_t nmeta, uint32_t r0 = 0u, uint32_t r1 = 0u) {
                const unsigned ob = (unsigned)vslot(kept, l, NLP) * 4u;
                stg(S, 4u * ob, make_float4(xn, vn, sf, __uint_as_float(nmeta)));
                if constexpr (REC) { stg(R0, ob, r0); stg(R1, ob, r1); tally(xn, vn, nmeta); }
                else if constexpr (KR) stg(R0, ob, r0);
                if (kept == 0) { hx = xn; hv = vn; hsf = sf; hm = nmeta; }
                tx = xn; tv = vn;
                ++kept;
                if (last && xn >= det) { ++d_wave; if (vn < kHalt) ++d_halt; }
            };
            // ---- head walk: full evaluation.  Without HELP it covers the whole lane; with HELP only the platoon
            // that is crossing in this second plus the first vehicle that stays (everything behind it is phase A1).
            struct Raw { float x, v, sf; uint32_t m, r0, r1; };
            // Loads are UNCONDITIONAL (slot index clamped; every slot is allocated): the compiler can only keep a
            // load in flight across the evaluation of the previous vehicle (s_waitcnt vmcnt(N > 0)) when the
            // number of younger memory operations is known, which a load under `if (i < n)` destroys.
            auto load_raw = [&](int i) {
                const unsigned ob = (unsigned)vslot(i < kCap ? i : kCap - 1, l, NLP) * 4u;
                const float4 a4 = ldg(S, 4u * ob);
                Raw r; r.x = a4.x; r.v = a4.y; r.sf = a4.z; r.m = __float_as_uint(a4.w);
                r.r0 = 0u; r.r1 = 0u;
                if constexpr (REC) { r.r0 = ldg(R0, ob); r.r1 = ldg(R1, ob); }
                else if constexpr (KR) r.r0 = ldg(R0, ob);
                return r;
            };
            int i = 0;
            // the head's record is what this thread wrote last (hx / hv / hsf / hm track slot 0): with HELP the walk starts from the
            // registers instead of waiting for a load of it -- one memory round trip less on the second's critical path
            Raw cur;
            if constexpr (HELP && !REC) {
                cur.x = hx; cur.v = hv; cur.sf = hsf; cur.m = hm; cur.r0 = 0u; cur.r1 = 0u;
                if constexpr (KR) cur.r0 = ldg(R0, (unsigned)vslot(0, l, NLP) * 4u);
            }
            else cur = load_raw(0);
            for (; i < n; ++i) {
                if (HELP && !all_crossed) break;
                const Raw nxt = load_raw(i + 1);
                const float x = cur.x, v = cur.v, sf = cur.sf;
                const uint32_t meta = cur.m;
                int w = (int)(meta & 0xFFFFu);
                const int r = (int)(meta >> 16);
                const int mvp = s.mv[l * NR + r];
                const int tl = mv_tl(mvp), k = mv_k(mvp), y = mv_yield(mvp), z = s.zip[l * NR + r];
                const float v0 = vmax * sf;
                const bool sink = tl == -1;
                const bool open = sig_open(tl, k, HELP ? s.node[l] : my_node, w, x, v, L, link, P.KMAX, P.teleport);
                bool can_cross = false, lc = false;
                int sb = -1;                                   // rule 10: the sibling lane this vehicle has to move over to
                if (all_crossed) {
                    can_cross = open;
                    if (can_cross && y >= 0 && w < P.teleport && s.n[y] > 0) {
                        // right of way: wait while the yield lane's head has an open priority movement and is near
                        const uint32_t om = s.hm[y];
                        const int mo = s.mv[y * NR + (int)(om >> 16)];
                        if (mv_prio(mo)) {
                            const float xo = s.hx[y], vo = s.hv[y], Lo = s.len[y];
                            if (sig_open(mv_tl(mo), mv_k(mo), s.node[y], (int)(om & 0xFFFFu), xo, vo, Lo, link, P.KMAX, P.teleport)) {
                                const float d = Lo - xo;
                                if (d < vo * kYieldT + kYieldD) can_cross = false;
                            }
                        }
                    }
                    // zipper merge by readiness: of the feeders of tl whose HEAD wants tl, sees an open signal and can reach
                    // its stop line within this second, the one with the smallest rotating rank (t + rank) % count sends
                    // (large_grid, SPEC 1, has no unsignalised merge: its zip table is all zero, checked at create time; zippers of
                    // three and four feeders under signals, next to teleporting heads: tests/test_networks_random_gpu.py)
                    if (SPEC != 1 && can_cross && (z >> 4) > 1) {
                        const uint32_t ups = s.up4[tl];
                        int best = -1, bestp = 1 << 30;
#pragma unroll
                        for (int u = 0; u < kMaxUp; ++u) {
                            const int f = (int)((ups >> (8 * u)) & 0xFFu);
                            if (f == 0xFF || s.n[f] == 0) continue;
                            const uint32_t om = s.hm[f];
                            const int ro = (int)(om >> 16), mo = s.mv[f * NR + ro];
                            if (mv_tl(mo) != tl) continue;
                            const int zo = s.zip[f * NR + ro], cnt = zo >> 4;
                            if (cnt <= 1) continue;
                            const float xo = s.hx[f], vo = s.hv[f], Lo = s.len[f];
                            if (!sig_open(tl, mv_k(mo), s.node[f], (int)(om & 0xFFFFu), xo, vo, Lo, link, P.KMAX, P.teleport)) continue;
                            if (!((Lo - xo) < vo + kAcc)) continue;
                            const int pr = (t + (zo & 0xF)) % cnt;
                            if (pr < bestp) { bestp = pr; best = f; }
                        }
                        if (best != l) can_cross = false;
                    }
                    if (can_cross && tl >= 0 && s.n[tl] + kMaxCross > kCap) can_cross = false;
                    if (can_cross && tl >= 0 && s.n[tl] > 0 && s.tx[tl] < kLen) can_cross = false;   // no room behind the tail
                    if (can_cross && ncross >= kMaxCross) can_cross = false;
                    if (tl < -1) can_cross = false;
                    // rule 10: a head-platoon vehicle on the wrong lane of a two-lane street moves over to the sibling lane as a
                    // hand-off that keeps its position: behind the sibling's OLD tail by the standstill gap + 1 s of the closing
                    // speed, room for two full platoons there (the sibling may receive from its junction in the same second)
                    if (tl < -1) {
                        const int sq = s.sib[l];
                        if (sq >= 0 && mv_tl(s.mv[sq * NR + r]) >= -1) {
                            sb = sq;
                            const int nsb = s.n[sb];
                            lc = (nsb + 2 * kMaxCross <= kCap) && (ncross < kMaxCross);
                            if (lc && nsb > 0) {
                                float dv = v - s.tv[sb];
                                if (dv < 0.0f) dv = 0.0f;
                                lc = ((s.tx[sb] - kLen) - x) >= (kS0 + dv);
                            }
                        }
                    }
                }
                // teleport (SUMO --time-to-teleport): the head, standing for >= teleport seconds, whose way is still blocked
                // (merge slot, capacity, no room behind the target's tail) leaves the network where it stands.  SUMO would
                // move it along its route and its trip would end later: the surrogate TRUNCATES the trip, so it is counted
                // as a teleport, not as an arrival, and its trip row carries a negative arrival second
                if (i == 0 && !can_cross && !lc && (tl >= 0 || sb >= 0) && w >= P.teleport) {
                    ++tele;
                    if constexpr (LD) { if (ldsec) ++s.ldi[kLdTeleported * nds + ld_slot(x)]; }
                    if constexpr (REC) {
                        const int k = atomicAdd(&P.n_trips[e], 1);
                        if (k < P.trip_cap) {
                            int *tr = P.trips + ((size_t)e * P.trip_cap + k) * 6;
                            tr[0] = r; tr[1] = (int)(cur.r0 >> 16); tr[2] = (int)(cur.r0 & 0xFFFFu); tr[3] = -(t + 1);
                            tr[4] = (int)(cur.r1 & 0xFFFFu); tr[5] = (int)(cur.r1 >> 16);
                        }
                    }
                    ++ncross;
                    pox = x; pov = v;
                    cur = nxt;
                    continue;
                }
                // (rule 10: a lane change is a hand-off to the sibling lane `sb` at distance 0 instead of L - x, with the stop line
                //  closed -- no lane change and junction crossing in one second; it shares the evaluation below)
                const bool line_block = lc || (all_crossed ? !can_cross : !open);
                const bool tgt_lead = lc ? s.n[sb] > 0 : (can_cross && !sink && s.n[tl] > 0);
                const int tq = tgt_lead ? (lc ? sb : tl) : 0;      // the lane whose old tail is the leader of the lane's head
                const float Lq = lc ? 0.0f : L;                    // distance to that lane's start
                // leader: vehicle ahead (old state), else the old tail of the target lane, else free road; the stop line
                // is a second leader when the link is closed (evaluating both branch-free was measured no faster and
                // costs 40 VGPRs)
                const bool has_lead = i > 0 || tgt_lead;
                const float lg = i > 0 ? (pox - kLen) - x : (Lq - x) + (s.tx[tq] - kLen);
                const float lvl = i > 0 ? pov : s.tv[tq];
                float vn = follow<KR>(v, v0, has_lead, lg, lvl, kS0);
                if (line_block) {
                    const float v2 = follow<KR>(v, v0, true, L - x, 0.0f, 0.0f);
                    if (v2 < vn) vn = v2;
                }
                // rule 10: the head of a lane that has to move over lines up BEHIND the sibling's queue instead of driving past
                // it: the sibling's old tail is a third leader while it is still ahead
                if (sb >= 0 && !lc && i == 0 && s.n[sb] > 0) {
                    const float g3 = (s.tx[sb] - kLen) - x;
                    if (g3 >= 0.0f) {
                        const float v3 = follow<KR>(v, v0, true, g3, s.tv[sb], kS0);
                        if (v3 < vn) vn = v3;
                    }
                }
                if constexpr (KR) {
                    if (P.sigma > 0.0f) vn = dawdle(vn, P.sigma, seed, (uint32_t)r, cur.r0 >> 16, (uint32_t)t);
                }
                float xn = x + vn;
                if (!HELP && !all_crossed) {
                    // behind the first vehicle that stays: x' = min(x + v', L, K - 5 i), K = exclusive prefix-min of the
                    // keys a_j + 5 j (the closed form of x'_i = min(a_i, x'_{i-1} - 5); the flat phase scans it)
                    const float xf = xn;
                    float a = xf;
                    if (a > L) a = L;
                    const float lim = K - (float)(5 * i);
                    xn = a < lim ? a : lim;
                    if (xn < x) xn = x;
                    if (xn != xf) vn = xn - x;
                    const float key = a + (float)(5 * i);
                    if (key < K) K = key;
                } else {
                    bool clamped = false;
                    if (xn > pnx - kLen) { xn = pnx - kLen; clamped = true; }
                    if (tgt_lead) {
                        const float lim = Lq + (s.tx[tq] - kLen);
                        if (xn > lim) { xn = lim; clamped = true; }
                    }
                    if (can_cross && !sink) {                          // target lane shorter than one step's travel
                        const float far = L + s.len[tl];
                        if (xn > far) { xn = far; clamped = true; }
                    }
                    if (!can_cross && xn > L) { xn = L; clamped = true; }
                    if (xn < x) { xn = x; clamped = true; }
                    if (clamped) vn = xn - x;
                }
                uint32_t r1n = cur.r1;
                if constexpr (REC) {                   // tripinfo waitingTime / waitingCount
                    if (vn < kHalt) r1n = (r1n + 1u) + (w == 0 ? 0x10000u : 0u);
                }
                w = (vn < kHalt) ? w + 1 : 0;
                pnx = xn; pox = x; pov = v;
                const uint32_t nmeta = (uint32_t)w | ((uint32_t)r << 16);
                if (lc) {                                   // rule 10: over to the sibling lane, position kept
                    const int o = nsent * NLA + l;
                    s.ox[o] = xn; s.ov[o] = vn; s.osf[o] = sf; s.om[o] = nmeta; s.oto[o] = sb;
                    if constexpr (LD) { if (ldsec) s.oto[o] = sb | 0x8000 | ld_slot(x) << 16; }   // LD: lane change (bit 15) from the old slot
                    if constexpr (REC) { s.or0[o] = cur.r0; s.or1[o] = r1n; }
                    else if constexpr (KR) s.or0[o] = cur.r0;
                    ++nsent; ++ncross;
                } else if (can_cross && xn >= L) {
                    if (!sink) {
                        const int o = nsent * NLA + l;
                        const float ex = xn - L, Lt = s.len[tl];          // rounding of (L + Lt) - L
                        s.ox[o] = ex > Lt ? Lt : ex; s.ov[o] = vn; s.osf[o] = sf; s.om[o] = nmeta; s.oto[o] = tl;
                        if constexpr (LD) { if (ldsec) s.oto[o] = tl | ld_slot(x) << 16; }
                        if constexpr (REC) { s.or0[o] = cur.r0; s.or1[o] = r1n; }
                        else if constexpr (KR) s.or0[o] = cur.r0;
                        ++nsent;
                    } else {
                        ++arrived;
                        if constexpr (LD) { if (ldsec) ++s.ldi[kLdArrived * nds + ld_slot(x)]; }
                        if constexpr (REC) {
                            ++rq_arr;
                            const int k = atomicAdd(&P.n_trips[e], 1);
                            if (k < P.trip_cap) {
                                int *tr = P.trips + ((size_t)e * P.trip_cap + k) * 6;
                                tr[0] = r; tr[1] = (int)(cur.r0 >> 16); tr[2] = (int)(cur.r0 & 0xFFFFu); tr[3] = t + 1;
                                tr[4] = (int)(r1n & 0xFFFFu); tr[5] = (int)(r1n >> 16);
                            }
                        }
                    }
                    ++ncross;
                } else {
                    if (all_crossed) K = xn + (float)(5 * i);      // the first vehicle that stays seeds the chain
                    all_crossed = false;
                    if constexpr (HELP) {
                        has_first = true; i0 = i; fxn = xn; fvn = vn; fsf = sf; fmeta = nmeta; fr0 = cur.r0;
                        if (last && xn >= det) { ++d_wave; if (vn < kHalt) ++d_halt; }
                    } else {
                        keep(xn, vn, sf, nmeta, cur.r0, r1n);
                        if constexpr (LD) {
                            if (ldsec) {                           // onto the next piece of a contracted lane: left / entered
                                const int ko = ld_slot(x), kn = ld_sample(xn, vn);
                                if (ko != kn && s.ldsu[ko] != s.ldsu[kn]) { ++s.ldi[kLdLeft * nds + ko]; ++s.ldi[kLdEntered * nds + kn]; }
                            }
                        }
                    }
                }
                cur = nxt;
            }
            if constexpr (HELP) {
                if (!has_first) i0 = n;                            // everybody crossed
                s.nc[l] = i0;
                s.seed[l] = has_first ? fxn + (float)(5 * i0) : INFINITY;
            }
            s.nout[l] = nsent;
        }
        TSC_STAMP();
        if constexpr (!HELP) __syncthreads();          // (HELP: the barrier sits inside the flat phase, behind its first half)
        TSC_STAMP();
        // ================= phase F (K2, HELP): every vehicle behind the first stayer, one per thread slot =============
        // Nobody behind a vehicle that stays can cross, so such a vehicle's new speed depends only on OLD state (itself, the
        // vehicle ahead, the signal) and its new position on the chain clamp x'_i = min(a_i, x'_{i-1} - 5), a_i = min(x_i +
        // v'_i, L).  The clamp is an exclusive prefix-min over the keys a_j + 5 j within a lane (MICROSIM_SPEC.md rule 4): all
        // queued vehicles of the instance are laid out flat over the workgroup (prefix sum of the lane counts, lane marks +
        // a prefix maximum to find a flat index's lane), kF consecutive ones per thread, and the chain is a segmented
        // min-scan -- in the thread, then over the wavefront on the DPP path, then across wavefronts through one LDS word
        // per wave (a lane's <= 27 queued vehicles touch at most two wavefronts).  Replaces the A1 scratch round trip
        // through HBM and the 28-deep sequential lane walk of round 1.
        if constexpr (HELP) {
            const int nseg = NLA >> 6;
            int total = 0;
            for (int w = 0; w < nseg; ++w) total += s.wtot[w];
            constexpr int kF = KF;
            // flat-phase thread index: rotated so that the lane wavefronts (busy with phase H first) own the LAST flat indices
            // (from an opaque copy of the thread index: the phase's lane tests -- first / last lane of a wavefront, first / last thread --
            //  are masks of this phase, not of the launch)
            int lo = l;
            asm volatile("" : "+v"(lo));
            const int lf = BD > NLA ? (lo >= NLA ? lo - NLA : lo + (BD - NLA)) : lo;
            const int wv = lf >> 6, wl = lf & 63, nwv = BD >> 6;
            int round = 0;
            for (int base = 0; base < total; base += kF * BD, ++round) {
                const float carry_round = round > 0 ? s.wtail[((round - 1) & 1) * 16 + nwv - 1] : INFINITY;
                // A wavefront whose first flat index is past the total has no vehicle in this (last) super-round: it only
                // keeps the barrier.  The kernel is VALU-issue bound and the four workgroups of a CU share its SIMDs, so the
                // ~600 instructions such a wave would run on clamped indices are real time for the others (on average half a
                // super-round: 17-25 % of the phase at 2-3 super-rounds).
                const bool wave_on = base + kF * (int)((unsigned)lf & ~63u) < total;
                int eq[kF], ei[kF];
                float x[kF], v[kF], sf[kF], px[kF], pv[kF];
                uint32_t m[kF], sr[kF];
                bool act[kF];
                float vn[kF], a[kF], key[kF], loc[kF];
                bool run0[kF];
                float pvs = INFINITY;
                int pfs = 1;
#pragma unroll
                for (int u = 0; u < kF; ++u) {
                    eq[u] = 0; ei[u] = 0; x[u] = v[u] = sf[u] = px[u] = pv[u] = 0.0f; m[u] = 0u; sr[u] = 0u; act[u] = false;
                    vn[u] = a[u] = 0.0f; key[u] = loc[u] = INFINITY; run0[u] = true;
                }
                if (wave_on) {
                    // flat index -> (lane, slot): the owner of index k is the last lane whose mark lies at or before k.  Marks hold
                    // the lane's index within its wavefront (a byte); the wavefront comes from the segment the index falls into, so
                    // the owners are increasing along the flat order and a prefix maximum finds them.
                    int kks[kF], val[kF];
    #pragma unroll
                    for (int u = 0; u < kF; ++u) {
                        const int k = base + kF * lf + u;
                        act[u] = k < total;
                        const int kk = act[u] ? k : total - 1;        // clamped: locate and load unconditionally
                        kks[u] = kk;
                        int w = 0, kr = kk;
                        for (; w < nseg - 1; ++w) {
                            const int c = s.wtot[w];
                            if (kr < c) break;
                            kr -= c;
                        }
                        const int m = (int)s.mark[kk];
                        val[u] = m ? (w << 6) + m : 0;
                    }
                    int lmax[kF], rmax = 0;
    #pragma unroll
                    for (int u = 0; u < kF; ++u) { rmax = max(rmax, val[u]); lmax[u] = rmax; }
                    const int incl = wave_scan_max(rmax);
                    int excl = TSC_DPP_I(0, incl, kDppWaveShr1, 0xF);                      // lanes before me; lane 0: none
                    excl = max(excl, (int)s.bound[(base >> 6) + kF * (lf >> 6)]);           // owner of this wavefront's first index
    #pragma unroll
                    for (int u = 0; u < kF; ++u) {
                        const int q = max(lmax[u], excl) - 1;
                        const int i = kks[u] - s.pre[q] + 1;
                        eq[u] = q; ei[u] = i;
                        const unsigned ob = (unsigned)vslot(i, q, NLP) * 4u, pb = (unsigned)vslot(i - 1, q, NLP) * 4u;
                        const float4 a4 = ldg(S, 4u * ob);
                        const float2 p2 = ldg((const float2 *)S, 4u * pb);
                        x[u] = a4.x; v[u] = a4.y; sf[u] = a4.z; m[u] = __float_as_uint(a4.w);
                        px[u] = p2.x; pv[u] = p2.y;
                        if constexpr (KR) sr[u] = ldg(R0, ob);
                    }
                    if (round > 0 && lf == 0 && ei[0] > 1) { px[0] = s.hz[0]; pv[0] = s.hz[1]; }   // overwritten by the previous super-round
    #pragma unroll
                    for (int u = 0; u < kF; ++u) {
                        const int q = eq[u];
                        const float Lq = s.len[q];
                        const int mvp = s.mv[q * NR + (int)(m[u] >> 16)];
                        const float v0 = s.vmax[q] * sf[u];
                        const bool open = sig_open(mv_tl(mvp), mv_k(mvp), s.node[q], (int)(m[u] & 0xFFFFu), x[u], v[u], Lq, link, P.KMAX, P.teleport);
                        float vv = follow<KR>(v[u], v0, true, (px[u] - kLen) - x[u], pv[u], kS0);
                        if (!open) {
                            const float v2 = follow<KR>(v[u], v0, true, Lq - x[u], 0.0f, 0.0f);
                            if (v2 < vv) vv = v2;
                        }
                        if constexpr (KR) {
                            if (P.sigma > 0.0f) vv = dawdle(vv, P.sigma, seed, m[u] >> 16, sr[u] >> 16, (uint32_t)t);
                        }
                        vn[u] = vv;
                        float aa = x[u] + vv;
                        if (aa > Lq) aa = Lq;
                        a[u] = aa;
                    }
                }
                // ---- everything above used OLD state only; what follows needs phase H's results (nc, seed) of this second
                if (round == 0) __syncthreads();
                if (wave_on) {
                    float run = INFINITY;
                    bool first_run = true;
    #pragma unroll
                    for (int u = 0; u < kF; ++u) {
                        const int q = eq[u];
                        const float aa = a[u];
                        const bool live = act[u] && ei[u] > s.nc[q];
                        act[u] = live;
                        key[u] = live ? aa + (float)(5 * ei[u]) : INFINITY;
                        if (u > 0 && eq[u] != eq[u - 1]) { run = INFINITY; first_run = false; }
                        loc[u] = run; run0[u] = first_run;
                        run = fminf(run, key[u]);
                    }
                    // segmented inclusive min-scan of the threads' last runs over the wavefront
                    float sv = run;
                    int sfl = (!first_run || ei[0] == 1) ? 1 : 0;
                    wave_seg_scan_min(sv, sfl);
                    pvs = TSC_DPP_F(sv, sv, kDppWaveShr1, 0xF);       // lane 0 keeps its own value (not read: its carry is the
                    pfs = TSC_DPP_I(sfl, sfl, kDppWaveShr1, 0xF);     // previous wavefront's tail)
                    if (wl == 63) s.wtail[(round & 1) * 16 + wv] = sv;
                }
                if (lf == BD - 1) { s.hz[2] = x[kF - 1]; s.hz[3] = v[kF - 1]; }
                __syncthreads();
                if (lf == 0) { s.hz[0] = s.hz[2]; s.hz[1] = s.hz[3]; }      // read by flat thread 0 after the next barrier only
                const float prev_tail = wv > 0 ? s.wtail[(round & 1) * 16 + wv - 1] : carry_round;
                const float carry = ei[0] > 1 ? (wl == 0 ? prev_tail : (pfs ? pvs : fminf(pvs, prev_tail))) : INFINITY;
#pragma unroll
                for (int u = 0; u < kF; ++u) {
                    if (!act[u]) continue;
                    const int q = eq[u], i = ei[u];
                    const float Kp = fminf(s.seed[q], fminf(run0[u] ? carry : INFINITY, loc[u]));
                    const float xf = x[u] + vn[u];
                    const float lim = Kp - (float)(5 * i);
                    float xn = a[u] < lim ? a[u] : lim;
                    if (xn < x[u]) xn = x[u];
                    float vv = vn[u];
                    if (xn != xf) vv = xn - x[u];
                    const uint32_t w = (vv < kHalt) ? (m[u] & 0xFFFFu) + 1u : 0u;
                    const uint32_t nmeta = w | (m[u] & 0xFFFF0000u);
                    const int shift = s.nc[q];
                    const unsigned ob = (unsigned)vslot(i - shift, q, NLP) * 4u;
                    stg(S, 4u * ob, make_float4(xn, vv, sf[u], __uint_as_float(nmeta)));
                    if constexpr (KR) stg(R0, ob, sr[u]);
                    if (i == s.n[q] - 1) { s.tx[q] = xn; s.tv[q] = vv; }
                    if (last && xn >= step_args()->P.lane_det[q]) { atomicAdd(&s.wave[q], 1); if (vv < kHalt) atomicAdd(&s.halt[q], 1); }
                }
                if (base + kF * BD < total) __syncthreads();     // next super-round reads what this one stored
            }
            TSC_STAMP();
            __syncthreads();
            TSC_STAMP();
            {   // this second's marks all lie below `total`: clear them for the next one (which sets its own after the next barrier)
                uint32_t *mk = (uint32_t *)s.mark;
                for (int q = l; q < (total + 3) / 4; q += BD) mk[q] = 0u;
            }
        }
        // ================= phase B (K3): gather hand-offs from feeder lanes, then demand =========
        if (lane) {
            if constexpr (HELP) {
                // the first vehicle that stays becomes slot 0 now that nobody reads its old slot any more; the rest of the
                // lane was compacted behind it by the flat phase
                kept = has_first ? n - i0 : 0;
                if (has_first) {
                    const unsigned ob0 = (unsigned)vslot(0, l, NLP) * 4u;
                    stg(S, 4u * ob0, make_float4(fxn, fvn, fsf, __uint_as_float(fmeta)));
                    if constexpr (KR) stg(R0, ob0, fr0);
                    hx = fxn; hv = fvn; hsf = fsf; hm = fmeta;
                    if (kept >= 2) { tx = s.tx[l]; tv = s.tv[l]; } else { tx = fxn; tv = fvn; }
                }
            }
            n = kept;
            uint32_t ups = 0xFFFFFFFFu;
            if constexpr (SPEC > 0) ups = s.up4[l];          // the feeders as bytes (0xFF = none): four registers less across the flat phase
            for (int u = 0; u < kMaxUp; ++u) {
                int src;
                if constexpr (SPEC > 0) { src = (int)((ups >> (8 * u)) & 0xFFu); if (src == 0xFF) src = -1; }
                else src = u == 0 ? up0 : u == 1 ? up1 : u == 2 ? up2 : up3;
                if (src < 0) continue;
                const int cnt = s.nout[src];
                for (int j = 0; j < cnt; ++j) {
                    const int o = j * NLA + src;
                    const int to = s.oto[o];
                    if ((LD ? (to & 0x7FFF) : to) == l && n < kCap) {
                        const int d = vslot(n, l, NLP);
                        float ax = s.ox[o];
                        const float av = s.ov[o];
                        const uint32_t am = s.om[o];
                        if (n > 0 && ax > tx - kLen) {                   // arrivals of two feeders in one second (yielding feeders of
                                                                         // one lane: tests/test_networks_random_gpu.py, half of its networks)
                            ax = tx - kLen;
                            if (ax < 0.0f) ax = 0.0f;
                        }
                        S[d] = make_float4(ax, av, s.osf[o], __uint_as_float(am));
                        if constexpr (REC) { R0[d] = s.or0[o]; R1[d] = s.or1[o]; tally(ax, av, am); }
                        else if constexpr (KR) R0[d] = s.or0[o];
                        if constexpr (LD) {
                            if (ldsec) {                           // the source's old slot rode in the upper half of `to`
                                const int kn = ld_sample(ax, av), ko = to >> 16;
                                if (to & 0x8000) { ++s.ldi[kLdLcTo * nds + kn]; atomicAdd(&s.ldi[kLdLcFrom * nds + ko], 1); }
                                else if (s.ldsu[ko] != s.ldsu[kn]) { ++s.ldi[kLdEntered * nds + kn]; atomicAdd(&s.ldi[kLdLeft * nds + ko], 1); }
                            }
                        }
                        if (n == 0) { hx = ax; hv = av; hsf = s.osf[o]; hm = am; }
                        tx = ax; tv = av;
                        ++n;
                        if (last && ax >= det) { ++d_wave; if (av < kHalt) ++d_halt; }
                    }
                }
            }
            uint32_t rlo = myr_lo, rhi = myr_hi;
            asm volatile("" : "+v"(rlo), "+v"(rhi));            // (opaque: the bytes' tests and hash terms are formed here, every second)
#pragma unroll
            for (int q = 0; q < kMaxEntry; ++q) {               // my entry routes, ascending (packed: 0xFF ends the list)
                const int r = (int)(((q < 4 ? rlo : rhi) >> (8 * (q & 3))) & 0xFFu);
                if (r == 0xFF) break;
                int pend = s.pend[r] + (int)s.emit[r * 8 + sub];
                int ser = s.ser[r];
                if (pend > 0 && n < kCap) {
                    const float L = HELP ? s.len[l] : L_;
                    const float xt = n > 0 ? tx : (L + kLen) + kS0;
                    float xmax = (xt - kLen) - kS0;
                    float xlo = kLen;
                    const float *const sorigin = SPEC != 1 ? step_args()->P.sorigin : nullptr;
                    if (SPEC != 1 && sorigin) {                      // the SUMO entry lane is one piece of this (contracted) lane
                        xlo = sorigin[2 * r] + kLen;
                        const float hi = sorigin[2 * r + 1];
                        if (xmax > hi) xmax = hi;
                    }
                    if (!(xmax < xlo)) {
                        const float u0 = u01(hash32(seed, (uint32_t)r, (uint32_t)ser, 0));
                        const float u1 = u01(hash32(seed, (uint32_t)r, (uint32_t)ser, 1));
                        const float u2 = u01(hash32(seed, (uint32_t)r, (uint32_t)ser, 2));
                        const float ax = xlo + u0 * (xmax - xlo);
                        const float asf = 1.0f + 0.2f * ((u1 + u2) - 1.0f);
                        int rt = r;                                  // the vehicle's route: the stream itself, ...
                        if (SPEC <= 0 && P.sroute) {                 // (the specialised instantiations have one-to-one streams)
                            const int md = P.smode[r];
                            rt = P.sroute[r];                        // ... the stream's fixed route, ...
                            if (md == 2) rt = P.iroute[(size_t)e * NS + r];      // ... this episode's draw of the host, ...
                            if (md == 1) {                           // ... or this vehicle's draw from the turn ratios
                                const int u16 = (int)(hash32(seed, (uint32_t)r, (uint32_t)ser, 3) >> 16);
                                const int iv = t / P.ilen < P.NI ? t / P.ilen : P.NI - 1;
                                const int *ch = P.schoice + ((size_t)r * P.NI + iv) * P.KC * 2;
                                rt = ch[0];
                                for (int c = 0; c < P.KC; ++c) {
                                    if (ch[2 * c] < 0) break;
                                    rt = ch[2 * c];
                                    if (u16 < ch[2 * c + 1]) break;
                                }
                            }
                        }
                        const uint32_t am = (uint32_t)rt << 16;
                        const int d = vslot(n, l, NLP);
                        S[d] = make_float4(ax, 0.0f, asf, __uint_as_float(am));
                        if constexpr (REC) { R0[d] = (uint32_t)t | ((uint32_t)ser << 16); R1[d] = 0u; tally(ax, 0.0f, am); ++rq_dep; }
                        else if constexpr (KR) R0[d] = (uint32_t)t | ((uint32_t)ser << 16);
                        if constexpr (LD) { if (ldsec) ++s.ldi[kLdDeparted * nds + ld_sample(ax, 0.0f)]; }
                        if (n == 0) { hx = ax; hv = 0.0f; hsf = asf; hm = am; }
                        tx = ax; tv = 0.0f;
                        ++n;
                        if (last && ax >= det) { ++d_wave; ++d_halt; }
                        --pend;
                        ++ser;
                    }
                }
                s.pend[r] = pend; s.ser[r] = ser;               // a route has exactly one entry lane: no race
            }
            if constexpr (LD) {                                  // this second's speed sums into the interval's, second after second
                if (ldsec) {
                    ld_flush();
                    for (int k = ld_k0; k < ld_k1; ++k) { s.ldsp[k] += s.ldsec[k]; s.ldsec[k] = 0.0; }
                }
            }
        }
        publish();
        if constexpr (REC) {
            if (lthr) { s.rq[l] = rq_halt; s.rsp[l] = rq_speed; }
            if (lane) {
                atomicAdd((unsigned long long *)&s.rint[0], (unsigned long long)n); atomicAdd((unsigned long long *)&s.rint[1], (unsigned long long)rq_dep);
                atomicAdd((unsigned long long *)&s.rint[2], (unsigned long long)rq_arr); atomicAdd((unsigned long long *)&s.rint[3], (unsigned long long)rq_wait);
            }
        }
        TSC_STAMP();
        __syncthreads();
        TSC_STAMP();
        if constexpr (REC) {
            // flush second `sub` of this control step: integers, speed (per-lane partial sums added in lane order: the
            // oracle's association), halting vehicles of every incoming lane in (agent, lane) order
            const size_t row = (size_t)e * 8 + sub;
            if (l < 4) P.rec_int[row * 4 + l] = s.rint[l];
            if (l == 0) {
                double sp = 0.0;
                for (int q = 0; q < P.NU; ++q) sp += s.rsp[q];
                P.rec_speed[row] = sp;
            }
            for (int p2 = l; p2 < P.A * P.LMAX; p2 += BD) {
                const int ln = P.agent_lanes[p2];
                P.rec_queue[row * (P.A * P.LMAX) + p2] = (ln >= 0 && ln < P.NU) ? s.rq[ln] : 0;
            }
            if constexpr (TR) {
                if (tslot >= 0 && t < P.episode) {
                    // per-vehicle rows of second t (tsc_env_trace).  The lanes' first rows: an exclusive prefix sum of the lane counts
                    // (wavefront scan, one LDS word per wavefront; s.pre / s.wtot belong to the flat phase, which the recording walk
                    // does not run), then the rows flat over all threads -- consecutive threads write consecutive 16-byte rows.
                    if (lthr) {
                        const int c = lane ? n : 0;
                        const int inc = wave_scan_add(c);
                        s.pre[l] = inc - c;
                        if ((l & 63) == 63) s.wtot[l >> 6] = inc;
                    }
                    __syncthreads();
                    int before = 0, tot = 0;
                    for (int w = 0; w < NLA / 64; ++w) { const int c = s.wtot[w]; if (w < (l >> 6)) before += c; tot += c; }
                    if (lthr) s.pre[l] += before;
                    __syncthreads();
                    uint4 *rows = P.trace_rows + (size_t)tslot * P.trace_cap;
                    for (int k = l; k < tot; k += BD) {
                        int lo = 0, hi = NLA - 1;            // the lane of row k: the last lane whose first row is <= k
                        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s.pre[mid] <= k) lo = mid; else hi = mid - 1; }
                        const unsigned ob = (unsigned)vslot(k - s.pre[lo], lo, NLP) * 4u;
                        const float4 a = ldg(S, 4u * ob);
                        const uint32_t r0 = ldg(R0, ob);
                        if (tcur + k < P.trace_cap)        // rows past the buffer are dropped, but counted (the cursor)
                            rows[tcur + k] = make_uint4((uint32_t)lo | (__float_as_uint(a.w) & 0xFFFF0000u), r0, __float_as_uint(a.x), __float_as_uint(a.y));
                    }
                    tcur += tot;
                    if (l == 0) {
                        int *cnt = P.trace_cnt + (size_t)tslot * (P.episode + 1);
                        cnt[1 + t] = tot;
                        cnt[0] = tcur;
                    }
                }
            }
            __syncthreads();
            if (l < 4) s.rint[l] = 0;
        }
    }

    // ---- the epilogue reads its arguments here, behind the loop (see "Scalar registers" above)
    const StepArgsPtr ka = step_args();
    const auto &Q = ka->P;
    const int A_ = SPEC > 0 ? P.A : Q.A, LMAX_ = SPEC > 0 ? P.LMAX : Q.LMAX, PMAX_ = SPEC > 0 ? P.PMAX : Q.PMAX, NBR_ = SPEC > 0 ? P.NBR : Q.NBR;   // (SPEC: constants)
    // ---- K4: detectors (envs/env.py:325-407): wave, halting, wait of the front-most vehicle
    {   // window-mean live vehicles: one atomic per wavefront
        int tot = lane ? n : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_down(tot, o, 64);
        if ((l & 63) == 0 && tot) atomicAdd(&Q.live_acc[e], (unsigned long long)tot);
    }
    if (lane) {
        Q.N[(size_t)e * NLP + l] = n;
        // counts were taken while the last simulated second wrote the vehicles; the front-most vehicle is slot 0
        const int hw = (n > 0 && hx >= det && hx > 0.0f) ? (int)(hm & 0xFFFFu) : 0;
        s.wave[l] += d_wave; s.halt[l] += d_halt; s.hwait[l] = hw;       // the flat phase added its vehicles with LDS atomics
    }
    for (int r = l; r < NS; r += BD) { Q.pending[(size_t)e * NS + r] = s.pend[r]; Q.serial[(size_t)e * NS + r] = s.ser[r]; }
    if (arrived) atomicAdd(&Q.arrived[e], (unsigned long long)arrived);
    if (tele) atomicAdd(&Q.teleported[e], (unsigned long long)tele);
    if constexpr (LD) {                 // the interval's sums back (the barrier that ended the last second orders the LDS)
        if (ldon) {
            for (int i = l; i < kLdInts * nds; i += BD) ld_gi[i] = s.ldi[i];
            for (int i = l; i < nds; i += BD) ld_gs[i] = s.ldsp[i];
        }
    }
    if (l == 0) { Q.tsec[e] = t; ka->done[e] = t >= Q.episode ? 1 : 0; }
    TSC_STAMP();
    __syncthreads();
    TSC_STAMP();

    // ---- K5: observations.  The float64 normalisation (envs/env.py:439-442, a division) is done once per lane,
    // not once per observation entry; the entries then only gather.  The outbox arrays are dead by now.
    float *o_wave = s.ox, *o_coop = s.ov, *o_wait = s.osf;        // [NLP] each (kMaxCross * NLA >= NLP)
    int *qacc = (int *)s.om, *wacc = qacc + A_;                   // per-agent queue / wait sums (integers: exact in any order)
    for (int q = l; q < NLP; q += BD) {
        const double wv = norm_clip((double)s.wave[q], Q.norm_wave, Q.clip_wave);
        o_wave[q] = (float)wv;
        o_coop[q] = (float)(wv * Q.coop_gamma);
        o_wait[q] = (float)norm_clip((double)s.hwait[q], Q.norm_wait, Q.clip_wait);
    }
    for (int a = l; a < 2 * A_; a += BD) qacc[a] = 0;
    __syncthreads();
    {
        const int tot = A_ * Q.SMAX;
        const float *fp = (Q.fp_bound ? Q.fp_bound : Q.fp) + (size_t)e * A_ * PMAX_;
        float *ob = ka->obs + (size_t)e * tot;
        constexpr int kOB = 6;                                     // entries per thread and round, loads first
        for (int base = l; base < tot; base += kOB * BD) {
            int ks[kOB];
#pragma unroll
            for (int u = 0; u < kOB; ++u) { const int idx = base + u * BD; ks[u] = Q.obs_ks[idx < tot ? idx : tot - 1]; }
#pragma unroll
            for (int u = 0; u < kOB; ++u) {
                const int idx = base + u * BD;
                if (idx >= tot) continue;
                const int kind = ks[u] >> 16, src = ks[u] & 0xFFFF;
                float o = 0.0f;
                if (kind == 1) o = o_wave[src];
                else if (kind == 2) o = o_coop[src];
                else if (kind == 3) o = o_wait[src];
                else if (kind == 4) o = fp[src];
                ob[idx] = o;
            }
        }
    }
    TSC_STAMP();
    // ---- K6: reward (envs/env.py:356-367) and shaping (:580,:590-631), float64.  Queue and wait of an agent are
    // sums of small integers: accumulated with LDS atomics over all (agent, lane) pairs in parallel.
    for (int p2 = l; p2 < A_ * LMAX_; p2 += BD) {
        const int ln = Q.agent_lanes[p2];
        const int a = p2 / LMAX_;
        if (ln >= 0 && p2 - a * LMAX_ < Q.agent_nlane[a]) {
            int q = s.halt[ln];
            if (Q.queue_cap >= 0 && q > Q.queue_cap) q = Q.queue_cap;
            atomicAdd(&qacc[a], q);
            atomicAdd(&wacc[a], s.hwait[ln]);
        }
    }
    __syncthreads();
    for (int a = l; a < A_; a += BD) {
        const long long queue = qacc[a];
        const double wsum = (double)wacc[a];
        double r;
        if (Q.objective == TSC_OBJ_QUEUE) r = (double)(-queue);
        else if (Q.objective == TSC_OBJ_WAIT) r = -wsum;
        else r = (double)(-queue) - Q.coef_wait * wsum;
        s.r[a] = r;
    }
    __syncthreads();
    if (l == 0) {                                   // (np_sum's scratch: the outbox targets, dead since the last second's gather)
        double g = np_sum(s.r, A_, (double *)s.oto, s.oto + 2 * kNpSumDepth);
        s.r[A_] = g; ka->greward[e] = g; Q.reward_acc[e] += g;
    }
    __syncthreads();
    // (the loop of shape_rewards, kept in place: calling it here changes the scalar register allocation of the whole kernel)
    for (int a = l; a < A_; a += BD) {
        const double g = s.r[A_];
        double out;
        if (!ka->train_mode) {
            out = s.r[a];
        } else if (Q.agent_kind == TSC_AGENT_GREEDY) {
            out = g;
        } else if (Q.agent_kind == TSC_AGENT_GLOBAL) {
            out = Q.realnet_scale ? g / (double)(A_ * 20) : g;
        } else {
            double cur = s.r[a];
            int deg = 0;
            for (int j = 0; j < NBR_; ++j) {
                const int nb = Q.nbr[a * NBR_ + j];
                if (nb < 0) break;
                cur += Q.coop_gamma * s.r[nb];
                ++deg;
            }
            out = Q.realnet_scale ? cur / (double)((1 + deg) * 20) : cur;
        }
        ka->reward[(size_t)e * A_ + a] = out;
    }
    TSC_STAMP();
#ifdef TSC_ENV_PHASE_SUMS
    if (wsum) {
#pragma unroll
        for (int b_ = 0; b_ < 5; ++b_) Q.dbg[64 + 2 * (size_t)Q.E + 5 * (size_t)blockIdx.x + b_] = pacc_[b_];
    }
#endif
    if (stamp && Q.dbg) Q.dbg[63] = nstamp;
    if (Q.dbg && threadIdx.x == 0) {
        unsigned hwid, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        // end time in the low 48 bits, XCC id and HW_ID (cu / se / simd / wave slot) on top
        Q.dbg[64 + 2 * blockIdx.x + 1] = (long long)(wall_clock64() & 0xFFFFFFFFFFFFll) | ((long long)(xcc & 0xF) << 60) | ((long long)(hwid & 0xFFF) << 48);
    }
#undef TSC_STAMP
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Every instantiation of step_kernel, one row each: the only place their template arguments are written.  plan_step picks a row.
using StepFn = void (*)(EnvDev, const int *, float *, double *, double *, uint8_t *, int);
struct StepVariant { int maxt, help, rec, kf, spec; StepFn fn; };
#define TSC_ROW(MAXT, HELP, REC, KF, SPEC) {MAXT, HELP, REC, KF, SPEC, step_kernel<MAXT, HELP, REC, KF, SPEC>}
constexpr StepVariant kStepVariants[] = {
    // compile-time table dimensions (large_grid 1, Monaco 2): workgroup 256 / 512 / 1024, flat phase 1 or 2 wide
    TSC_ROW(256, true, false, 1, 1),  TSC_ROW(256, true, false, 2, 1),  TSC_ROW(256, true, false, 1, 2),  TSC_ROW(256, true, false, 2, 2),
    TSC_ROW(512, true, false, 1, 1),  TSC_ROW(512, true, false, 2, 1),  TSC_ROW(512, true, false, 1, 2),  TSC_ROW(512, true, false, 2, 2),
    TSC_ROW(1024, true, false, 1, 1), TSC_ROW(1024, true, false, 2, 1), TSC_ROW(1024, true, false, 1, 2), TSC_ROW(1024, true, false, 2, 2),
    // runtime dimensions, IDM: the flat phase 1 / 2 / 4 wide up to 256 threads, 4 wide above; the plain walk (TSC_ENV_HELP=0)
    TSC_ROW(256, true, false, 1, 0),  TSC_ROW(256, true, false, 2, 0),  TSC_ROW(256, true, false, 4, 0),  TSC_ROW(1024, true, false, 4, 0),
    TSC_ROW(256, false, false, 4, 0), TSC_ROW(1024, false, false, 4, 0),
    // the recording walk; with the trace; with the lane data
    TSC_ROW(256, false, true, 4, 0),             TSC_ROW(1024, false, true, 4, 0),
    TSC_ROW(256, false, true, 4, kSpecTrace),    TSC_ROW(1024, false, true, 4, kSpecTrace),
    TSC_ROW(256, false, true, 4, kSpecLaneData), TSC_ROW(1024, false, true, 4, kSpecLaneData),
    // Krauss (runtime dimensions): the same families, the flat phase 1 wide except up to 256 threads
    TSC_ROW(256, true, false, 1, kSpecKrauss),  TSC_ROW(256, true, false, 2, kSpecKrauss),  TSC_ROW(256, true, false, 4, kSpecKrauss),
    TSC_ROW(1024, true, false, 1, kSpecKrauss), TSC_ROW(256, false, false, 1, kSpecKrauss), TSC_ROW(1024, false, false, 1, kSpecKrauss),
    TSC_ROW(256, false, true, 1, kSpecKrauss),         TSC_ROW(1024, false, true, 1, kSpecKrauss),
    TSC_ROW(256, false, true, 1, kSpecKraussTrace),    TSC_ROW(1024, false, true, 1, kSpecKraussTrace),
    TSC_ROW(256, false, true, 1, kSpecKraussLaneData), TSC_ROW(1024, false, true, 1, kSpecKraussLaneData),
};
#undef TSC_ROW
struct StepPlan { const StepVariant *v = nullptr; int threads = 0; size_t lds = 0; };
constexpr size_t kLdsMax = 160 * 1024;     // LDS of a CU (gfx950): what one workgroup may ask for

struct tsc_env {
    EnvDev P;
    int device;
    hipStream_t stream;
    tsc::DeviceBufs bufs;           // every device buffer of the handle
    size_t smem;                    // LDS of reset_kernel (the IDM layout for the recording state)
    int threads;                    // IDM workgroup size (pick_workgroup)
    int kf;                         // IDM flat-phase vehicles per thread (measurement knob TSC_ENV_KF)
    int spec;                       // kSpec row the scenario's table dimensions match -> specialised step_kernel (TSC_ENV_SPEC=0: off)
    StepPlan plan;                  // what tsc_env_step launches (plan_step)
    uint32_t *d_seeds;
    std::vector<int> h_mode, h_sroute;      // host copies of the stream tables (tsc_env_set_stream_routes)
    std::vector<int> h_cand;                // [NS][KC] a stream's candidates: its interval-0 routes up to the first pad, then -1
    std::vector<int> ir_next;               // [E][NS] the routes the next reset uploads into P.iroute (tsc_env_set_stream_routes)
    bool ir_dirty = false;
    int *order_buf = nullptr;       // tsc_env_set_block_order
    bool auto_threads;              // the workgroup size follows the number of instances resident on the device (pick_workgroup)
    int kf_default;
    // car following (tsc_env_set_car_following): the model in force (P.sigma its dawdling) and the one the next reset installs
    int cf = TSC_CF_IDM, cf_next = TSC_CF_IDM;
    float sigma_next = 0.0f;
    int n_trace = 0;                // traced instances (tsc_env_trace); their buffers are P.trace_*
    // lane data (tsc_env_lane_data): buffers P.ld_*, live from the reset after arming on; the caller's slot count (P.ld_nslot:
    // the prefix of it the device keeps), intervals per episode
    bool ld_live = false;
    int ld_nslot_all = 0, ld_nint = 0;
    // per-instance demand (tsc_env_set_demand): the scenario's flow table; the [E][n_flow] veh/h columns in force and those the next
    // reset installs (empty: the scenario's own for every instance); the scenario's table and, from the first set_demand on, the
    // instances' tables, the uploaded columns and the flow elements grouped by stream (demand_kernel)
    int n_flow = 0;
    std::vector<int> h_flows, dem_cur, dem_next;
    bool dem_dirty = false;
    const uint8_t *emit_shared = nullptr;
    uint8_t *dem_rows = nullptr;
    int *dem_vph = nullptr, *dem_off = nullptr, *dem_fl = nullptr;
    // max-pressure controller (tsc_env_set_pressure): its tables and hold state, null until armed; LDS of pressure_kernel
    PressDev Q = {};
    size_t smem_press = 0;
    std::vector<int> h_nphase;      // host copy of agent_nphase (tsc_env_set_pressure checks the served lists against it)
    // pressure reward (tsc_env_set_reward_pressure): its tables and accumulator, R.acc null until armed; LDS of pressure_reward_kernel
    PressRewDev R = {};
    size_t smem_prew = 0;
    // actuated / SOTL controller (tsc_env_set_actuated): its tables and state, D.hold null until armed; LDS of actuated_kernel; the
    // initial hold state {0, min_green} of every (instance, agent), which arming and tsc_env_reset copy in
    ActDev D = {};
    size_t smem_act = 0;
    std::vector<int> act_init;
};

// TSC_ENV_THREADS / TSC_ENV_KF (measurement / test knobs) over the library's own choice
static int env_threads(const EnvDev &P, int threads) {
    const char *ev = getenv("TSC_ENV_THREADS");
    const int tv = ev ? atoi(ev) : 0;
    return (tv >= P.NLA && tv <= 1024 && tv % 64 == 0) ? tv : threads;
}
static int env_kf(int kf) {
    const char *ev = getenv("TSC_ENV_KF");
    if (!ev) return kf;
    const int kv = atoi(ev);
    return (kv == 2 || kv == 4) ? kv : 1;
}

// IDM workgroup size / flat-phase width for `n_resident` env instances on the device (this handle's and whatever shares the GPU
// with it): the specialised kernels follow the device's load, everything else keeps what tsc_env_create chose.
static void pick_workgroup(tsc_env *h, int n_resident) {
    if (h->auto_threads) {
        int dev_cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) dev_cus = prop.multiProcessorCount;
        h->threads = 256; h->kf = h->kf_default;
        if (n_resident <= dev_cus) { h->threads = 1024; h->kf = 1; }
        else if (n_resident <= 2 * dev_cus) { h->threads = 512; h->kf = 2; }  // (Monaco, E = 512, saturated: 59.6 us with 2, 67.1 with 1)
    }
    h->threads = env_threads(h->P, h->threads);
    h->kf = env_kf(h->kf);
}

// LDS of the step kernels of one family for the handle's current tables and recording state.  KR: the R0 outbox on top when
// recording is off; LD: the flat phase's arrays make room for the lane data.
static size_t step_lds(const EnvDev &P, bool kr, bool ld) {
    return kr ? (ld ? smem_bytes<true, true>(P) : smem_bytes<true>(P)) : (ld ? smem_bytes<false, true>(P) : smem_bytes(P));
}

// The one place that turns the handle's state into a kernel, a workgroup size and an LDS size (header comment: "Which kernel
// runs").  Called by every entry point that changes one of its inputs (`who`), never per step.
static int plan_step(tsc_env *h, const char *who) {
    const EnvDev &P = h->P;
    const bool kr = h->cf == TSC_CF_KRAUSS, help = P.help != 0, ld = P.rec && h->ld_live;
    // Krauss: runtime table dimensions, so the workgroup of TSC_ENV_SPEC=0 whatever shares the device
    const int threads = kr ? env_threads(P, (help && P.NLA < 256) ? 256 : P.NLA) : h->threads;
    const int kf = kr ? env_kf(1) : h->kf;
    const bool narrow = threads <= 256;
    const int wide = narrow ? 256 : 1024;
    StepVariant k;
    if (P.rec) {
        const int what = ld ? (kr ? kSpecKraussLaneData : kSpecLaneData) : P.trace_slot ? (kr ? kSpecKraussTrace : kSpecTrace) : (kr ? kSpecKrauss : 0);
        k = {wide, false, true, kr ? 1 : 4, what, nullptr};
    }
    else if (kr) k = {wide, help, false, (narrow && help) ? kf : 1, kSpecKrauss, nullptr};
    else if (h->spec && help && kf != 4 && (threads == 256 || threads == 512 || threads == 1024)) k = {threads, true, false, kf, h->spec, nullptr};
    else if (narrow && help && kf != 4) k = {256, true, false, kf, 0, nullptr};
    else k = {wide, help, false, 4, 0, nullptr};      // (any wider workgroup with runtime dimensions: the 4-wide flat phase)
    h->plan = StepPlan();                              // a failure below leaves no plan: tsc_env_step refuses
    const StepVariant *v = nullptr;
    for (const StepVariant &r : kStepVariants)
        if (r.maxt == k.maxt && r.help == k.help && r.rec == k.rec && r.kf == k.kf && r.spec == k.spec) v = &r;
    if (!v) return tsc::fail("tsc_env_step: no instantiation for %d threads, kf %d, spec %d", threads, kf, k.spec);
    const size_t lds = step_lds(P, kr, ld);
    if (lds > kLdsMax) return tsc::fail("%s: LDS need %zu B > 160 KiB", who, lds);
    TSC_HIP(hipFuncSetAttribute((const void *)v->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->plan.v = v; h->plan.threads = threads; h->plan.lds = lds;
    return 0;
}

namespace tsc {
ProfState &prof() { static ProfState p; return p; }
}  // namespace tsc

extern "C" {

const char *tsc_last_error(void) { return tsc::err_buf(); }

int tsc_profile_enable(int32_t on) { tsc::prof().on = on != 0; tsc::prof().stride = on > 1 ? on : 1; return 0; }
int tsc_profile_select(uint64_t mask) { tsc::prof().only = mask ? mask : ~0ull; return 0; }

static int prof_fold() {
    tsc::ProfState &p = tsc::prof();
    for (auto &r : p.recs) {
        TSC_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        TSC_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        p.total_ms[r.id] += ms; p.count[r.id] += 1;
        p.pool.push_back(r.a); p.pool.push_back(r.b);
    }
    p.recs.clear();
    return 0;
}

int tsc_profile_reset(void) {
    if (prof_fold()) return 1;
    tsc::ProfState &p = tsc::prof();
    for (int i = 0; i < tsc::KID_COUNT; ++i) { p.total_ms[i] = 0; p.count[i] = 0; p.seq[i] = 0; }
    return 0;
}

int tsc_profile_read(int32_t kernel_id, double *total_ms, int64_t *count) {
    if (kernel_id < 0 || kernel_id >= tsc::KID_COUNT || !total_ms || !count) return tsc::fail("tsc_profile_read: bad arguments");
    if (prof_fold()) return 1;
    const tsc::ProfState &p = tsc::prof();
    const long long timed = p.count[kernel_id], all = p.seq[kernel_id];
    *total_ms = timed ? p.total_ms[kernel_id] / (double)timed * (double)all : 0.0;     // average x launches
    *count = all;
    return 0;
}

const char *tsc_profile_name(int32_t id) {
    static const char *names[] = {"env_step", "fc_gemm", "zx_gemm", "lstm_fwd", "head_fwd", "sample", "add_transition",
                                  "returns", "head_bwd", "lstm_bwd", "dwo_gemm", "dwh_gemm", "dwx_gemm", "dx1_gemm",
                                  "dw1_gemm", "grad_norm", "rmsprop", "transpose_wx", "fingerprint", "policy_fwd_fused",
                                  "iql_act", "iql_grad", "iql_reduce", "iql_sample", "iql_add", "iql_adam", "iql_target",
                                  "iql_per_sample", "iql_per_update", "iql_per_add", "iql_nstep", "pressure", "pressure_reward", "actuated", "demand",
                                  "gae", "head_bwd_ppo"};
    static_assert(sizeof(names) / sizeof(names[0]) == tsc::KID_COUNT, "one name per kernel id");
    return (id >= 0 && id < tsc::KID_COUNT) ? names[id] : "";
}

int tsc_version(void) { return 124; }      // 1.24: tsc_iql_set_sharing / tsc_iql_get_sharing / tsc_iql_share_grads; 1.23: tsc_model_set_sharing / tsc_model_get_sharing / tsc_model_share_grads; 1.22: tsc_model_dx_split / tsc_dx1w1_f32; 1.21: tsc_model_dw_split / tsc_dwxh_f32; 1.20: tsc_env_set_actuated / tsc_env_actuated_actions / tsc_env_actuated_state; 1.19: tsc_iql_set_return_steps / tsc_iql_get_return_steps / tsc_iql_debug_nstep; 1.18: tsc_model_plan; 1.17: tsc_iql_set_dueling / tsc_iql_get_dueling; 1.16: tsc_iql_set_per / tsc_iql_set_per_beta / tsc_iql_get_priorities / tsc_iql_set_priorities / tsc_iql_debug_per; 1.15: tsc_iql_set_target / tsc_iql_sync_target / tsc_iql_set_target_params / tsc_iql_get_target_params / tsc_iql_debug_targets; 1.14: tsc_env_set_reward_pressure; 1.13: tsc_env_step_plan; 1.12: tsc_env_set_pressure / tsc_env_pressure_actions / tsc_env_fixed_time_actions; 1.11: tsc_model_compute_grads_ppo / tsc_model_apply_grads_ex / tsc_model_ppo_stats; 1.10: tsc_env_set_demand / tsc_env_demand; 1.09: tsc_env_lane_data / tsc_env_read_lane_data; 1.08: tsc_env_trace / tsc_env_read_trace; 1.07: tsc_env_set_car_following / tsc_env_car_following; 1.06: tsc_model_path; 1.05: round 5 (tsc_env_set_greedy / tsc_env_greedy_actions); 1.04: tsc_env_counters, negative arrival = truncated trip

int tsc_env_create(const tsc_scenario *sc, int32_t n_env, int32_t device, tsc_env **out) {
    if (!sc || !out || n_env <= 0) return tsc::fail("tsc_env_create: bad arguments");
    // (every refusal below has its twin in Scenario.check_limits, scenario.py; tests/test_networks_gpu.py asks for each by its text)
    if (sc->n_lane < 1 || sc->n_route < 1 || sc->n_agent < 1)         // (the table prefetch of step_kernel reads entry n_mv - 1)
        return tsc::fail("tsc_env_create: %d lanes, %d routes, %d agents: a scenario needs at least one of each", sc->n_lane, sc->n_route, sc->n_agent);
    if (sc->n_lane > 1024) return tsc::fail("tsc_env_create: n_lane %d > 1024 unsupported (one thread per live lane): split the network", sc->n_lane);
    if (sc->n_route > 254) return tsc::fail("tsc_env_create: n_route %d > 254 unsupported (route ids are bytes on the device): let disjoint parts of the network share route indices", sc->n_route);
    TSC_HIP(hipSetDevice(device));
    tsc_env *h = new tsc_env();
    tsc::CreateGuard<tsc_env, tsc_env_destroy> guard(h);        // an error return below frees the handle and its buffers
    h->device = device;
    h->stream = nullptr;
    EnvDev &P = h->P;
    P.NL = sc->n_lane; P.NLP = (sc->n_lane + 63) / 64 * 64; P.NR = sc->n_route; P.A = sc->n_agent;
    P.KMAX = sc->k_max; P.PMAX = sc->p_max; P.LMAX = sc->l_max; P.SMAX = sc->s_max;
    P.NBR = sc->nbr_max; P.E = n_env;
    P.ctrl = sc->control_interval_sec; P.yellow = sc->yellow_interval_sec; P.episode = sc->episode_length_sec;
    P.teleport = sc->teleport_sec; P.queue_cap = sc->queue_cap; P.objective = sc->objective;
    P.agent_kind = sc->agent_kind; P.realnet_scale = sc->realnet_scale;
    P.coop_gamma = sc->coop_gamma; P.norm_wave = sc->norm_wave; P.norm_wait = sc->norm_wait;
    P.clip_wave = sc->clip_wave; P.clip_wait = sc->clip_wait; P.coef_wait = sc->coef_wait;

    const int NL = P.NL, NR = P.NR, A = P.A;
    bool any_zip = false;                   // some lane has more than one feeder without a right-of-way table (zipper merge)
    // insertion streams: none declared -> every route is its own stream
    const bool streams = sc->n_stream > 0;
    const int NS = streams ? sc->n_stream : NR, KC = streams ? sc->k_choice : 1;
    P.NS = NS; P.KC = KC;
    if (NS > 254) return tsc::fail("tsc_env_create: n_stream %d > 254 unsupported (stream lists are bytes on the device): merge the flow elements of streams that share an entry lane and a route", NS);
    if (streams && (!sc->stream_entry || !sc->stream_mode || !sc->stream_choice || KC < 1 || sc->n_interval < 1 || sc->choice_interval_sec < 1))
        return tsc::fail("tsc_env_create: incomplete stream tables");
    const int NI = streams ? sc->n_interval : 1;
    P.NI = NI; P.ilen = streams ? sc->choice_interval_sec : 1 << 30;
    auto stream_entry = [&](int s_) { return streams ? sc->stream_entry[s_] : sc->route_entry[s_]; };
    // Lanes that can ever hold a vehicle: the chains route entry lane -> mv_next[lane][route] -> ...  (the movement
    // table also has rows for the sibling lanes of every edge a route passes, which no vehicle of that route is
    // ever put on).  After load sorting they are a prefix; only they get a thread and LDS rows.
    std::vector<char> reach((size_t)NL, 0);
    {
        int nu = 0;
        for (int s_ = 0; s_ < NS; ++s_)
            for (int c = 0; c < KC * NI; ++c) {
                const int r = streams ? sc->stream_choice[((size_t)s_ * KC * NI + c) * 2] : s_;
                if (r < 0) continue;
                if (r >= NR) return tsc::fail("tsc_env_create: stream %d names route %d of %d", s_, r, NR);
                int l = stream_entry(s_);
                for (int hops = 0; l >= 0 && l < NL && hops <= 2 * NL; ++hops) {
                    reach[l] = 1;
                    if (l + 1 > nu) nu = l + 1;
                    int nx = sc->mv_next[(size_t)l * NR + r];
                    if (nx < -1 && sc->lane_sib && sc->lane_sib[l] >= 0 && sc->lane_sib[l] < NL &&
                        sc->mv_next[(size_t)sc->lane_sib[l] * NR + r] >= -1) nx = sc->lane_sib[l];     // rule 10: the vehicle moves over
                    l = nx;
                }
            }
        P.NU = nu < 1 ? 1 : nu;
        P.NLA = (P.NU + 63) / 64 * 64;
    }
    TSC_HIP(h->bufs.upload(&P.lane_len, sc->lane_len, NL)); TSC_HIP(h->bufs.upload(&P.lane_vmax, sc->lane_vmax, NL));
    TSC_HIP(h->bufs.upload(&P.lane_det, sc->lane_det_start, NL));
    TSC_HIP(h->bufs.upload(&P.lane_node, sc->lane_node, NL));
    if (sc->lane_sib) {
        for (int l = 0; l < NL; ++l)
            if (sc->lane_sib[l] >= NL || sc->lane_sib[l] == l) return tsc::fail("tsc_env_create: lane %d names sibling lane %d of %d", l, sc->lane_sib[l], NL);
        // the domain of MICROSIM_SPEC.md rule 10: a changer keeps its position and is gathered before the junction's arrivals
        for (int l = 0; l < NL; ++l) {
            const int sb = sc->lane_sib[l];
            if (sb < 0) continue;
            if (sc->lane_sib[sb] != l)
                return tsc::fail("tsc_env_create: lane %d names sibling lane %d, whose sibling is lane %d: lane_sib must be symmetric, name each lane of a two-lane street on the other", l, sb, sc->lane_sib[sb]);
            if (sc->lane_len[l] != sc->lane_len[sb])
                return tsc::fail("tsc_env_create: lanes %d and %d are siblings of different length (%g m and %g m): a lane changer keeps its position, give both lanes of a street one length", l, sb, (double)sc->lane_len[l], (double)sc->lane_len[sb]);
            if (sc->lane_up[(size_t)l * kMaxUp] != sb)
                return tsc::fail("tsc_env_create: lane %d does not list its sibling lane %d first in lane_up: lane changers are gathered before the junction's arrivals, put the sibling in slot 0", l, sb);
        }
        TSC_HIP(h->bufs.upload(&P.lane_sib, sc->lane_sib, NL));
    }
    {
        std::vector<int> up(sc->lane_up, sc->lane_up + (size_t)NL * kMaxUp);
        for (int &u : up) if (u >= 0 && (u >= NL || !reach[u])) u = -1;        // a feeder that is never occupied never sends
        TSC_HIP(h->bufs.upload(&P.lane_up, up.data(), up.size()));
    }
    if (NL > 0xFFD) return tsc::fail("tsc_env_create: n_lane %d > 4093 unsupported", NL);
    std::vector<int> mv((size_t)NL * NR);
    for (int i = 0; i < NL * NR; ++i) {
        const int nx = sc->mv_next[i], lk = sc->mv_link[i], pr = sc->mv_prio[i];
        const int yl = (sc->mv_yield[i] >= 0 && reach[sc->mv_yield[i]]) ? sc->mv_yield[i] : -1;   // an empty lane has no right of way to give
        if (lk > 62) return tsc::fail("tsc_env_create: signal link index %d > 62 unsupported (six bits of the movement word, 63 = none): split the junction into two agents", lk);
        const unsigned a = nx == -1 ? 0xFFFu : nx < -1 ? 0xFFEu : (unsigned)nx;
        const unsigned b = lk < 0 ? 63u : (unsigned)lk;
        const unsigned c = yl < 0 ? 0xFFFu : (unsigned)yl;
        mv[i] = (int)(a | (b << 12) | (c << 18) | ((pr ? 1u : 0u) << 30));
        if (mv_tl(mv[i]) != (nx < -1 ? -2 : nx) || mv_k(mv[i]) != (lk < 0 ? -1 : lk) || mv_yield(mv[i]) != yl)
            return tsc::fail("tsc_env_create: movement table overflow");
    }
    TSC_HIP(h->bufs.upload(&P.mv, mv.data(), NL * NR));
    {
        std::vector<uint8_t> zp(((size_t)NL * NR + 3) / 4 * 4, 0);
        for (int i = 0; i < NL * NR; ++i) {
            const int z = sc->mv_zip[i], rank = z & 0xFF, cnt = z >> 8;
            if (z < 0 || rank > 15 || cnt > 15)
                return tsc::fail("tsc_env_create: zipper slot overflow: rank %d of %d at lane %d, route %d (four bits each on the device)", rank, cnt, i / NR, i % NR);
            zp[i] = (uint8_t)(rank | (cnt << 4));
        }
        TSC_HIP(h->bufs.upload(&P.zip, zp.data(), zp.size()));
        for (uint8_t v : zp) if (v >> 4 > 1) any_zip = true;
        // the merge arbitration packs a lane's feeders into bytes (Smem::up4, 0xFF = none): a feeder index >= 255 would be
        // left out of the winner search and wait for the teleport
        if (any_zip && NL > 255)
            return tsc::fail("tsc_env_create: zipper merges need lane indices < 255 (feeders are bytes on the device), the scenario has %d lanes", NL);
    }
    P.sroute = nullptr; P.smode = nullptr; P.schoice = nullptr; P.sorigin = nullptr; P.iroute = nullptr;
    if (streams) {
        std::vector<int> sr(NS);
        bool any_origin = false, identity = NS == NR;
        for (int s_ = 0; s_ < NS; ++s_) {
            const int md = sc->stream_mode[s_];
            if (md < 0 || md > 2) return tsc::fail("tsc_env_create: stream %d has mode %d", s_, md);
            sr[s_] = sc->stream_choice[(size_t)s_ * NI * KC * 2];
            // a mode-1 stream draws from the table of the second it inserts in: a table that begins with a pad would hand out route -1
            for (int iv = 0; iv < (md == 1 ? NI : 1); ++iv)
                if (sc->stream_choice[((size_t)s_ * NI + iv) * KC * 2] < 0)
                    return tsc::fail("tsc_env_create: stream %d has no route in interval %d", s_, iv);
            if (md != 0 || sr[s_] != s_) identity = false;
            if (sc->stream_origin && sc->stream_origin[s_] != 0.0f) any_origin = true;
            if (sc->stream_limit && sc->stream_limit[s_] < sc->lane_len[stream_entry(s_)]) any_origin = true;
        }
        h->h_mode.assign(sc->stream_mode, sc->stream_mode + NS); h->h_sroute = sr;
        h->h_cand.assign((size_t)NS * KC, -1);
        for (int s_ = 0; s_ < NS; ++s_)
            for (int c = 0; c < KC && sc->stream_choice[((size_t)s_ * NI * KC + c) * 2] >= 0; ++c)
                h->h_cand[(size_t)s_ * KC + c] = sc->stream_choice[((size_t)s_ * NI * KC + c) * 2];
        if (!identity) {                              // fixed one-to-one streams keep the round-2 fast path (sroute == null)
            TSC_HIP(h->bufs.upload(&P.sroute, sr.data(), NS));
            TSC_HIP(h->bufs.upload(&P.smode, sc->stream_mode, NS));
            TSC_HIP(h->bufs.upload(&P.schoice, sc->stream_choice, (size_t)NS * NI * KC * 2));
            TSC_HIP(h->bufs.alloc(&P.iroute, (size_t)n_env * NS, true));
            std::vector<int> ir((size_t)n_env * NS);
            for (size_t i = 0; i < ir.size(); ++i) ir[i] = sr[i % NS];
            TSC_HIP(hipMemcpy(P.iroute, ir.data(), sizeof(int) * ir.size(), hipMemcpyHostToDevice));
        }
        if (any_origin) {
            std::vector<float> so((size_t)NS * 2);
            for (int s_ = 0; s_ < NS; ++s_) {
                so[2 * s_] = sc->stream_origin ? sc->stream_origin[s_] : 0.0f;
                so[2 * s_ + 1] = sc->stream_limit ? sc->stream_limit[s_] : INFINITY;
            }
            TSC_HIP(h->bufs.upload(&P.sorigin, so.data(), so.size()));
        }
    }
    {   // per-lane entry routes (<= 2) and per-route emission table (MICROSIM_SPEC.md, rule 6)
        std::vector<int> lr((size_t)NL * kMaxEntry, -1);
        for (int r = 0; r < NS; ++r) {
            const int l = stream_entry(r);
            if (l < 0 || l >= NL) return tsc::fail("tsc_env_create: stream %d has no entry lane", r);
            int q = 0;
            while (q < kMaxEntry && lr[l * kMaxEntry + q] >= 0) ++q;
            if (q == kMaxEntry) return tsc::fail("tsc_env_create: more than %d streams enter lane %d: merge the flow elements of streams that share a route", kMaxEntry, l);
            lr[l * kMaxEntry + q] = r;
        }
        std::vector<uint32_t> lrp((size_t)NL * 2, 0xFFFFFFFFu);         // one byte per route (n_route <= 255 checked above)
        for (int l = 0; l < NL; ++l)
            for (int q = 0; q < kMaxEntry; ++q)
                if (lr[l * kMaxEntry + q] >= 0)
                    lrp[l * 2 + q / 4] = (lrp[l * 2 + q / 4] & ~(0xFFu << (8 * (q % 4)))) | ((uint32_t)lr[l * kMaxEntry + q] << (8 * (q % 4)));
        TSC_HIP(h->bufs.upload(&P.lane_routes, lrp.data(), lrp.size()));
        P.emit_len = (sc->episode_length_sec + 64 + 3) / 4 * 4;       // (whole words: demand_kernel stores four seconds at once)
        std::vector<uint8_t> em((size_t)NS * P.emit_len, 0);
        for (int f = 0; f < sc->n_flow; ++f) {
            const long long b = sc->flows[f * 4], en = sc->flows[f * 4 + 1], vph = sc->flows[f * 4 + 2];
            const int r = sc->flows[f * 4 + 3];
            if (r < 0 || r >= NS) return tsc::fail("tsc_env_create: flow %d names stream %d of %d", f, r, NS);
            if (b < 0 || vph < 0)                         // (the table starts at second 0: t = b would index in front of it)
                return tsc::fail("tsc_env_create: flow %d begins at second %lld with %lld veh/h: neither may be negative: cut the element at 0", f, b, vph);
            for (long long t = b; t < en && t < P.emit_len; ++t) {
                const long long tau = t - b;
                const long long c = (((tau + 1) * vph + 3599) / 3600) - ((tau * vph + 3599) / 3600);
                const long long v = em[(size_t)r * P.emit_len + t] + c;
                if (v > 255) return tsc::fail("tsc_env_create: flow %d makes stream %d emit more than 255 vehicles per second (a byte per second and stream): spread the vehicles over more seconds", f, r);
                em[(size_t)r * P.emit_len + t] = (uint8_t)v;
            }
        }
        TSC_HIP(h->bufs.upload(&P.emit_tab, em.data(), em.size()));
        P.emit_inst = 0;
        h->emit_shared = P.emit_tab;
        h->n_flow = sc->n_flow;
        h->h_flows.assign(sc->flows, sc->flows + (size_t)sc->n_flow * 4);
    }
    if (sc->control_interval_sec > 8) return tsc::fail("tsc_env_create: control interval %d > 8 s unsupported (eight emission and record rows per launch)", sc->control_interval_sec);
    TSC_HIP(h->bufs.upload(&P.agent_lanes, sc->agent_lanes, A * P.LMAX));
    TSC_HIP(h->bufs.upload(&P.agent_nlane, sc->agent_nlane, A)); TSC_HIP(h->bufs.upload(&P.agent_nlink, sc->agent_nlink, A));
    TSC_HIP(h->bufs.upload(&P.agent_nphase, sc->agent_nphase, A));
    h->h_nphase.assign(sc->agent_nphase, sc->agent_nphase + A);
    TSC_HIP(h->bufs.upload(&P.green_tab, sc->green_tab, (size_t)A * P.PMAX * P.KMAX));
    TSC_HIP(h->bufs.upload(&P.yellow_tab, sc->yellow_tab, (size_t)A * P.PMAX * P.PMAX * P.KMAX));
    TSC_HIP(h->bufs.upload(&P.nbr, sc->nbr, A * P.NBR));
    TSC_HIP(h->bufs.upload(&P.obs_kind, sc->obs_kind, A * P.SMAX)); TSC_HIP(h->bufs.upload(&P.obs_src, sc->obs_src, A * P.SMAX));
    {
        std::vector<int> ks((size_t)A * P.SMAX);
        for (size_t i = 0; i < ks.size(); ++i) {
            if (sc->obs_src[i] < 0 || sc->obs_src[i] > 0xFFFF) { ks[i] = 0; continue; }
            ks[i] = (sc->obs_kind[i] << 16) | sc->obs_src[i];
        }
        TSC_HIP(h->bufs.upload(&P.obs_ks, ks.data(), ks.size()));
    }

    const size_t slots = (size_t)n_env * kCap * P.NLP;
    TSC_HIP(h->bufs.alloc(&P.S, slots, true));
    TSC_HIP(h->bufs.alloc(&P.N, (size_t)n_env * P.NLP, true));
    TSC_HIP(h->bufs.alloc(&P.pending, (size_t)n_env * NS, true)); TSC_HIP(h->bufs.alloc(&P.serial, (size_t)n_env * NS, true));
    TSC_HIP(h->bufs.alloc(&P.tsec, n_env, true)); TSC_HIP(h->bufs.alloc(&P.seed, n_env, true));
    TSC_HIP(h->bufs.alloc(&P.prev_action, (size_t)n_env * A, true));
    TSC_HIP(h->bufs.alloc(&P.fp, (size_t)n_env * A * P.PMAX, true));
    TSC_HIP(h->bufs.alloc(&P.arrived, n_env, true));
    TSC_HIP(h->bufs.alloc(&P.teleported, n_env, true));
    TSC_HIP(h->bufs.alloc(&P.reward_acc, n_env, true));
    TSC_HIP(h->bufs.alloc(&P.n_trips, n_env, true)); TSC_HIP(h->bufs.alloc(&P.live_acc, n_env, true));
    {
        std::vector<float> org((size_t)NL, 0.0f);
        if (sc->lane_origin) org.assign(sc->lane_origin, sc->lane_origin + NL);
        TSC_HIP(h->bufs.upload(&P.lane_origin, org.data(), NL));
    }
    P.rec = 0; P.trip_cap = 0; P.R0 = P.R1 = nullptr; P.rec_int = nullptr; P.rec_speed = nullptr; P.rec_queue = nullptr;
    P.trips = nullptr;
    P.trace_cap = 0; P.trace_slot = nullptr; P.trace_cnt = nullptr; P.trace_rows = nullptr;
    P.ld_period = 0; P.ld_nslot = 0; P.ld_slot0 = nullptr; P.ld_bound = nullptr; P.ld_sumo = nullptr; P.ld_int = nullptr; P.ld_speed = nullptr;
    P.fp_bound = nullptr;
    P.dbg = nullptr;
    P.order = nullptr;
    TSC_HIP(h->bufs.alloc(&h->d_seeds, n_env, false));
    {   // phase A1 (helper threads) unless switched off for A/B measurements
        const char *ev = getenv("TSC_ENV_HELP");
        P.help = (ev && ev[0] == '0') ? 0 : 1;
    }
    if (kMaxCross * P.NLA < P.NLP || kMaxCross * P.NLA < 2 * P.A)
        return tsc::fail("tsc_env_create: too few live lanes (%d of %d, %d agents) for the observation scratch: leave out lanes and junctions that no route reaches", P.NU, P.NL, P.A);
    h->smem = smem_bytes(P);
    h->threads = (P.help && P.NLA < 256) ? 256 : P.NLA;
    // the reference's large_grid / Monaco get the instantiation with compile-time table dimensions (TSC_ENV_SPEC=0: off)
    h->spec = 0;
    for (int k = 1; k < 3; ++k) {
        const SpecDims &D = kSpec[k];
        // (NU: the scenario's live lanes are a prefix of the instantiation's; the lanes in between stay empty)
        if (P.NS == P.NR && P.NLP == D.NLP && P.NLA == D.NLA && P.NU <= D.NU && D.NU <= P.NL && P.NR == D.NR && P.A == D.A && P.KMAX == D.KMAX && P.PMAX == D.PMAX &&
            P.LMAX == D.LMAX && P.NBR == D.NBR && P.ctrl == D.ctrl && P.yellow == D.yellow && P.teleport == D.teleport &&
            (k != 1 || (!any_zip && !P.sorigin)) && !P.sroute) { h->spec = k; P.NU = D.NU; h->smem = smem_bytes(P); }
    }
    if (const char *ev = getenv("TSC_ENV_SPEC")) if (!atoi(ev)) h->spec = 0;
    // vehicles per thread and super-round of the flat phase (TSC_ENV_KF = 1 / 2 / 4 for A/B runs).  With runtime dimensions
    // 1 is best (296 M env-steps/s; 2: 294, 4: 284 -- fewer barriers do not pay for the registers); the specialised kernel
    // has the registers for 2 (env step 11.5 -> 10.7 ms per rollout; 4 spills: 11.4; round 5, rule-10 traffic, episode average:
    // 3 -- 128 VGPRs, 8 spilled dwords, bit-exact -- 94.9 / 95.3 us per control step against 92.7 / 92.8 with 2; again without the
    // scalar spills -- 99 VGPRs, no scratch, bit-exact -- 81.0 - 81.3 us against 75.6 - 76.1 with 2, five runs each, V = 859: the
    // third vehicle per thread lengthens every wavefront's chain by more than the rare second super-round costs.  Not built.)
    h->kf = env_kf(h->spec == 1 ? 2 : 1);                    // (Monaco, spec 2: 330 M env-steps/s with 1, 323 M with 2)
    if (h->spec && h->kf == 4) h->spec = 0;                  // (no specialised instantiation of the 4-wide variant)
    // Workgroup size of the specialised kernels: a CU holds 16 wavefronts of this kernel (128 VGPRs), i.e. four workgroups of 256
    // threads.  With fewer instances than that the flat phase -- a latency chain per wavefront -- is spread over more wavefronts of
    // the same instance instead of leaving the slots idle (sim only, saturated large_grid: E = 256: 63.0 -> 52.5 us per control
    // step with 1024 threads, E = 512: 70.9 -> 64.8 us with 512; Monaco 69.6 -> 59.9 / 77.9 -> 71.5; E = 1024 wants 256).
    // TSC_ENV_THREADS overrides (parity tests run every size).
    // What counts is how many instances share the DEVICE, not this handle's own: tsc_env_set_resident_instances (half-batches on
    // separate streams, ranks sharing a GPU).
    h->auto_threads = h->spec && P.help && h->threads == 256;
    h->kf_default = h->kf;
    pick_workgroup(h, n_env);
    if (plan_step(h, "tsc_env_create")) return 1;            // (checks h->smem, the LDS of a fresh handle's kernels, against kLdsMax)
    TSC_HIP(hipFuncSetAttribute((const void *)reset_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem));
    *out = guard.release();
    return 0;
}

int tsc_env_record(tsc_env *h, int32_t enable, int32_t trip_cap) {
    if (!h || trip_cap < 0) return tsc::fail("tsc_env_record: bad arguments");
    EnvDev &P = h->P;
    EnvDev want = P;                             // checked before anything changes: a refusal leaves the handle, its plan included, as it was
    want.rec = enable ? 1 : 0;
    const size_t need = smem_bytes(want);
    if (need > kLdsMax) return tsc::fail("tsc_env_record: LDS need %zu B > 160 KiB", need);
    TSC_HIP(hipStreamSynchronize(h->stream));
    if (enable && !P.R1) {
        const size_t slots = (size_t)P.E * kCap * P.NLP;
        if (!P.R0) TSC_HIP(h->bufs.alloc(&P.R0, slots, true));          // (a Krauss handle has it already: one word per slot for both)
        TSC_HIP(h->bufs.alloc(&P.R1, slots, true));
        TSC_HIP(h->bufs.alloc(&P.rec_int, (size_t)P.E * 8 * 4, true)); TSC_HIP(h->bufs.alloc(&P.rec_speed, (size_t)P.E * 8, true));
        TSC_HIP(h->bufs.alloc(&P.rec_queue, (size_t)P.E * 8 * P.A * P.LMAX, true));
        P.trip_cap = trip_cap > 0 ? trip_cap : 8192;
        TSC_HIP(h->bufs.alloc(&P.trips, (size_t)P.E * P.trip_cap * 6, true));
    }
    P.rec = enable ? 1 : 0;
    h->smem = need;
    TSC_HIP(hipFuncSetAttribute((const void *)reset_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem));
    // (the Krauss and lane-data layouts need no check of their own here: with recording on a Krauss kernel takes what the IDM one
    // takes, without it what tsc_env_set_car_following checked; lane data was checked, recording on, when it was armed)
    return plan_step(h, "tsc_env_record");
}

// Build, then swap (tsc_env_lane_data, tsc_env_trace): the caller has built new tables into D, a copy of the handle's EnvDev.  Waits
// for the stream (a running step may still write the old buffers), installs D and plans the step for it.  On return D holds what
// the handle does not use, for the caller to release: the old tables, or on failure the new ones -- the handle, its plan and
// ld_live are then as they were.
static int swap_and_plan(tsc_env *h, EnvDev &D, bool ld_live, const char *who) {
    TSC_HIP(hipStreamSynchronize(h->stream));
    const StepPlan plan0 = h->plan;
    const bool live0 = h->ld_live;
    std::swap(h->P, D); h->ld_live = ld_live;
    if (!plan_step(h, who)) return 0;
    std::swap(h->P, D); h->ld_live = live0; h->plan = plan0;
    return 1;
}

int tsc_env_lane_data(tsc_env *h, int32_t period_sec, int32_t n_slot, const int32_t *lane_slot0_host, const float *slot_start_host,
                      const int32_t *slot_sumo_host) {
    if (!h) return tsc::fail("tsc_env_lane_data: bad arguments");
    EnvDev &P = h->P;
    const int NL = P.NL;
    if (period_sec > 0) {
        if (!P.rec) return tsc::fail("tsc_env_lane_data: recording is off (call tsc_env_record(h, 1, ...) first: the lane data rides on the recording walk)");
        if (period_sec % P.ctrl) return tsc::fail("tsc_env_lane_data: period %d s is not a multiple of the control interval (%d s)", period_sec, P.ctrl);
        if (!lane_slot0_host || !slot_start_host || !slot_sumo_host || n_slot < NL) return tsc::fail("tsc_env_lane_data: bad slot tables");
        if (lane_slot0_host[0] != 0 || lane_slot0_host[NL] != n_slot) return tsc::fail("tsc_env_lane_data: lane_slot0 must run from 0 to n_slot = %d", n_slot);
        for (int l = 0; l < NL; ++l) {
            const int k0 = lane_slot0_host[l], k1 = lane_slot0_host[l + 1];
            if (k1 <= k0) return tsc::fail("tsc_env_lane_data: lane %d has no slot", l);
            if (k1 - k0 > kLdMaxPieces) return tsc::fail("tsc_env_lane_data: lane %d has %d pieces, at most %d", l, k1 - k0, kLdMaxPieces);
            for (int k = k0 + 1; k < k1; ++k)
                if (!(slot_start_host[k] >= slot_start_host[k - 1])) return tsc::fail("tsc_env_lane_data: the pieces of lane %d are out of order", l);
        }
        for (int k = 0; k < n_slot; ++k)
            if (slot_sumo_host[k] < 0) return tsc::fail("tsc_env_lane_data: slot %d has SUMO lane %d", k, slot_sumo_host[k]);
        if (lane_slot0_host[P.NU] >= 0x8000) return tsc::fail("tsc_env_lane_data: %d slots on the live lanes, at most 32767", lane_slot0_host[P.NU]);
    }
    (void)hipSetDevice(h->device);
    EnvDev D = P;                                               // with the new lane-data tables (none: detached)
    D.ld_slot0 = nullptr; D.ld_bound = nullptr; D.ld_sumo = nullptr; D.ld_int = nullptr; D.ld_speed = nullptr;
    D.ld_period = 0; D.ld_nslot = 0;
    const int nds = period_sec > 0 ? lane_slot0_host[P.NU] : 0;
    const int nint = period_sec > 0 ? (P.episode + period_sec - 1) / period_sec : 0;
    const auto drop = [h](const EnvDev &d) {
        h->bufs.release(d.ld_slot0); h->bufs.release(d.ld_bound); h->bufs.release(d.ld_sumo); h->bufs.release(d.ld_int); h->bufs.release(d.ld_speed);
    };
    const auto build = [&]() {
        if (period_sec <= 0) return 0;
        D.ld_period = period_sec; D.ld_nslot = nds;
        // what the reset will install, checked here (IDM and Krauss: either may be in force by then)
        const size_t need = std::max(step_lds(D, false, true), step_lds(D, true, true));
        if (need > kLdsMax) return tsc::fail("tsc_env_lane_data: LDS need %zu B > 160 KiB (%d slots)", need, nds);
        TSC_HIP(h->bufs.upload(&D.ld_slot0, lane_slot0_host, NL + 1));
        // a lane's piece starts 2..5 as one 16-byte LDS word per lane (the lookup: four compares)
        std::vector<float4> b((size_t)P.NU);
        for (int l = 0; l < P.NU; ++l) {
            float v[4];
            for (int j = 0; j < 4; ++j) {
                const int k = lane_slot0_host[l] + 1 + j;
                v[j] = k < lane_slot0_host[l + 1] ? slot_start_host[k] : INFINITY;
            }
            b[l] = make_float4(v[0], v[1], v[2], v[3]);
        }
        TSC_HIP(h->bufs.upload(&D.ld_bound, b.data(), P.NU));
        TSC_HIP(h->bufs.upload(&D.ld_sumo, slot_sumo_host, nds));
        TSC_HIP(h->bufs.alloc(&D.ld_int, (size_t)P.E * nint * kLdInts * nds, true));
        TSC_HIP(h->bufs.alloc(&D.ld_speed, (size_t)P.E * nint * nds, true));
        return 0;
    };
    // (ld_live false: until the next reset the recording kernels without lane data run)
    const int rc = build() || swap_and_plan(h, D, false, "tsc_env_lane_data");
    drop(D);
    if (rc) return 1;
    h->ld_nslot_all = period_sec > 0 ? n_slot : 0; h->ld_nint = nint;
    return 0;                                                   // (ld_live: from the next reset on)
}

int tsc_env_read_lane_data(tsc_env *h, int32_t *ints_host, double *speed_host) {
    if (!h || !ints_host || !speed_host) return tsc::fail("tsc_env_read_lane_data: bad arguments");
    const EnvDev &P = h->P;
    if (!P.ld_int) return tsc::fail("tsc_env_read_lane_data: no lane data armed (tsc_env_lane_data)");
    TSC_HIP(hipStreamSynchronize(h->stream));
    const int nds = P.ld_nslot, ns = h->ld_nslot_all;
    const size_t rows = (size_t)P.E * h->ld_nint;
    std::vector<int> gi(rows * kLdInts * nds);
    std::vector<double> gs(rows * nds);
    TSC_HIP(hipMemcpy(gi.data(), P.ld_int, sizeof(int) * gi.size(), hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(gs.data(), P.ld_speed, sizeof(double) * gs.size(), hipMemcpyDeviceToHost));
    memset(ints_host, 0, sizeof(int32_t) * rows * kLdInts * ns);       // slots of lanes >= NU: never a vehicle
    memset(speed_host, 0, sizeof(double) * rows * ns);
    for (size_t r = 0; r < rows; ++r) {
        for (int f = 0; f < kLdInts; ++f)
            memcpy(ints_host + (r * kLdInts + f) * ns, gi.data() + (r * kLdInts + f) * nds, sizeof(int) * nds);
        memcpy(speed_host + r * ns, gs.data() + r * nds, sizeof(double) * nds);
    }
    return 0;
}

int tsc_env_trace(tsc_env *h, int32_t n_trace, const int32_t *instances_host, int32_t row_cap) {
    if (!h || n_trace < 0) return tsc::fail("tsc_env_trace: bad arguments");
    EnvDev &P = h->P;
    if (n_trace > 0) {
        if (!P.rec) return tsc::fail("tsc_env_trace: recording is off (call tsc_env_record(h, 1, ...) first: the trace rides on the recording walk)");
        if (!instances_host) return tsc::fail("tsc_env_trace: no instance list");
        if (n_trace > P.E) return tsc::fail("tsc_env_trace: %d instances traced, the handle has %d", n_trace, P.E);
        if (row_cap < 1) return tsc::fail("tsc_env_trace: row_cap %d < 1", row_cap);
    }
    std::vector<int> slot((size_t)P.E, -1);
    for (int k = 0; k < n_trace; ++k) {
        const int e = instances_host[k];
        if (e < 0 || e >= P.E) return tsc::fail("tsc_env_trace: instance %d of %d", e, P.E);
        if (slot[e] >= 0) return tsc::fail("tsc_env_trace: instance %d listed twice", e);
        slot[e] = k;
    }
    (void)hipSetDevice(h->device);
    EnvDev D = P;                                               // with the new trace buffers (none: detached)
    D.trace_slot = nullptr; D.trace_cnt = nullptr; D.trace_rows = nullptr; D.trace_cap = 0;
    const auto drop = [h](const EnvDev &d) { h->bufs.release(d.trace_slot); h->bufs.release(d.trace_cnt); h->bufs.release(d.trace_rows); };
    const auto build = [&]() {
        if (n_trace == 0) return 0;
        TSC_HIP(h->bufs.upload(&D.trace_slot, slot.data(), P.E));
        TSC_HIP(h->bufs.alloc(&D.trace_cnt, (size_t)n_trace * (P.episode + 1), true));
        TSC_HIP(h->bufs.alloc(&D.trace_rows, (size_t)n_trace * row_cap, true));
        D.trace_cap = row_cap;
        return 0;
    };
    // the tracing kernels from the next step on (detached: the untraced recording kernels again)
    const int rc = build() || swap_and_plan(h, D, h->ld_live, "tsc_env_trace");
    drop(D);
    if (rc) return 1;
    h->n_trace = n_trace;
    return 0;
}

int tsc_env_read_trace(tsc_env *h, int32_t k, int32_t *counts_host, uint32_t *rows_host, int32_t max_rows, int32_t *n_rows) {
    if (!h || !n_rows || !counts_host || (max_rows > 0 && !rows_host)) return tsc::fail("tsc_env_read_trace: bad arguments");
    const EnvDev &P = h->P;
    if (k < 0 || k >= h->n_trace) return tsc::fail("tsc_env_read_trace: trace %d of %d", k, h->n_trace);
    TSC_HIP(hipStreamSynchronize(h->stream));
    std::vector<int> cnt((size_t)P.episode + 1);
    TSC_HIP(hipMemcpy(cnt.data(), P.trace_cnt + (size_t)k * (P.episode + 1), sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    memcpy(counts_host, cnt.data() + 1, sizeof(int) * (size_t)P.episode);
    *n_rows = cnt[0];
    int n = cnt[0];
    if (n > P.trace_cap) n = P.trace_cap;
    if (n > max_rows) n = max_rows;
    if (n > 0) TSC_HIP(hipMemcpy(rows_host, P.trace_rows + (size_t)k * P.trace_cap, sizeof(uint4) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_read_record(tsc_env *h, int64_t *ints_host, double *speed_host, int32_t *queue_host) {
    if (!h || !h->P.rec_int || !ints_host || !speed_host || !queue_host) return tsc::fail("tsc_env_read_record: recording is off");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(ints_host, P.rec_int, sizeof(long long) * (size_t)P.E * 8 * 4, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(speed_host, P.rec_speed, sizeof(double) * (size_t)P.E * 8, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(queue_host, P.rec_queue, sizeof(int) * (size_t)P.E * 8 * P.A * P.LMAX, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_read_trips(tsc_env *h, int32_t e, int32_t *trips_host, int32_t max_trips, int32_t *count) {
    if (!h || !h->P.trips || e < 0 || e >= h->P.E || !trips_host || !count) return tsc::fail("tsc_env_read_trips: recording is off");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    int n = 0;
    TSC_HIP(hipMemcpy(&n, P.n_trips + e, sizeof(int), hipMemcpyDeviceToHost));
    *count = n;
    if (n > P.trip_cap) n = P.trip_cap;
    if (n > max_trips) n = max_trips;
    if (n > 0) TSC_HIP(hipMemcpy(trips_host, P.trips + (size_t)e * P.trip_cap * 6, sizeof(int) * (size_t)n * 6, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_counters(tsc_env *h, uint64_t *arrived_host, uint64_t *teleported_host) {
    if (!h || (!arrived_host && !teleported_host)) return tsc::fail("tsc_env_counters: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    if (arrived_host) TSC_HIP(hipMemcpy(arrived_host, h->P.arrived, sizeof(uint64_t) * h->P.E, hipMemcpyDeviceToHost));
    if (teleported_host) TSC_HIP(hipMemcpy(teleported_host, h->P.teleported, sizeof(uint64_t) * h->P.E, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_live_sum(tsc_env *h, double *sum_host, int32_t reset) {
    if (!h || !sum_host) return tsc::fail("tsc_env_live_sum: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> acc(h->P.E);
    TSC_HIP(hipMemcpy(acc.data(), h->P.live_acc, sizeof(unsigned long long) * h->P.E, hipMemcpyDeviceToHost));
    double t = 0;
    for (unsigned long long v : acc) t += (double)v;
    *sum_host = t;
    if (reset) TSC_HIP(hipMemset(h->P.live_acc, 0, sizeof(unsigned long long) * h->P.E));
    return 0;
}

int tsc_env_destroy(tsc_env *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;                                    // (h->bufs frees the device buffers)
    return 0;
}

int tsc_env_set_resident_instances(tsc_env *h, int32_t n_resident) {
    if (!h || n_resident <= 0) return tsc::fail("tsc_env_set_resident_instances: bad arguments");
    pick_workgroup(h, n_resident > h->P.E ? n_resident : h->P.E);
    return plan_step(h, "tsc_env_set_resident_instances");
}

int tsc_env_set_stream(tsc_env *h, void *hip_stream) {
    if (!h) return tsc::fail("null handle");
    h->stream = (hipStream_t)hip_stream;
    return 0;
}

int tsc_env_reset(tsc_env *h, const uint32_t *seeds_host, float *obs_dev) {
    if (!h || !seeds_host || !obs_dev) return tsc::fail("tsc_env_reset: bad arguments");
    h->P.fp_bound = nullptr;                     // reset(): fingerprints <- uniform policy (envs/env.py:556-557)
    h->cf = h->cf_next;                          // tsc_env_set_car_following takes effect here
    h->P.sigma = h->cf == TSC_CF_KRAUSS ? h->sigma_next : 0.0f;
    TSC_HIP(hipMemcpyAsync(h->d_seeds, seeds_host, sizeof(uint32_t) * h->P.E, hipMemcpyHostToDevice, h->stream));
    if (h->P.trace_cnt)                                // tsc_env_trace: cursors and per-second counts start over
        TSC_HIP(hipMemsetAsync(h->P.trace_cnt, 0, sizeof(int) * (size_t)h->n_trace * (h->P.episode + 1), h->stream));
    if (h->ir_dirty) {                                 // tsc_env_set_stream_routes takes effect here
        TSC_HIP(hipMemcpyAsync(h->P.iroute, h->ir_next.data(), sizeof(int) * h->ir_next.size(), hipMemcpyHostToDevice, h->stream));
        h->ir_dirty = false;
    }
    if (h->dem_dirty) {                                // tsc_env_set_demand takes effect here
        EnvDev &P = h->P;
        if (h->dem_next.empty()) { P.emit_tab = h->emit_shared; P.emit_inst = 0; }
        else {
            h->dem_cur = h->dem_next;                  // (the copy reads the vector that no set_demand reassigns)
            TSC_HIP(hipMemcpyAsync(h->dem_vph, h->dem_cur.data(), sizeof(int) * h->dem_cur.size(), hipMemcpyHostToDevice, h->stream));
            {
                tsc::ProfScope ps(tsc::KID_DEMAND, h->stream);
                hipLaunchKernelGGL(demand_kernel, dim3(P.NS, P.E), dim3(256), 0, h->stream, h->dem_rows, h->dem_vph, h->dem_off, h->dem_fl,
                                   P.NS, P.emit_len, h->n_flow);
            }
            TSC_HIP(hipGetLastError());
            P.emit_tab = h->dem_rows; P.emit_inst = P.NS * P.emit_len;
        }
        h->dem_cur = h->dem_next;
        h->dem_dirty = false;
    }
    if (h->Q.hold)                                     // max-pressure hold: age >= min_green, the first decision is free
        TSC_HIP(hipMemsetAsync(h->Q.hold, 0x7F, sizeof(int) * 2 * (size_t)h->P.E * h->P.A, h->stream));
    if (h->D.hold) {                                   // actuated / SOTL: cur = 0, age = min_green (the first decision is free), kappa = 0
        TSC_HIP(hipMemcpyAsync(h->D.hold, h->act_init.data(), sizeof(int) * h->act_init.size(), hipMemcpyHostToDevice, h->stream));
        TSC_HIP(hipMemsetAsync(h->D.kappa, 0, sizeof(int) * (size_t)h->P.E * h->P.A * h->P.PMAX, h->stream));
    }
    h->ld_live = h->P.ld_int != nullptr;               // tsc_env_lane_data takes effect here; its sums start over
    if (h->ld_live) {
        const size_t rows = (size_t)h->P.E * h->ld_nint;
        TSC_HIP(hipMemsetAsync(h->P.ld_int, 0, sizeof(int) * rows * kLdInts * h->P.ld_nslot, h->stream));
        TSC_HIP(hipMemsetAsync(h->P.ld_speed, 0, sizeof(double) * rows * h->P.ld_nslot, h->stream));
    }
    if (plan_step(h, "tsc_env_reset")) return 1;       // the model and the lane data now in force (their setters checked the LDS)
    hipLaunchKernelGGL(reset_kernel, dim3(h->P.E), dim3(h->P.NLP), h->smem, h->stream, h->P, h->d_seeds, obs_dev);
    TSC_HIP(hipGetLastError());
    TSC_HIP(hipStreamSynchronize(h->stream));          // seeds_host may be reused by the caller
    return 0;
}

int tsc_env_set_car_following(tsc_env *h, int32_t model, double sigma) {
    if (!h) return tsc::fail("tsc_env_set_car_following: null handle");
    if (model != TSC_CF_IDM && model != TSC_CF_KRAUSS) return tsc::fail("tsc_env_set_car_following: model %d is neither TSC_CF_IDM (0) nor TSC_CF_KRAUSS (1)", model);
    if (!(sigma >= 0.0 && sigma <= 1.0)) return tsc::fail("tsc_env_set_car_following: sigma %g outside [0, 1]", sigma);
    EnvDev &P = h->P;
    if (model == TSC_CF_KRAUSS && !P.R0) {       // the vehicles' serials (R0), shared with the recording path
        TSC_HIP(hipStreamSynchronize(h->stream));
        TSC_HIP(h->bufs.alloc(&P.R0, (size_t)P.E * kCap * P.NLP, true));
    }
    // what the reset will install, checked here
    if (model == TSC_CF_KRAUSS && step_lds(P, true, false) > kLdsMax)
        return tsc::fail("tsc_env_set_car_following: LDS need %zu B > 160 KiB", step_lds(P, true, false));
    h->cf_next = model;
    h->sigma_next = (float)sigma;
    return 0;
}

int tsc_env_car_following(tsc_env *h, int32_t *model, double *sigma) {
    if (!h || !model || !sigma) return tsc::fail("tsc_env_car_following: bad arguments");
    *model = h->cf;
    *sigma = (double)h->P.sigma;
    return 0;
}

int tsc_env_set_demand(tsc_env *h, const int32_t *vph_host) {
    if (!h) return tsc::fail("tsc_env_set_demand: null handle");
    const EnvDev &P = h->P;
    const int NF = h->n_flow, NS = P.NS;
    if (!vph_host) {                             // back to the scenario's column at the next reset
        h->dem_dirty = h->dem_dirty || !h->dem_next.empty() || !h->dem_cur.empty();
        h->dem_next.clear();
        return 0;
    }
    if (NF < 1) return tsc::fail("tsc_env_set_demand: the scenario has no flows");
    for (int f = 0; f < NF; ++f)                 // (the tables' seconds start at 0: demand_kernel counts an element's seconds from its begin)
        if (h->h_flows[f * 4] < 0) return tsc::fail("tsc_env_set_demand: flow %d begins at second %d < 0", f, h->h_flows[f * 4]);
    // Everything is checked before anything changes.  The flow windows are the scenario's, so the seconds of a stream split into
    // a few segments with one set of overlapping elements each (cut at every begin / end); an element emits at most ceil(vph / 3600)
    // vehicles in a second, so a segment whose elements' bounds add up to <= 255 needs no look at its seconds.
    struct Seg { int r, t0, t1; std::vector<int> fs; };
    std::vector<Seg> segs;
    for (int r = 0; r < NS; ++r) {
        std::vector<int> cuts;
        for (int f = 0; f < NF; ++f)
            if (h->h_flows[f * 4 + 3] == r) {
                cuts.push_back(std::min(std::max(h->h_flows[f * 4], 0), P.emit_len));
                cuts.push_back(std::min(std::max(h->h_flows[f * 4 + 1], 0), P.emit_len));
            }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
            Seg sg{r, cuts[c], cuts[c + 1], {}};
            for (int f = 0; f < NF; ++f)
                if (h->h_flows[f * 4 + 3] == r && h->h_flows[f * 4] <= sg.t0 && h->h_flows[f * 4 + 1] >= sg.t1) sg.fs.push_back(f);
            if (!sg.fs.empty()) segs.push_back(std::move(sg));
        }
    }
    for (int e = 0; e < P.E; ++e) {
        const int32_t *v = vph_host + (size_t)e * NF;
        for (int f = 0; f < NF; ++f)
            if (v[f] < 0) return tsc::fail("tsc_env_set_demand: instance %d flow %d: negative rate %d veh/h", e, f, v[f]);
        for (const Seg &sg : segs) {
            long long bound = 0;
            for (int f : sg.fs) bound += ((long long)v[f] + 3599) / 3600;
            if (bound <= 255) continue;
            for (int t = sg.t0; t < sg.t1; ++t) {
                long long sum = 0;
                for (int f : sg.fs) {
                    const long long tau = t - h->h_flows[f * 4], vph = v[f];
                    sum += (((tau + 1) * vph + 3599) / 3600) - ((tau * vph + 3599) / 3600);
                    if (sum > 255)
                        return tsc::fail("tsc_env_set_demand: instance %d flow %d (%d veh/h): stream %d emits more than 255 vehicles in second %d",
                                         e, f, v[f], sg.r, t);
                }
            }
        }
    }
    if (!h->dem_rows) {                          // first use: the instances' tables and what demand_kernel reads
        (void)hipSetDevice(h->device);
        std::vector<int> off(NS + 1, 0), fl;
        for (int r = 0; r < NS; ++r) {
            for (int f = 0; f < NF; ++f)
                if (h->h_flows[f * 4 + 3] == r) {
                    const int b = std::min(std::max(h->h_flows[f * 4], 0), P.emit_len);
                    const int en = std::min(std::max(h->h_flows[f * 4 + 1], b), P.emit_len);
                    fl.push_back(b); fl.push_back(en); fl.push_back(f);
                }
            off[r + 1] = (int)fl.size() / 3;
        }
        if (fl.empty()) fl.assign(3, 0);
        // (a call that fails half way is completed by the next one)
        const size_t bytes = (size_t)P.E * NS * P.emit_len;
        if (!h->dem_vph) TSC_HIP(h->bufs.alloc(&h->dem_vph, (size_t)P.E * NF, false));
        if (!h->dem_off) TSC_HIP(h->bufs.upload(&h->dem_off, off.data(), off.size()));
        if (!h->dem_fl) TSC_HIP(h->bufs.upload(&h->dem_fl, fl.data(), fl.size()));
        if (h->bufs.alloc(&h->dem_rows, bytes, false) != hipSuccess) {
            (void)hipGetLastError();
            return tsc::fail("tsc_env_set_demand: no device memory for %zu B of per-instance emission tables (%d instances x %d streams x %d s)",
                             bytes, P.E, NS, P.emit_len);
        }
    }
    h->dem_next.assign(vph_host, vph_host + (size_t)P.E * NF);
    h->dem_dirty = true;
    return 0;
}

int tsc_env_demand(tsc_env *h, int32_t *vph_host) {
    if (!h || !vph_host) return tsc::fail("tsc_env_demand: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    const size_t NF = (size_t)h->n_flow;
    for (size_t e = 0; e < (size_t)h->P.E; ++e)
        for (size_t f = 0; f < NF; ++f)
            vph_host[e * NF + f] = h->dem_cur.empty() ? h->h_flows[f * 4 + 2] : h->dem_cur[e * NF + f];
    return 0;
}

int tsc_env_set_stream_routes(tsc_env *h, const int32_t *routes_host) {
    if (!h || !routes_host) return tsc::fail("tsc_env_set_stream_routes: bad arguments");
    const EnvDev &P = h->P;
    if (!P.iroute) return tsc::fail("tsc_env_set_stream_routes: the scenario has no per-episode stream routes");
    std::vector<int> ir((size_t)P.E * P.NS);
    for (int e = 0; e < P.E; ++e)
        for (int s_ = 0; s_ < P.NS; ++s_) {
            int r = h->h_sroute[s_];
            if (h->h_mode[s_] == 2) {
                r = routes_host[(size_t)e * P.NS + s_];
                if (r < 0 || r >= P.NR) return tsc::fail("tsc_env_set_stream_routes: instance %d stream %d: route %d of %d", e, s_, r, P.NR);
                // only a candidate's lanes were walked for the live-lane prefix: another route may lead onto a lane without a thread
                bool cand = false;
                for (int c = 0; c < P.KC && !cand; ++c) cand = h->h_cand[(size_t)s_ * P.KC + c] == r;
                if (!cand) return tsc::fail("tsc_env_set_stream_routes: instance %d stream %d: route %d is not one of the stream's candidates", e, s_, r);
            }
            ir[(size_t)e * P.NS + s_] = r;
        }
    h->ir_next.swap(ir);                         // staged: tsc_env_reset uploads them; a running episode keeps its routes
    h->ir_dirty = true;
    return 0;
}

int tsc_env_bind_fingerprint(tsc_env *h, const float *pi_dev) {
    if (!h) return tsc::fail("null handle");
    h->P.fp_bound = pi_dev;                      // null: back to the copied fingerprints
    return 0;
}

int tsc_env_reward_sum(tsc_env *h, double *sum_host, int32_t reset) {
    if (!h || !sum_host) return tsc::fail("tsc_env_reward_sum: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> acc(h->P.E);
    // armed pressure reward: its own accumulator (step_kernel keeps adding the built-in reward to reward_acc, which nobody reads then)
    TSC_HIP(hipMemcpy(acc.data(), h->R.acc ? h->R.acc : h->P.reward_acc, sizeof(double) * h->P.E, hipMemcpyDeviceToHost));
    double t = 0;
    for (double v : acc) t += v;
    *sum_host = t;
    if (reset) {
        TSC_HIP(hipMemset(h->P.reward_acc, 0, sizeof(double) * h->P.E));
        if (h->R.acc) TSC_HIP(hipMemset(h->R.acc, 0, sizeof(double) * h->P.E));
    }
    return 0;
}

int tsc_env_set_fingerprint(tsc_env *h, const float *pi_dev) {
    if (!h || !pi_dev) return tsc::fail("tsc_env_set_fingerprint: bad arguments");
    h->P.fp_bound = nullptr;
    size_t tot = (size_t)h->P.E * h->P.A * h->P.PMAX;
    tsc::ProfScope ps(tsc::KID_FINGERPRINT, h->stream);
    hipLaunchKernelGGL(fingerprint_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->P, pi_dev);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_env_set_greedy(tsc_env *h, int32_t n_cand_max, int32_t n_term_max, const int32_t *n_cand, const int32_t *term,
                       const int32_t *cand_action) {
    if (!h || !n_cand || !term || !cand_action || n_cand_max <= 0 || n_term_max <= 0)
        return tsc::fail("tsc_env_set_greedy: bad arguments");
    EnvDev &P = h->P;
    std::vector<int8_t> t8((size_t)P.A * n_cand_max * n_term_max);
    for (int a = 0; a < P.A; ++a) {
        if (n_cand[a] <= 0 || n_cand[a] > n_cand_max) return tsc::fail("tsc_env_set_greedy: agent %d has %d candidates of %d", a, n_cand[a], n_cand_max);
        for (int c = 0; c < n_cand_max; ++c) {
            if (c < n_cand[a] && (cand_action[a * n_cand_max + c] < 0 || cand_action[a * n_cand_max + c] >= P.PMAX))
                return tsc::fail("tsc_env_set_greedy: agent %d candidate %d: action %d of %d", a, c, cand_action[a * n_cand_max + c], P.PMAX);
            for (int k = 0; k < n_term_max; ++k) {
                const int j = term[((size_t)a * n_cand_max + c) * n_term_max + k];
                if (j >= P.SMAX || j > 127) return tsc::fail("tsc_env_set_greedy: agent %d candidate %d: observation index %d of %d", a, c, j, P.SMAX);
                t8[((size_t)a * n_cand_max + c) * n_term_max + k] = (int8_t)(j < 0 ? -1 : j);
            }
        }
    }
    (void)hipSetDevice(h->device);
    EnvDev G = P;                                              // the new tables; a second call replaces the old ones
    G.g_ncand = nullptr; G.g_term = nullptr; G.g_action = nullptr;
    G.GC = n_cand_max; G.GT = n_term_max;
    const auto drop = [h](const EnvDev &D) { h->bufs.release(D.g_ncand); h->bufs.release(D.g_term); h->bufs.release(D.g_action); };
    const auto build = [&]() {
        TSC_HIP(h->bufs.upload(&G.g_ncand, n_cand, P.A));
        TSC_HIP(h->bufs.upload(&G.g_term, t8.data(), t8.size()));
        TSC_HIP(h->bufs.upload(&G.g_action, cand_action, (size_t)P.A * n_cand_max));
        TSC_HIP(hipStreamSynchronize(h->stream));              // a running greedy_kernel may still read the old tables
        return 0;
    };
    if (build()) { drop(G); return 1; }
    drop(P);
    P = G;
    return 0;
}

int tsc_env_greedy_actions(tsc_env *h, const float *obs_dev, int32_t *action_dev) {
    if (!h || !obs_dev || !action_dev) return tsc::fail("tsc_env_greedy_actions: bad arguments");
    if (!h->P.g_ncand) return tsc::fail("tsc_env_greedy_actions: no controller tables (tsc_env_set_greedy)");
    const int tot = h->P.E * h->P.A;
    hipLaunchKernelGGL(greedy_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->P, obs_dev, action_dev);
    TSC_HIP(hipGetLastError());
    return 0;
}

// The range checks and the compiled movement tables that tsc_env_set_pressure and tsc_env_set_reward_pressure share: walk = the
// lanes that appear in a movement, ascending; mov_of = lane_route_mov as 16-bit values; mov_dn = a movement's downstream lane as an
// index into walk.  `who` names the caller in the error.  Changes nothing of the handle.
static int compile_movements(const char *who, const EnvDev &P, int measure, int n_mov, const int32_t *mov, const int32_t *lane_route_mov,
                             std::vector<short> &walk, std::vector<short> &mov_of, std::vector<short> &mov_dn) {
    if (measure != TSC_PRESSURE_COUNT && measure != TSC_PRESSURE_QUEUE)
        return tsc::fail("%s: measure %d is neither TSC_PRESSURE_COUNT (0) nor TSC_PRESSURE_QUEUE (1)", who, measure);
    if (n_mov > 4096 || P.A * P.PMAX > 4096)
        return tsc::fail("%s: %d movements, %d (agent, phase) pairs: at most 4096 each", who, n_mov, P.A * P.PMAX);
    std::vector<int> widx((size_t)P.NL, -1);
    for (int i = 0; i < n_mov; ++i) {
        const int a = mov[4 * i], l = mov[4 * i + 1], m = mov[4 * i + 2], k = mov[4 * i + 3];
        if (a < 0 || a >= P.A) return tsc::fail("%s: movement %d names agent %d of %d", who, i, a, P.A);
        if (l < 0 || l >= P.NL || m < 0 || m >= P.NL) return tsc::fail("%s: movement %d names lanes %d -> %d of %d", who, i, l, m, P.NL);
        if (k < 0 || k >= P.KMAX) return tsc::fail("%s: movement %d names signal link %d of %d", who, i, k, P.KMAX);
        widx[l] = widx[m] = 0;
    }
    walk.clear(); mov_of.assign((size_t)P.NL * P.NR, 0); mov_dn.assign((size_t)n_mov, 0);
    for (int l = 0; l < P.NL; ++l)
        if (widx[l] == 0) { widx[l] = (int)walk.size(); walk.push_back((short)l); }
    for (int i = 0; i < n_mov; ++i) mov_dn[i] = (short)widx[mov[4 * i + 2]];
    for (int l = 0; l < P.NL; ++l)
        for (int r = 0; r < P.NR; ++r) {
            const int i = lane_route_mov[(size_t)l * P.NR + r];
            if (i < -1 || i >= n_mov || (i >= 0 && mov[4 * i + 1] != l))
                return tsc::fail("%s: lane %d route %d names movement %d of %d (or one of another lane)", who, l, r, i, n_mov);
            mov_of[(size_t)l * P.NR + r] = (short)i;
        }
    return 0;
}

// compile_movements, then its three tables on the device: fills M through the handle's buffers and *lds with the LDS bytes of
// pressure_walk's arrays (start, down, up, scan scratch).  Changes nothing else of the handle; on failure M holds what was uploaded,
// for the caller to release.
static int upload_movements(const char *who, tsc_env *h, int measure, int n_mov, const int32_t *mov, const int32_t *lane_route_mov,
                            MovDev &M, size_t *lds) {
    std::vector<short> walk, mov_of, mov_dn;
    if (compile_movements(who, h->P, measure, n_mov, mov, lane_route_mov, walk, mov_of, mov_dn)) return 1;
    M.n_mov = n_mov; M.n_walk = (int)walk.size(); M.measure = measure;
    *lds = sizeof(int) * (2 * walk.size() + 1 + (size_t)n_mov + kPressT);
    TSC_HIP(h->bufs.upload(&M.walk, walk.data(), walk.size()));
    TSC_HIP(h->bufs.upload(&M.mov_of, mov_of.data(), mov_of.size()));
    TSC_HIP(h->bufs.upload(&M.mov_dn, mov_dn.data(), mov_dn.size()));
    return 0;
}
static void release_movements(tsc_env *h, const MovDev &M) { h->bufs.release(M.walk); h->bufs.release(M.mov_of); h->bufs.release(M.mov_dn); }

// The range checks and the compiled lists of served [A, PMAX, srv_max] (-1 padded) that tsc_env_set_pressure and tsc_env_set_actuated
// share: phase (a, p) serves the movements srv[off[a * PMAX + p] .. off[.. + 1]).  Changes nothing of the handle.
static int compile_served(const char *who, const tsc_env *h, int n_mov, const int32_t *mov, int srv_max, const int32_t *served,
                          std::vector<int> &off, std::vector<short> &srv) {
    const EnvDev &P = h->P;
    srv.clear(); off.assign((size_t)P.A * P.PMAX + 1, 0);
    for (int a = 0; a < P.A; ++a)
        for (int p = 0; p < P.PMAX; ++p) {
            for (int j = 0; j < srv_max; ++j) {
                const int i = served[((size_t)a * P.PMAX + p) * srv_max + j];
                if (i < 0) break;
                if (p >= h->h_nphase[a]) return tsc::fail("%s: agent %d phase %d of %d serves a movement", who, a, p, h->h_nphase[a]);
                if (i >= n_mov || mov[4 * i] != a) return tsc::fail("%s: agent %d phase %d serves movement %d of %d (or another agent's)", who, a, p, i, n_mov);
                srv.push_back((short)i);
            }
            off[(size_t)a * P.PMAX + p + 1] = (int)srv.size();
        }
    return 0;
}

int tsc_env_set_pressure(tsc_env *h, int32_t measure, int32_t min_green, int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov,
                         int32_t srv_max, const int32_t *served) {
    if (!h || !mov || !lane_route_mov || !served || n_mov < 0 || srv_max <= 0) return tsc::fail("tsc_env_set_pressure: bad arguments");
    if (min_green < 1) return tsc::fail("tsc_env_set_pressure: min_green %d must be >= 1", min_green);
    const EnvDev &P = h->P;
    (void)hipSetDevice(h->device);
    // Build, then swap: the handle's Q changes only when every table of the new one, N, is on the device.
    PressDev N = {};
    size_t smem = 0;
    const auto drop = [h](const PressDev &q) { release_movements(h, q.M); h->bufs.release(q.srv_off); h->bufs.release(q.srv); h->bufs.release(q.hold); };
    const auto build = [&]() {
        if (upload_movements("tsc_env_set_pressure", h, measure, n_mov, mov, lane_route_mov, N.M, &smem)) return 1;
        std::vector<short> srv;
        std::vector<int> off;
        if (compile_served("tsc_env_set_pressure", h, n_mov, mov, srv_max, served, off, srv)) return 1;
        smem += sizeof(int) * (size_t)P.A * P.PMAX;
        if (smem > 48 * 1024) return tsc::fail("tsc_env_set_pressure: LDS need %zu B > 48 KiB (%d walked lanes, %d movements)", smem, N.M.n_walk, n_mov);
        TSC_HIP(h->bufs.upload(&N.srv_off, off.data(), off.size()));
        TSC_HIP(h->bufs.upload(&N.srv, srv.data(), srv.size()));
        N.min_green = min_green;
        N.hold = h->Q.hold;                                    // the hold state: the handle's from the first arming on
        if (!N.hold) TSC_HIP(h->bufs.alloc(&N.hold, 2 * (size_t)P.E * P.A, false));
        TSC_HIP(hipStreamSynchronize(h->stream));              // a running pressure_kernel may still read the old tables
        TSC_HIP(hipMemset(N.hold, 0x7F, sizeof(int) * 2 * (size_t)P.E * P.A));      // age >= min_green: the next decision is free
        return 0;
    };
    if (build()) {                                             // refused: the handle is as it was
        if (N.hold == h->Q.hold) N.hold = nullptr;             // (an armed handle's hold state stays its own)
        drop(N);
        return 1;
    }
    h->Q.hold = nullptr;                                       // (N's now)
    drop(h->Q);
    h->Q = N;
    h->smem_press = smem;
    return 0;
}

int tsc_env_pressure_actions(tsc_env *h, int32_t *action_dev, int32_t *pressure_dev) {
    if (!h || !action_dev) return tsc::fail("tsc_env_pressure_actions: bad arguments");
    if (!h->Q.hold) return tsc::fail("tsc_env_pressure_actions: no controller tables (tsc_env_set_pressure)");
    tsc::ProfScope ps(tsc::KID_PRESSURE, h->stream);
    hipLaunchKernelGGL(pressure_kernel, dim3(h->P.E), dim3(kPressT), h->smem_press, h->stream, h->P, h->Q, action_dev, pressure_dev);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_env_set_actuated(tsc_env *h, int32_t rule, int32_t min_green, int32_t max_green, int32_t theta, int32_t mu, const float *zone_host,
                         int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov, int32_t srv_max, const int32_t *served) {
    const char *who = "tsc_env_set_actuated";
    if (!h || !zone_host || !mov || !lane_route_mov || !served || n_mov < 0 || srv_max <= 0) return tsc::fail("%s: bad arguments", who);
    if (rule != TSC_ACTUATED_GAP && rule != TSC_ACTUATED_SOTL)
        return tsc::fail("%s: rule %d is neither TSC_ACTUATED_GAP (0) nor TSC_ACTUATED_SOTL (1)", who, rule);
    if (min_green < 1) return tsc::fail("%s: min_green %d must be >= 1", who, min_green);
    if (rule == TSC_ACTUATED_GAP && max_green < min_green) return tsc::fail("%s: max_green %d must be >= min_green %d", who, max_green, min_green);
    if (rule == TSC_ACTUATED_SOTL && theta < 1) return tsc::fail("%s: theta %d must be >= 1", who, theta);
    if (rule == TSC_ACTUATED_SOTL && mu < 0) return tsc::fail("%s: mu %d must be >= 0", who, mu);
    const EnvDev &P = h->P;
    for (int l = 0; l < P.NL; ++l)
        if (!(std::isfinite(zone_host[l]) && zone_host[l] > 0.0f)) return tsc::fail("%s: zone of lane %d is %g: must be finite and > 0", who, l, (double)zone_host[l]);
    if (P.PMAX > 32) return tsc::fail("%s: %d phases per agent: the phase mask holds 32", who, P.PMAX);
    // every check before anything changes: the movement tables, the served lists, the LDS need
    std::vector<short> walk_all, mov_of, mov_dn, srv, walk;
    std::vector<int> off;
    if (compile_movements(who, P, TSC_PRESSURE_COUNT, n_mov, mov, lane_route_mov, walk_all, mov_of, mov_dn)) return 1;
    if (compile_served(who, h, n_mov, mov, srv_max, served, off, srv)) return 1;
    std::vector<char> incoming((size_t)P.NL, 0);
    for (int i = 0; i < n_mov; ++i) incoming[mov[4 * i + 1]] = 1;
    for (int l = 0; l < P.NL; ++l)
        if (incoming[l]) walk.push_back((short)l);
    std::vector<unsigned> mask((size_t)n_mov, 0u);
    for (int i = 0; i < P.A * P.PMAX; ++i)
        for (int j = off[i]; j < off[i + 1]; ++j) mask[srv[j]] |= 1u << (i % P.PMAX);
    const size_t smem = sizeof(int) * (walk.size() + 1 + 2 * (size_t)n_mov + 3 * (size_t)P.A * P.PMAX + kPressT);
    if (smem > 48 * 1024) return tsc::fail("%s: LDS need %zu B > 48 KiB (%zu walked lanes, %d movements)", who, smem, walk.size(), n_mov);
    (void)hipSetDevice(h->device);
    // Build, then swap: the handle's D changes only when every table of the new one, N, is on the device.
    ActDev N = {};
    const auto drop = [h](const ActDev &d) {
        h->bufs.release(d.walk); h->bufs.release(d.mov_of); h->bufs.release(d.zone); h->bufs.release(d.srv_off); h->bufs.release(d.srv);
        h->bufs.release(d.mask); h->bufs.release(d.hold); h->bufs.release(d.kappa);
    };
    std::vector<int> init(2 * (size_t)P.E * P.A, 0);
    for (size_t i = 1; i < init.size(); i += 2) init[i] = min_green;
    const auto build = [&]() {
        N.n_mov = n_mov; N.n_walk = (int)walk.size(); N.rule = rule; N.min_green = min_green; N.max_green = max_green; N.theta = theta; N.mu = mu;
        TSC_HIP(h->bufs.upload(&N.walk, walk.data(), walk.size()));
        TSC_HIP(h->bufs.upload(&N.mov_of, mov_of.data(), mov_of.size()));
        TSC_HIP(h->bufs.upload(&N.zone, zone_host, (size_t)P.NL));
        TSC_HIP(h->bufs.upload(&N.srv_off, off.data(), off.size()));
        TSC_HIP(h->bufs.upload(&N.srv, srv.data(), srv.size()));
        TSC_HIP(h->bufs.upload(&N.mask, mask.data(), mask.size()));
        N.hold = h->D.hold; N.kappa = h->D.kappa;              // the state: the handle's from the first arming on
        if (!N.hold) {
            TSC_HIP(h->bufs.alloc(&N.hold, 2 * (size_t)P.E * P.A, false));
            TSC_HIP(h->bufs.alloc(&N.kappa, (size_t)P.E * P.A * P.PMAX, false));
        }
        TSC_HIP(hipStreamSynchronize(h->stream));              // a running actuated_kernel may still read the old tables
        TSC_HIP(hipMemcpy(N.hold, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice));    // the next decision is free
        TSC_HIP(hipMemset(N.kappa, 0, sizeof(int) * (size_t)P.E * P.A * P.PMAX));
        return 0;
    };
    if (build()) {                                             // failed: the handle keeps its tables
        if (N.hold == h->D.hold) { N.hold = nullptr; N.kappa = nullptr; }     // (an armed handle's state stays its own)
        drop(N);
        return 1;
    }
    h->D.hold = nullptr; h->D.kappa = nullptr;                 // (N's now)
    drop(h->D);
    h->D = N;
    h->smem_act = smem;
    h->act_init.swap(init);
    return 0;
}

int tsc_env_actuated_actions(tsc_env *h, int32_t *action_dev, int32_t *counts_dev) {
    if (!h || !action_dev) return tsc::fail("tsc_env_actuated_actions: bad arguments");
    if (!h->D.hold) return tsc::fail("tsc_env_actuated_actions: no controller tables (tsc_env_set_actuated)");
    tsc::ProfScope ps(tsc::KID_ACTUATED, h->stream);
    hipLaunchKernelGGL(actuated_kernel, dim3(h->P.E), dim3(kPressT), h->smem_act, h->stream, h->P, h->D, action_dev, counts_dev);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_env_actuated_state(tsc_env *h, int32_t *hold_host, int32_t *kappa_host) {
    if (!h || !hold_host) return tsc::fail("tsc_env_actuated_state: bad arguments");
    if (!h->D.hold) return tsc::fail("tsc_env_actuated_state: no controller tables (tsc_env_set_actuated)");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(hold_host, h->D.hold, sizeof(int) * 2 * (size_t)P.E * P.A, hipMemcpyDeviceToHost));
    if (kappa_host) TSC_HIP(hipMemcpy(kappa_host, h->D.kappa, sizeof(int) * (size_t)P.E * P.A * P.PMAX, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_set_reward_pressure(tsc_env *h, int32_t measure, int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov) {
    if (!h) return tsc::fail("tsc_env_set_reward_pressure: null handle");
    const EnvDev &P = h->P;
    const auto drop = [h](const PressRewDev &r) { release_movements(h, r.M); h->bufs.release(r.agt_off); h->bufs.release(r.agt_mov); h->bufs.release(r.acc); };
    if (measure == -1) {                                       // disarm: tsc_env_step and tsc_env_reward_sum return to the built-in reward
        if (!h->R.acc) return 0;
        (void)hipSetDevice(h->device);
        TSC_HIP(hipStreamSynchronize(h->stream));              // a running pressure_reward_kernel still reads the tables
        drop(h->R);
        h->R = PressRewDev();
        h->smem_prew = 0;
        // the built-in sum starts over: what step_kernel added to it while the pressure reward was returned is no part of either sum
        TSC_HIP(hipMemset(P.reward_acc, 0, sizeof(double) * P.E));
        return 0;
    }
    if (!mov || !lane_route_mov || n_mov < 0) return tsc::fail("tsc_env_set_reward_pressure: bad arguments (null tables with measure %d)", measure);
    (void)hipSetDevice(h->device);
    // Build, then swap: the handle's R changes only when every table of the new one, N, is on the device.
    PressRewDev N = {};
    size_t smem = 0;
    const auto build = [&]() {
        if (upload_movements("tsc_env_set_reward_pressure", h, measure, n_mov, mov, lane_route_mov, N.M, &smem)) return 1;
        std::vector<short> agt_mov;
        std::vector<int> off((size_t)P.A + 1, 0);              // agent -> movements, each agent's in ascending order
        for (int a = 0; a < P.A; ++a) {
            for (int i = 0; i < n_mov; ++i)
                if (mov[4 * i] == a) agt_mov.push_back((short)i);
            off[(size_t)a + 1] = (int)agt_mov.size();
        }
        smem += sizeof(double) * ((size_t)P.A + 1);
        if (smem > 48 * 1024) return tsc::fail("tsc_env_set_reward_pressure: LDS need %zu B > 48 KiB (%d walked lanes, %d movements)", smem, N.M.n_walk, n_mov);
        TSC_HIP(h->bufs.upload(&N.agt_off, off.data(), off.size()));
        TSC_HIP(h->bufs.upload(&N.agt_mov, agt_mov.data(), agt_mov.size()));
        N.acc = h->R.acc;                                      // the pressure sum: kept across a re-arm, from zero on first arming
        if (!N.acc) TSC_HIP(h->bufs.alloc(&N.acc, (size_t)P.E, true));
        TSC_HIP(hipStreamSynchronize(h->stream));              // a running pressure_reward_kernel may still read the old tables
        return 0;
    };
    if (build()) {                                             // refused: the handle is as it was
        if (N.acc == h->R.acc) N.acc = nullptr;                // (an armed handle's accumulator stays its own)
        drop(N);
        return 1;
    }
    h->R.acc = nullptr;                                        // (N's now)
    drop(h->R);
    h->R = N;
    h->smem_prew = smem;
    return 0;
}

int tsc_env_fixed_time_actions(tsc_env *h, int32_t steps_per_phase, int32_t *action_dev) {
    if (!h || !action_dev) return tsc::fail("tsc_env_fixed_time_actions: bad arguments");
    if (steps_per_phase < 1) return tsc::fail("tsc_env_fixed_time_actions: steps_per_phase %d must be >= 1", steps_per_phase);
    const int tot = h->P.E * h->P.A;
    hipLaunchKernelGGL(fixed_time_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->P, (int)steps_per_phase, action_dev);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_env_step(tsc_env *h, const int32_t *action_dev, float *obs_dev, double *reward_dev,
                 double *global_reward_dev, uint8_t *done_dev, int32_t train_mode) {
    if (!h || !action_dev || !obs_dev || !reward_dev || !global_reward_dev || !done_dev)
        return tsc::fail("tsc_env_step: bad arguments");
    const StepPlan &pl = h->plan;
    if (!pl.v) return tsc::fail("tsc_env_step: the call that last changed the handle's configuration failed");
    {
        tsc::ProfScope ps(tsc::KID_ENV_STEP, h->stream);
        hipLaunchKernelGGL(pl.v->fn, dim3(h->P.E), dim3(pl.threads), pl.lds, h->stream, h->P, action_dev, obs_dev, reward_dev,
                           global_reward_dev, done_dev, (int)train_mode);
    }
    TSC_HIP(hipGetLastError());
    if (h->R.acc) {                                    // tsc_env_set_reward_pressure: the rewards of the state the step left
        {
            tsc::ProfScope ps(tsc::KID_PRESSURE_REWARD, h->stream);
            hipLaunchKernelGGL(pressure_reward_kernel, dim3(h->P.E), dim3(kPressT), h->smem_prew, h->stream, h->P, h->R, reward_dev,
                               global_reward_dev, (int)train_mode);
        }
        TSC_HIP(hipGetLastError());
    }
    return 0;
}

int tsc_env_step_plan(tsc_env *h, int32_t out[7]) {
    if (!h || !out || !h->plan.v) return tsc::fail("tsc_env_step_plan: bad arguments");
    const StepVariant &v = *h->plan.v;
    const int32_t r[7] = {v.maxt, v.help, v.rec, v.kf, v.spec, h->plan.threads, (int32_t)h->plan.lds};
    std::copy(r, r + 7, out);
    return 0;
}

int tsc_env_get_state(tsc_env *h, int32_t e, int32_t *n, float *x, float *v, float *sf, int32_t *w, int32_t *r,
                      int32_t *pending, int32_t *serial, int32_t *time_sec) {
    if (!h || e < 0 || e >= h->P.E) return tsc::fail("tsc_env_get_state: bad arguments");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    const size_t slab = (size_t)kCap * P.NLP;
    std::vector<float4> hs4(slab);
    std::vector<int> hn(P.NLP);
    TSC_HIP(hipMemcpy(hs4.data(), P.S + e * slab, slab * sizeof(float4), hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(hn.data(), P.N + (size_t)e * P.NLP, P.NLP * 4, hipMemcpyDeviceToHost));
    for (int l = 0; l < P.NL; ++l) {
        n[l] = hn[l];
        for (int i = 0; i < kCap; ++i) {
            const bool live = i < hn[l];
            const size_t s = (size_t)vslot(i, l, P.NLP), d = (size_t)l * kCap + i;
            uint32_t mb = 0u;
            if (live) memcpy(&mb, &hs4[s].w, 4);
            x[d] = live ? hs4[s].x : 0.0f; v[d] = live ? hs4[s].y : 0.0f; sf[d] = live ? hs4[s].z : 0.0f;
            w[d] = (int)(mb & 0xFFFFu); r[d] = (int)(mb >> 16);
        }
    }
    if (pending) TSC_HIP(hipMemcpy(pending, P.pending + (size_t)e * P.NS, P.NS * 4, hipMemcpyDeviceToHost));
    if (serial) TSC_HIP(hipMemcpy(serial, P.serial + (size_t)e * P.NS, P.NS * 4, hipMemcpyDeviceToHost));
    if (time_sec) TSC_HIP(hipMemcpy(time_sec, P.tsec + e, 4, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_debug_clock(tsc_env *h, int32_t enable, int64_t *stamps64_host) {
    if (!h) return tsc::fail("null handle");
    TSC_HIP(hipStreamSynchronize(h->stream));
    if (enable && !h->P.dbg) {
        TSC_HIP(h->bufs.alloc(&h->P.dbg, 64 + 7 * (size_t)h->P.E, true));
    }
    if (stamps64_host && h->P.dbg)
        TSC_HIP(hipMemcpy(stamps64_host, h->P.dbg, (enable == 3 ? 64 + 7 * (size_t)h->P.E : enable == 2 ? 64 + 2 * (size_t)h->P.E : 64) * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

int tsc_env_vehicle_counts(tsc_env *h, int32_t *counts_host) {
    if (!h || !counts_host) return tsc::fail("tsc_env_vehicle_counts: bad arguments");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    std::vector<int> hn((size_t)P.E * P.NLP);
    TSC_HIP(hipMemcpy(hn.data(), P.N, hn.size() * 4, hipMemcpyDeviceToHost));
    for (int e = 0; e < P.E; ++e) {
        int tot = 0;
        for (int l = 0; l < P.NL; ++l) tot += hn[(size_t)e * P.NLP + l];
        counts_host[e] = tot;
    }
    return 0;
}

int tsc_env_set_block_order(tsc_env *h, const int32_t *order_host) {
    if (!h) return tsc::fail("tsc_env_set_block_order: null handle");
    TSC_HIP(hipStreamSynchronize(h->stream));
    if (!order_host) { h->P.order = nullptr; return 0; }
    std::vector<char> seen(h->P.E, 0);
    for (int b = 0; b < h->P.E; ++b) {
        const int e = order_host[b];
        if (e < 0 || e >= h->P.E || seen[e]) return tsc::fail("tsc_env_set_block_order: not a permutation of the %d instances", h->P.E);
        seen[e] = 1;
    }
    if (!h->order_buf) TSC_HIP(h->bufs.alloc(&h->order_buf, (size_t)h->P.E, false));
    TSC_HIP(hipMemcpy(h->order_buf, order_host, sizeof(int) * (size_t)h->P.E, hipMemcpyHostToDevice));
    h->P.order = h->order_buf;
    return 0;
}

int tsc_env_live_vehicles(tsc_env *h, double *mean_live) {
    if (!h || !mean_live) return tsc::fail("tsc_env_live_vehicles: bad arguments");
    const EnvDev &P = h->P;
    TSC_HIP(hipStreamSynchronize(h->stream));
    std::vector<int> hn((size_t)P.E * P.NLP);
    TSC_HIP(hipMemcpy(hn.data(), P.N, hn.size() * 4, hipMemcpyDeviceToHost));
    double tot = 0;
    for (int e = 0; e < P.E; ++e)
        for (int l = 0; l < P.NL; ++l) tot += hn[(size_t)e * P.NLP + l];
    *mean_live = tot / P.E;
    return 0;
}

}  // extern "C"
