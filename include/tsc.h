/*
 * tsc.h -- C ABI of the MI355X-native traffic-signal-control hot path.
 *
 * The reference (cts198859/deeprl_signal_control) has no FFI: its boundary is two
 * Python duck-types (env + model) plus the TraCI wire protocol.
 * This header is what a binding for that boundary would bind; every entry point
 * names the reference interface it replaces.  The Python host side that presents
 * the reference's own method names on top of it lives in
 * deeprl_signal_control_amd/{env,agents,trainer}.py (ctypes), and INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; tsc_last_error()
 *     gives the message (thread-local).
 *   - "dev" pointers are device (HBM) pointers owned by the caller (e.g. torch
 *     tensors); "host" pointers are ordinary host memory.  No torch types.
 *   - one HIP stream per handle (tsc_*_set_stream); a handle is not thread-safe,
 *     handles are independent across threads / GPUs.
 *   - E = number of parallel env instances on this GPU, A = agents
 *     (intersections), SMAX / AMAX = padded observation / action widths.
 */
#ifndef TSC_H_
#define TSC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSC_MAX_UP     4   /* feeder lanes per lane                         */
#define TSC_MAX_CROSS  4   /* vehicles leaving one lane per simulated second */
#define TSC_LANE_CAP   28  /* vehicle slots per lane                         */

enum { TSC_AGENT_GREEDY = 0, TSC_AGENT_GLOBAL = 1 /* ia2c, iql */, TSC_AGENT_MA2C = 2 };
enum { TSC_OBJ_QUEUE = 0, TSC_OBJ_WAIT = 1, TSC_OBJ_HYBRID = 2 };
enum { TSC_CF_IDM = 0, TSC_CF_KRAUSS = 1 };        /* car-following model (tsc_env_set_car_following) */
enum { TSC_PRESSURE_COUNT = 0, TSC_PRESSURE_QUEUE = 1 };   /* what a vehicle counts for under max-pressure (tsc_env_set_pressure, tsc_env_set_reward_pressure) */

/* Dense scenario tables (host pointers, copied at create time).  Produced by
 * deeprl_signal_control_amd/scenario.py; meaning and reference provenance of every
 * table is documented there (large_grid/data/build_file.py, envs/large_grid_env.py,
 * envs/env.py:207-254,303-323). */
typedef struct tsc_scenario {
    int32_t n_lane, n_route, n_agent, n_flow;
    int32_t k_max;        /* signal links per agent (padded)   */
    int32_t p_max;        /* phases per agent (padded) = AMAX  */
    int32_t l_max;        /* incoming lanes per agent (padded) */
    int32_t s_max;        /* observation width (padded)        */
    int32_t nbr_max;      /* neighbours per agent (padded)     */
    const float   *lane_len, *lane_vmax, *lane_det_start;      /* [n_lane] */
    const int32_t *lane_node;                                  /* [n_lane] downstream agent or -1 */
    const int32_t *lane_up;                                    /* [n_lane, TSC_MAX_UP] */
    const int32_t *mv_next, *mv_link;                          /* [n_lane, n_route] */
    const int32_t *mv_yield, *mv_prio;                         /* [n_lane, n_route] right of way */
    const int32_t *mv_zip;                                     /* [n_lane, n_route] zipper slot: rank | count << 8 */
    const int32_t *route_entry;                                /* [n_route] */
    const int32_t *flows;                                      /* [n_flow, 4] begin,end,vph,route */
    const int32_t *agent_lanes;                                /* [n_agent, l_max] */
    const int32_t *agent_nlane, *agent_nlink, *agent_nphase;   /* [n_agent] */
    const uint8_t *green_tab;                                  /* [n_agent, p_max, k_max] */
    const uint8_t *yellow_tab;                                 /* [n_agent, p_max(prev), p_max(new), k_max] */
    const int32_t *nbr;                                        /* [n_agent, nbr_max], -1 padded */
    const int32_t *obs_kind, *obs_src;                         /* [n_agent, s_max] */
    /* ENV_CONFIG (config/config_*.ini) */
    int32_t control_interval_sec, yellow_interval_sec, episode_length_sec, teleport_sec;
    int32_t queue_cap;        /* real_net: min(10, halting) (envs/env.py:332-333); -1 = none */
    int32_t objective;        /* TSC_OBJ_*   */
    int32_t agent_kind;       /* TSC_AGENT_* */
    int32_t realnet_scale;    /* envs/env.py:599-601,625-629 */
    double coop_gamma, norm_wave, norm_wait, clip_wave, clip_wait, coef_wait;
    const float *lane_origin;  /* [n_lane] or NULL: where the SUMO lane begins inside a contracted lane chain (scenario.py
                                * contract_chains); the lane.* getters of the recording path count from here */
    /* Insertion streams (round 3).  A stream is one <flow> source: an entry lane, its flow elements (flows[.][3] is then
     * a STREAM index) and the route its vehicles take.  n_stream == 0: every route is its own stream (route_entry[] is the
     * entry lane, the layout of rounds 1-2).  Otherwise, per stream: stream_entry[s] = entry lane; stream_origin[s] = start
     * of the insertion window on it (metres; the SUMO entry lane may be an inner piece of a contracted chain);
     * stream_mode[s]: 0 = fixed route stream_choice[s][0][0];  1 = every vehicle draws its route from stream_choice[s]
     * ({route, cumulative weight of 65536} pairs, k_choice per stream and interval, route -1 pads) with the counter-based hash of
     * (seed, stream, serial) -- SUMO's jtrrouter turn ratios (small_grid/data/build_file.py:223-335);  2 = the route is
     * given per env instance and episode by tsc_env_set_stream_routes() -- the sinks large_grid's init_routes() draws
     * from np.random (large_grid/data/build_file.py:223-266); stream_choice[s] then lists the routes it may take. */
    int32_t n_stream, k_choice;
    const int32_t *stream_entry;   /* [n_stream] */
    const float   *stream_origin;  /* [n_stream] or NULL */
    const float   *stream_limit;   /* [n_stream] or NULL */
    const int32_t *stream_mode;    /* [n_stream] */
    const int32_t *stream_choice;  /* [n_stream, n_interval, k_choice, 2]; the choices in force at second t: interval
                                    * min(t / choice_interval_sec, n_interval - 1) (time-variant turn ratios) */
    int32_t n_interval, choice_interval_sec;
    /* Lane changing on two-lane streets (round 5; MICROSIM_SPEC.md rule 10; SUMO's lane-change model behind simulationStep,
     * envs/env.py:464, with the reference's connection table large_grid/data/build_file.py:107-124): lane_sib[l] = the other lane
     * of lane l's edge or -1; NULL = none.  mv_next then names the lane a junction's CONNECTION enters; a vehicle standing on a
     * lane whose mv_next entry for its route is "not served" (< -1) while lane_sib[l] serves it moves over as a hand-off that keeps
     * its position (lane_up must list the sibling FIRST: lane changers are gathered before the junction's arrivals).  The
     * relation is symmetric (lane_sib[lane_sib[l]] == l) and both lanes of a street have the same lane_len (the position a changer
     * keeps is one on the sibling too); tsc_env_create refuses a scenario that breaks one of the three. */
    const int32_t *lane_sib;       /* [n_lane] or NULL */
} tsc_scenario;

typedef struct tsc_env tsc_env;

const char *tsc_last_error(void);
int tsc_version(void);            /* 100 * major + minor; 124: tsc_iql_set_sharing / tsc_iql_get_sharing / tsc_iql_share_grads; 123: tsc_model_set_sharing / tsc_model_get_sharing / tsc_model_share_grads; 122: tsc_model_dx_split / tsc_dx1w1_f32; 121: tsc_model_dw_split / tsc_dwxh_f32; 120: tsc_env_set_actuated / tsc_env_actuated_actions / tsc_env_actuated_state; 119: tsc_iql_set_return_steps / tsc_iql_get_return_steps / tsc_iql_debug_nstep; 118: tsc_model_plan; 117: tsc_iql_set_dueling / tsc_iql_get_dueling; 116: tsc_iql_set_per / tsc_iql_set_per_beta / tsc_iql_get_priorities / tsc_iql_set_priorities / tsc_iql_debug_per; 115: tsc_iql_set_target / tsc_iql_sync_target / tsc_iql_set_target_params / tsc_iql_get_target_params / tsc_iql_debug_targets; 114: tsc_env_set_reward_pressure; 113: tsc_env_step_plan; 112: tsc_env_set_pressure / tsc_env_pressure_actions / tsc_env_fixed_time_actions; 111: tsc_model_compute_grads_ppo / tsc_model_apply_grads_ex / tsc_model_ppo_stats; 110: tsc_env_set_demand / tsc_env_demand; 109: tsc_env_lane_data / tsc_env_read_lane_data; 108: tsc_env_trace / tsc_env_read_trace; 107: tsc_env_set_car_following / tsc_env_car_following; 106: tsc_model_path; 105: tsc_env_set_greedy / tsc_env_greedy_actions; 104: tsc_env_counters, truncated trips flagged in tsc_env_read_trips */

/* Per-kernel timing with HIP events on the launch stream (bench.py's live roofline figure; the
 * reference has no equivalent).  Off by default; read() synchronises the recorded events.
 * enable(on): 0 = off, 1 = time every launch, n > 1 = time every n-th launch of the kernels that run once per
 * control step (an event pair serialises dependent kernels for a few microseconds); read() then returns
 * total_ms = average of the timed launches x all launches, count = all launches. */
int tsc_profile_enable(int32_t on);
int tsc_profile_reset(void);
/* Time only the kernel ids whose bit is set (0 = all, the default): an event pair between two dependent launches costs the
 * FOLLOWING launch up to ~17 us (the packets behind a kernel that leaves much dirty data), so a kernel's own duration is
 * measured with only ITS launches bracketed; read() of an unselected id returns count without time. */
int tsc_profile_select(uint64_t mask);
int tsc_profile_read(int32_t kernel_id, double *total_ms, int64_t *count);
const char *tsc_profile_name(int32_t kernel_id);   /* "" past the last id */

/* ---- env: replaces TrafficSimulator (envs/env.py:82-635) + SUMO/TraCI ------------------ */

/* TrafficSimulator.__init__ (envs/env.py:83-110) for E parallel instances. */
int tsc_env_create(const tsc_scenario *scn, int32_t n_env, int32_t device, tsc_env **out);
int tsc_env_destroy(tsc_env *h);                               /* terminate(), envs/env.py:563 */
int tsc_env_set_stream(tsc_env *h, void *hip_stream);
/* How many env instances share the DEVICE with this handle's (other handles of the process -- half-batches on separate
 * streams -- or other ranks on the same GPU), this handle's included.  The step kernel's workgroup size follows the device's
 * load, not the handle's: with fewer instances than workgroup slots an instance is spread over 512 / 1024 threads, with a full
 * device it runs 256.  Default: the handle's own n_env.  (No reference counterpart: one SUMO process per env, main.py:93.) */
int tsc_env_set_resident_instances(tsc_env *h, int32_t n_resident);

/* Car-following model of the vehicles (MICROSIM_SPEC.md rule 3): TSC_CF_IDM (the default: IDM acceleration clamped by the Krauss
 * safe speed, no dawdling) or TSC_CF_KRAUSS (SUMO's default model: v = min(v + a, v_safe, v0), then dawdling by sigma in [0, 1],
 * SUMO's default 0.5; 0 = none).  Takes effect at the next tsc_env_reset; the first Krauss call allocates a serial word per vehicle
 * slot (4 B x n_env x 28 x lanes rounded up to 64; shared with tsc_env_record).  Krauss handles run the kernels with runtime
 * table dimensions.  An out-of-range model or sigma is an error (tsc_last_error). */
int tsc_env_set_car_following(tsc_env *h, int32_t model, double sigma);
/* The model and sigma in force (those of the last reset; sigma 0 under TSC_CF_IDM). */
int tsc_env_car_following(tsc_env *h, int32_t *model, double *sigma);

/* reset(), envs/env.py:544-561.  seeds: host [E] (the caller does the reference's
 * `seed += 1` bookkeeping); obs: dev float32 [E, A, SMAX] = float32(state) at t = 0. */
int tsc_env_reset(tsc_env *h, const uint32_t *seeds_host, float *obs_dev);

/* Routes of the mode-2 streams for the NEXT reset(): host int32 [E, n_stream] (entries of other streams are ignored) --
 * what gen_rou_file(seed) would write for every instance's episode seed (the caller draws them; env.py does it with
 * numpy's RandomState(seed), the generator the reference's np.random.seed(seed) + np.random.choice uses).  The routes are kept
 * on the host and uploaded by the next tsc_env_reset: a running episode keeps the routes it was reset with.  A route must be one
 * of its stream's candidates -- stream_choice[s][0][.], up to the first pad -- because only their lanes count as live; any other
 * route is an error (tsc_last_error names instance, stream and route) and the handle keeps the routes it had. */
int tsc_env_set_stream_routes(tsc_env *h, const int32_t *routes_host);

/* Per-instance traffic demand.  vph: host int32 [E, n_flow], the veh/h of flow element f for env instance e in place of
 * flows[f][2]; the elements' windows and streams stay the scenario's.  Takes effect at the NEXT reset() -- a running episode is
 * never touched -- and stays in force until changed; NULL returns the handle to the scenario's own column at the next reset.
 * Checked on the host before anything changes: no negative rate, and no second in which the overlapping elements of a stream
 * emit more than 255 vehicles (the limit of tsc_env_create).  On error the call returns non-zero, tsc_last_error names the
 * instance and the flow, and the handle keeps the demand it had.  The first call allocates the instances' emission tables
 * (E x n_stream x (episode + 64) bytes, written on the device at each reset that installs a new demand: only the E x n_flow
 * rates cross the bus); a handle that never calls it allocates and launches nothing. */
int tsc_env_set_demand(tsc_env *h, const int32_t *vph_host);
/* The [E, n_flow] veh/h column in force since the last reset (the scenario's own, repeated, without tsc_env_set_demand).
 * Synchronises. */
int tsc_env_demand(tsc_env *h, int32_t *vph_host);

/* update_fingerprint(policy), envs/env.py:633-635.  pi: dev float32 [E, A, AMAX];
 * entries k >= n_a - 1 are ignored. */
int tsc_env_set_fingerprint(tsc_env *h, const float *pi_dev);

/* Zero-copy variant of update_fingerprint: the env gathers fingerprints straight from the caller's policy
 * buffer (dev float32 [E, A, AMAX]) at the next step(), which is when the reference reads them; the buffer
 * must stay untouched until then (true for Trainer.explore, utils.py:148-160).  reset() and
 * tsc_env_set_fingerprint() unbind. */
int tsc_env_bind_fingerprint(tsc_env *h, const float *pi_dev);

/* The reference's greedy controllers -- LargeGridController (envs/large_grid_env.py:45-60), RealNetController
 * (envs/real_net_env.py:78-111), SmallGridController (envs/small_grid_env.py:40-55) -- as one rule over tables (what their
 * constructors hold: node names, phase strings, STATE_PHASE_MAP): agent a compares n_cand[a] candidate flows; candidate c is
 * the float64 sum, from 0 and in table order, of the observation entries term[a][c][.] (indices into the agent's
 * observation row, -1 ends the list); np.argmax keeps the first maximum; the winner stands for action cand_action[a][c].
 * Host pointers, int32: n_cand [A], term [A, n_cand_max, n_term_max], cand_action [A, n_cand_max]; copied.
 * deeprl_signal_control_amd/scenario.py:Scenario.greedy_controller_tables compiles them. */
int tsc_env_set_greedy(tsc_env *h, int32_t n_cand_max, int32_t n_term_max, const int32_t *n_cand, const int32_t *term,
                       const int32_t *cand_action);
/* Controller.forward(obs) for every instance (envs/large_grid_env.py:50-54): obs dev float32 [E, A, SMAX] as reset() /
 * step() wrote it, action dev int32 [E, A].  The controllers read the env's float64 state; the kernel recovers it from the
 * float32 entries (a wave entry is a vehicle count / norm_wave, clipped: envs/env.py:439-442), so ties fall as in numpy. */
int tsc_env_greedy_actions(tsc_env *h, const float *obs_dev, int32_t *action_dev);

/* The max-pressure controller (Varaiya 2013; no reference counterpart; INTEGRATION.md "Baseline controllers" states the rule).  A
 * movement is a row of mov [n_mov, 4] = {agent, incoming lane l, downstream lane m, signal link k}; lane_route_mov [n_lane, n_route]
 * names the movement a vehicle of that route takes from that lane, -1 = none (end of the route, or the wrong lane of a two-lane
 * street); served [A, p_max, srv_max] lists, -1 padded, the movements a phase serves (none for p >= n_phase).  Host pointers, int32,
 * copied; deeprl_signal_control_amd/scenario.py:Scenario.pressure_tables compiles them.  With q(vehicle) = 1 (TSC_PRESSURE_COUNT) or
 * 1 only if v < 0.1 m/s (TSC_PRESSURE_QUEUE): up(movement) = sum of q over the vehicles on l whose route takes it, down(m) = sum of
 * q over ALL vehicles on m, pressure(p) = int32 sum over the served movements of up - down(m); p* = the FIRST maximum over p <
 * n_phase.  min_green = g >= 1 control steps: per (instance, agent) the device keeps cur and age; age < g: the action is cur, age += 1;
 * otherwise p* != cur: cur = p*, age = 1; p* == cur: age += 1.  tsc_env_reset and this call set age = g (the next decision is free); g = 1
 * is stateless.  Rejects a bad measure, min_green < 1 and out-of-range agents, lanes, links, movements or phases (tsc_last_error),
 * before anything changes.  Synchronises before replacing tables.  A handle that never calls it allocates and launches nothing. */
int tsc_env_set_pressure(tsc_env *h, int32_t measure, int32_t min_green, int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov,
                         int32_t srv_max, const int32_t *served);
/* The controller's actions from the vehicle state as it stands (pressure_kernel, one workgroup per instance): action dev int32
 * [E, A]; pressure (nullable) dev int32 [E, A, p_max], padded phases 0.  ONE CALL PER CONTROL STEP: a call advances the hold state
 * (cur, age) whenever min_green > 1.  Changes nothing of the simulation. */
int tsc_env_pressure_actions(tsc_env *h, int32_t *action_dev, int32_t *pressure_dev);
/* Gap-based actuated control (SUMO's `actuated`) and self-organising traffic lights (SOTL: Gershenson 2005, Cools et al. 2008); no
 * reference counterpart; INTEGRATION.md "Baseline controllers" states both rules.  rule = TSC_ACTUATED_GAP | TSC_ACTUATED_SOTL.  mov,
 * lane_route_mov, srv_max and served are tsc_env_set_pressure's tables; zone_host float32 [n_lane]: a vehicle on lane l with
 * float32(lane_len[l] - x) <= zone[l] is near the stop line (gap rule: gap seconds x the lane's speed limit; SOTL: omega metres).  Host
 * pointers, copied.  Per movement i: cnt[i] = the vehicles on its incoming lane whose route takes it, near[i] = those of them that
 * are near; per phase p: call(p) = sum of near, dem(p) = sum of cnt over the served movements, red(p | cur) = sum of cnt over the
 * served movements that phase cur does not serve too.  The device keeps cur, age and (SOTL) kappa [p_max] per (instance, agent), all
 * int32; this call and tsc_env_reset set cur = 0, age = min_green (the first decision is free), kappa = 0.
 * Gap rule (min_green = g >= 1, max_green = G >= g control steps; theta and mu are not read): age < g: keep, age += 1; else age < G
 * and call(cur) > 0: keep, age += 1 (the extension); else q = the first of cur + 1, ..., cur + n - 1 (mod n) with dem(q) > 0: none:
 * keep, age = min(age + 1, G); otherwise cur = q, age = 1.
 * SOTL (min_green = g >= 1, theta >= 1 vehicles x control steps, mu >= 0; max_green is not read): first kappa[p] += red(p | cur) for
 * p != cur and kappa[cur] = 0; then age < g: keep, age += 1; else 0 < call(cur) <= mu: keep, age += 1; else q = the FIRST maximum of
 * kappa[p] over p != cur: kappa[q] >= theta: cur = q, age = 1, kappa[q] = 0; otherwise (or with one phase) keep, age += 1.  age
 * saturates at 2^30.
 * Range-checks everything before anything changes (non-zero and tsc_last_error; the handle keeps what it had): a bad rule, min_green
 * < 1, max_green < min_green (gap rule), theta < 1 or mu < 0 (SOTL), a zone entry that is not finite and > 0, p_max > 32, every table
 * error tsc_env_set_pressure rejects, more than 48 KiB of LDS.  Synchronises before replacing tables.  Independent of
 * tsc_env_set_pressure and tsc_env_set_reward_pressure.  A handle that never calls it allocates nothing and launches nothing more. */
enum { TSC_ACTUATED_GAP = 0, TSC_ACTUATED_SOTL = 1 };
int tsc_env_set_actuated(tsc_env *h, int32_t rule, int32_t min_green, int32_t max_green, int32_t theta, int32_t mu, const float *zone_host,
                         int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov, int32_t srv_max, const int32_t *served);
/* The armed rule's actions from the vehicle state as it stands (actuated_kernel, one workgroup per instance): action dev int32 [E, A]
 * = cur after the update; counts (nullable) dev int32 [E, A, p_max, 2] = {call, dem} under the gap rule, {call, red(p | cur before
 * the update)} under SOTL, padded phases 0.  ONE CALL PER CONTROL STEP: a call advances the state.  Changes nothing of the simulation. */
int tsc_env_actuated_actions(tsc_env *h, int32_t *action_dev, int32_t *counts_dev);
/* The controller's state, for tests and checkpoints: hold host int32 [E, A, 2] = {cur, age}, kappa (nullable) host int32 [E, A, p_max]
 * (all 0 under the gap rule).  Synchronises. */
int tsc_env_actuated_state(tsc_env *h, int32_t *hold_host, int32_t *kappa_host);
/* The pressure reward (PressLight / MPLight; no reference counterpart; INTEGRATION.md "Pressure reward" states the rule).  mov and
 * lane_route_mov are tsc_env_set_pressure's (host pointers, int32, copied), up / down and the two measures as there.  While armed,
 * tsc_env_step launches step_kernel exactly as otherwise and then pressure_reward_kernel on the same stream, which OVERWRITES
 * reward_dev and global_reward_dev from the state the step left: P[a] = int32 sum over the movements of agent a of up - down(m),
 * r[a] = -|P[a]|, global_reward[e] = g = sum of r; reward[e, a] is r shaped by the call's train_mode, the agent kind, coop_gamma and
 * realnet_scale exactly as the built-in reward is (queue_cap, coef_wait, norm_wait and clip_wait play no part).  Observations, done,
 * the vehicle state, counters, recording, trace and lane data are untouched.  tsc_env_reward_sum then returns the sum of g, kept in an
 * accumulator of its own that starts at zero when the handle is armed.  measure = -1 disarms (the pointers may be NULL): rewards and
 * tsc_env_reward_sum return to the built-in reward, whose sum starts over at zero.  Arming and disarming take effect at the next
 * tsc_env_step; neither sum spans the change, so arm before an episode if the sum matters.  Independent of tsc_env_set_pressure:
 * tables, measure and hold state of the controller are separate, either may be armed without the other.  Runs the range checks of
 * tsc_env_set_pressure before anything changes (non-zero and tsc_last_error on a bad measure, agent, lane, link or movement, or NULL
 * tables with measure >= 0; the handle keeps what it had).  Synchronises before replacing tables.  A handle that never calls it
 * allocates nothing and launches nothing more. */
int tsc_env_set_reward_pressure(tsc_env *h, int32_t measure, int32_t n_mov, const int32_t *mov, const int32_t *lane_route_mov);
/* Fixed-time cycle: action[e, a] = (t / steps_per_phase) % n_phase[a], t = simulated seconds of instance e / control_interval_sec at
 * the time of the call.  action dev int32 [E, A]; steps_per_phase >= 1.  Needs no tables. */
int tsc_env_fixed_time_actions(tsc_env *h, int32_t steps_per_phase, int32_t *action_dev);

/* Sum over instances and control steps of the global reward since the last reset of the accumulator
 * (what Trainer logs per episode, utils.py:161,296-305): the per-instance sums, each accumulated in step order, added in instance
 * order.  Of the pressure reward's g while tsc_env_set_reward_pressure is armed.  Synchronises. */
int tsc_env_reward_sum(tsc_env *h, double *sum_host, int32_t reset);

/* step(action), envs/env.py:566-631: yellow FSM -> 2 sim-steps -> green -> 3 sim-steps
 * -> detectors -> obs -> reward -> shaping.  action: dev int32 [E, A];
 * obs: dev float32 [E, A, SMAX]; reward: dev float64 [E, A]; global_reward: dev float64 [E];
 * done: dev uint8 [E].  train_mode = 0 returns local rewards (envs/env.py:590-592). */
int tsc_env_step(tsc_env *h, const int32_t *action_dev, float *obs_dev, double *reward_dev,
                 double *global_reward_dev, uint8_t *done_dev, int32_t train_mode);
/* Which step_kernel instantiation tsc_env_step launches right now, and how: out[] = {MAXT (workgroup bound), HELP (flat phase),
 * REC (recording walk), KF (flat-phase vehicles per thread), SPEC, threads per workgroup, bytes of LDS}.  SPEC: 0 runtime table
 * dimensions, 1 large_grid's and 2 Monaco's as compile-time constants, -1 Krauss, -2 trace, -3 Krauss + trace, -4 lane data,
 * -5 Krauss + lane data (the negative ones: runtime dimensions).  Chosen when the handle is created and again by every call that
 * changes an input of the choice (tsc_env_record, tsc_env_trace, tsc_env_lane_data, tsc_env_set_resident_instances,
 * tsc_env_reset -- where a new car-following model and armed lane data take effect), never per step; the rules are in the header
 * comment of csrc/tsc_env.hip and in INTEGRATION.md section 5. */
int tsc_env_step_plan(tsc_env *h, int32_t out[7]);

/* Debug / parity access: vehicle state of env `e` as dense host arrays [n_lane, TSC_LANE_CAP]
 * (front vehicle first) + counts [n_lane] + per-stream pending/serial [n_stream, = n_route without stream tables].
 * Synchronises. */
int tsc_env_get_state(tsc_env *h, int32_t e, int32_t *n, float *x, float *v, float *sf,
                      int32_t *w, int32_t *r, int32_t *pending, int32_t *serial, int32_t *time_sec);

/* Tuning aid: shader-clock stamps (s_memtime) taken by workgroup 0 / thread 0 of the last step at
 * every phase boundary; stamps[63] = number of stamps. enable != 0 allocates the buffer; enable == 2 also
 * returns [64 + 2e], [64 + 2e + 1] = constant-rate (100 MHz) start / end time of workgroup e (host buffer of
 * 64 + 2E entries); enable == 3 also [64 + 2E + 5e + b] = shader-clock cycles workgroup e spent in phase kind b (0 prologue +
 * epilogue, 1 head walk, 2 flat phase, 3 gather + demand, 4 the barriers between them; host buffer of 64 + 7E entries; zeros unless
 * the library was built with -DTSC_ENV_PHASE_SUMS, tools/build_variant.sh). */
int tsc_env_debug_clock(tsc_env *h, int32_t enable, int64_t *stamps64_host);

/* Tuning aids of the simulator's launch geometry.  tsc_env_vehicle_counts: vehicles in the network of every instance (host int32
 * [E]; synchronises).  tsc_env_set_block_order: workgroup b of tsc_env_step simulates instance order[b] (host int32 [E], a
 * permutation; null = identity).  The order changes which instances share a CU, never a result. */
int tsc_env_vehicle_counts(tsc_env *h, int32_t *counts_host);
int tsc_env_set_block_order(tsc_env *h, const int32_t *order_host);

/* Per-instance counters of the running episode, uint64 [E] each (either pointer may be null): vehicles that reached the
 * end of their route (simulation.getArrivedNumber summed over the episode, envs/env.py:413) and vehicles the teleport
 * surrogate removed (SUMO --time-to-teleport, envs/env.py:283-284; they are NOT arrivals).  Host pointers. Synchronises. */
int tsc_env_counters(tsc_env *h, uint64_t *arrived_host, uint64_t *teleported_host);
/* Mean number of live vehicles per env (roofline bookkeeping). Synchronises. */
int tsc_env_live_vehicles(tsc_env *h, double *mean_live);
/* sum over instances and control steps since the last reset of the accumulator of the vehicles in
 * the network at the end of the step: window-mean V = sum / (steps * E)  (SURVEY.md 8d); reset() does not clear it.
 * Synchronises. */
int tsc_env_live_sum(tsc_env *h, double *sum_host, int32_t reset);

/* Evaluation recording = init_data(is_record=True) (envs/env.py:517-528): the following steps also keep, per simulated
 * second, _measure_traffic_step's inputs (envs/env.py:409-437) and a log of finished trips (the --tripinfo-output file
 * collect_tripinfo parses, :498-515).  Off on the training path (separate kernel instantiation).  Call before reset().
 * Refused, with the LDS need in the error, where the recording kernels' arrays do not fit beside the scenario's tables; a refused
 * call changes nothing: the handle goes on as it was. */
int tsc_env_record(tsc_env *h, int32_t enable, int32_t trip_cap);
/* Rows of the LAST step: ints [E, 8, 4] = vehicles in the network, departed, arrived, sum of waiting times of second q <
 * control_interval_sec; speed [E, 8] = sum of speeds; queue [E, 8, A * l_max] = lane.getLastStepHaltingNumber of every
 * incoming lane in (agent, ild) order (-1-padded lanes report 0).  Host pointers. Synchronises. */
int tsc_env_read_record(tsc_env *h, int64_t *ints_host, double *speed_host, int32_t *queue_host);
/* Finished trips of instance e since reset(): rows {route, serial within the route, depart_sec, arrival_sec, waiting
 * seconds, waiting count}; *count = trips finished (may exceed max_trips / the capacity given to tsc_env_record).
 * A row with a NEGATIVE arrival_sec (= -second) is a trip the teleport surrogate truncated (MICROSIM_SPEC.md rule 1): SUMO
 * would have moved that vehicle on and written its tripinfo later, so collect_tripinfo (envs/env.py:498-515) must not
 * count it as a finished trip. */
int tsc_env_read_trips(tsc_env *h, int32_t e, int32_t *trips_host, int32_t max_trips, int32_t *count);
/* Per-vehicle trajectories (SUMO's --fcd-output without coordinates) of n_trace instances, instances_host[k] going to trace k:
 * after every simulated second t < episode_length_sec the recording walk of a traced instance appends one 16-byte row per
 * live vehicle, in (lane, slot) order: {lane | route << 16, depart_sec | serial << 16 (the trip log's ids), x, v} (x, v: the
 * float bits; x from the start of the simulator's lane).  row_cap rows per trace; rows beyond it are dropped but counted.
 * Needs tsc_env_record on; call before reset(), which clears the cursors.  n_trace = 0 detaches the trace (the untraced
 * recording kernels run again).  Rejects out-of-range or repeated instances and row_cap < 1.  Synchronises. */
int tsc_env_trace(tsc_env *h, int32_t n_trace, const int32_t *instances_host, int32_t row_cap);
/* Trace k since reset(): counts_host[episode_length_sec] = rows of every second; rows_host [max_rows][4] = the first
 * min(*n_rows, row_cap, max_rows) rows; *n_rows = rows written and dropped (> row_cap: the buffer overflowed).  Host pointers.
 * Synchronises. */
int tsc_env_read_trace(tsc_env *h, int32_t k, int32_t *counts_host, uint32_t *rows_host, int32_t max_rows, int32_t *n_rows);
/* Per-lane traffic statistics (SUMO's laneData) of every instance, over intervals of period_sec seconds: second t < episode_length_sec
 * counts in interval t / period_sec (n_interval = ceil(episode_length_sec / period_sec)).  A slot is one piece of a lane: the
 * lane_slot0_host[NL + 1] table gives every lane's first slot (a lane's pieces in driving order, one to five; lane_slot0_host[NL]
 * = n_slot), slot_start_host[n_slot] the smallest float position on the lane that lies on the piece (a lane's first piece also takes
 * everything before it), slot_sumo_host[n_slot] the SUMO lane it is a piece of (an index >= 0).  A vehicle belongs to the slot of
 * its lane and position at the end of a second.  Per slot and interval the recording walk sums (in this order): vehicle-seconds,
 * vehicle-seconds with v < 0.1, departed (inserted onto the slot), arrived and teleported (left the network from it), entered / left
 * (a move between slots of different SUMO lanes, other than a lane change: counted on the new / the old slot), laneChangedFrom /
 * laneChangedTo (a rule-10 move to the sibling lane: on the old / the new slot); the speeds as a double: per slot and second a sum
 * of the float speeds in queue order, added up second after second.  period_sec must be a multiple of control_interval_sec, so
 * that a control step lies in one interval.  Needs tsc_env_record on; takes effect at the next reset(), which clears the sums.
 * period_sec <= 0 detaches (the recording kernels without lane data run again).  Works together with tsc_env_trace.
 * Synchronises. */
int tsc_env_lane_data(tsc_env *h, int32_t period_sec, int32_t n_slot, const int32_t *lane_slot0_host, const float *slot_start_host,
                      const int32_t *slot_sumo_host);
/* The sums since reset(), every instance: ints_host [E][n_interval][9][n_slot] in the order above, speed_host
 * [E][n_interval][n_slot].  Host pointers.  Synchronises. */
int tsc_env_read_lane_data(tsc_env *h, int32_t *ints_host, double *speed_host);

/* ---- model: replaces IA2C / MA2C (agents/models.py:132-262) + LstmACPolicy / FPLstmACPolicy
 *      (agents/policies.py:75-211) + OnPolicyBuffer (agents/utils.py:182-228) + the TF1 runtime ---- */

typedef struct tsc_model_cfg {
    int32_t n_agent;          /* A                                                        */
    int32_t s_max, a_max;     /* padded obs / action widths (= tsc_scenario s_max, p_max) */
    const int32_t *n_wave;    /* [A] wave inputs   (policy n_s = env n_s - n_w - n_f)      */
    const int32_t *n_wait;    /* [A] wait inputs   (n_w)                                   */
    const int32_t *n_fp;      /* [A] fingerprint inputs (n_f; 0 for IA2C)                 */
    const int32_t *n_act;     /* [A] actions (n_a)                                        */
    int32_t n_fc_wave, n_fc_wait, n_fc_fp, n_lstm;   /* num_fw, num_ft, num_fp, num_lstm  */
    int32_t n_step;           /* batch_size: control steps per update                     */
    double gamma, reward_norm, reward_clip, value_coef, max_grad_norm, rmsp_alpha, rmsp_epsilon;
    int32_t policy_kind;      /* 0 = LstmACPolicy / FPLstmACPolicy (agents/policies.py:75-211),
                                 1 = FcACPolicy (agents/policies.py:214-256; fingerprints unsupported there) */
} tsc_model_cfg;

typedef struct tsc_model tsc_model;

/* Parameter layout.  Agent-tower group g = 2*agent + tower (0 = pi, 1 = v); every group owns
 * `stride` consecutive floats: W1[s_max][H] (block-diagonal fcw|fcf|fct, obs rows in env order),
 * b1[H], Wx[H][4L], Wh[L][4L], bl[4L], Wo[L][8], bo[8]   (H = n_fc_wave+n_fc_fp+n_fc_wait,
 * L = n_lstm, LSTM gate order i,f,o,u as agents/utils.py:107).  FC policy: Wx -> Wfc[H][L], no Wh, bl -> bfc[L].  out[] = {G, stride, H, L,
 * off_W1, off_b1, off_Wx, off_Wh, off_bl, off_Wo, off_bo, out_pad(8)}. */
int tsc_model_create(const tsc_model_cfg *cfg, int32_t n_env, int32_t device, tsc_model **out);
int tsc_model_destroy(tsc_model *m);
int tsc_model_set_stream(tsc_model *m, void *hip_stream);
int tsc_model_layout(tsc_model *m, int64_t out[12]);
/* Which kernels the FC policy (policy_kind 1) runs, fixed at create time: out[0] = rollout forward, 2 for
 * policy_fwd_fc_mfma_kernel (H = 128 / 160 / 192 / 224, s_max <= 64; not with TSC_FC_MFMA=0 in the environment), 1 for the
 * per-thread policy_fwd_fc_kernel, 0 for the dense GEMMs + head kernel; out[1] = update, 1 for the fused fc_bwd_kernel (same
 * widths; not with TSC_UNFUSED_DX=1), 0 for the grouped split-K GEMMs.  Both -1 for the LSTM policy. */
int tsc_model_path(tsc_model *m, int32_t out[2]);
/* The handle's plan, fixed at create: out[] = {rollout forward (0 Dense, 1 Tile, 2 Ws, 3 FcThread, 4 FcMfma),
 * dwxh, dx1w1, fc_bwd (0 / 1), s_fwd, s_upd}. */
int tsc_model_plan(tsc_model *m, int32_t out[6]);
/* Which kernel the one-pass dWx | dWh | dbl update (plan field dwxh) runs: *out = 1 for dwxh_split_kernel (bf16 matrix cores,
 * every f32 operand cut into three bf16 pieces, six products: f32 accuracy, not bit-equal to the f32 kernel), 0 for the exact-f32
 * dwxh_kernel (TSC_DW_SPLIT=0 in the environment) or when dwxh is 0. */
int tsc_model_dw_split(tsc_model *m, int32_t *out);
/* Which kernel the one-pass first-layer update of the LSTM policy (plan field dx1w1) runs: *out = 1 for dx1w1_split_kernel (the
 * dX1 = dZ Wx^T product on the bf16 matrix cores, both operands cut into three bf16 pieces, six products: f32 accuracy, not
 * bit-equal), 0 for the exact-f32 dx1w1_kernel2 (TSC_DX_SPLIT=0 in the environment) or when dx1w1 is 0.  (tsc_version 122) */
int tsc_model_dx_split(tsc_model *m, int32_t *out);
int tsc_model_set_params(tsc_model *m, const float *params_host);     /* optimizer state untouched */
int tsc_model_reset_opt_state(tsc_model *m);                         /* RMSProp ms <- 1 (TF1 slot init) */
int tsc_model_get_params(tsc_model *m, float *params_host);
int tsc_model_get_opt_state(tsc_model *m, float *ms_host);
int tsc_model_set_opt_state(tsc_model *m, const float *ms_host);

/* Parameter sharing across like-shaped agents (opt-in; no reference counterpart; INTEGRATION.md "Parameter sharing").  class_of_host
 * [A]: class ids in [0, A); agents with the same id form a class and must have equal (n_wave, n_wait, n_fp, n_act), so that their
 * towers have the same layout inside `stride`.  Refused (tsc_last_error names the agents, nothing changes): an id out of range, two
 * agents of one class with unequal dims.  On arming, the lowest-index member's parameters and RMSProp accumulator are copied to the
 * other members (device to device), with the side effects of tsc_model_set_params.  From then on tsc_model_apply_grads(_ex) first
 * replaces every member's gradient slice [a * 2 stride, (a + 1) * 2 stride) by the class mean (share_reduce_kernel: float64 sums in
 * ascending member order, times the float64 1 / k, one rounding to float32) and then runs the unchanged update: the members see the
 * same gradient, norm, parameters and accumulator and stay bit-identical; stats[:, 3] is the class's norm for every member.  Classes
 * of one agent are never read or written.  While armed, tsc_model_set_params / tsc_model_set_opt_state refuse a host buffer in which
 * two members of a class differ (the first differing pair is named).  class_of_host = null disarms and leaves the parameters as they
 * are.  Synchronises.  (tsc_version 123) */
int tsc_model_set_sharing(tsc_model *m, const int32_t *class_of_host);
/* The class ids tsc_model_set_sharing was given; a disarmed handle reports every agent in its own class (class_of_host[a] = a). */
int tsc_model_get_sharing(tsc_model *m, int32_t *class_of_host);
/* Parity hook: the class-mean reduce alone, on the gradient buffer (tsc_model_grad_buffer), on the handle's stream.  A no-op when
 * disarmed. */
int tsc_model_share_grads(tsc_model *m);

/* IA2C.reset (agents/models.py:218-220): zero the forward and backward LSTM states. */
int tsc_model_reset(tsc_model *m);

/* IA2C.forward (agents/models.py:185-200 -> policies.py:125-136).  obs: dev f32 [E,A,SMAX];
 * done: dev u8 [E] (pre-decision done, resets the LSTM state); pi: dev f32 [E,A,AMAX] (padded
 * actions get 0), v: dev f32 [E,A].  advance = 1 <=> out_type contains 'p' (state is advanced);
 * advance = 0 <=> out_type 'v' (bootstrap value, state untouched, policies.py:127-135). */
int tsc_model_forward(tsc_model *m, const float *obs_dev, const uint8_t *done_dev, float *pi_dev,
                      float *v_dev, int32_t advance);

/* forward(out_type='pv') + tsc_model_sample in one call (the action is drawn inside the fused forward).
 * t_slot = index of the transition this forward belongs to (0 .. n_step-1, the slot the following
 * tsc_model_add_transition fills) lets the kernel keep the step's activations for the update, so that
 * tsc_model_compute_grads need not re-evaluate the forward graph (agents/policies.py:94-96 builds it twice);
 * t_slot = -1 disables that.  The cache is used only if all n_step slots were filled in order. */
int tsc_model_forward_sample(tsc_model *m, const float *obs_dev, const uint8_t *done_dev, float *pi_dev,
                             float *v_dev, int32_t *action_dev, uint64_t seed, uint64_t step, int32_t t_slot);

/* np.random.choice(n_a, p=pi) per agent (utils.py:155-157) with a counter-based generator:
 * u = U(seed, step, e, a); action = searchsorted(cumsum(pi)/sum, u, right). action: dev i32 [E,A]. */
int tsc_model_sample(tsc_model *m, const float *pi_dev, int32_t *action_dev, uint64_t seed, uint64_t step);

/* IA2C.add_transition (agents/models.py:222-229): reward / reward_norm, clip, store
 * (obs, action, reward, value, done) at slot t of the on-policy buffer.  reward: dev f64 [E,A]. */
int tsc_model_add_transition(tsc_model *m, int32_t t, const float *obs_dev, const uint8_t *done_pre_dev,
                             const int32_t *action_dev, const double *reward_dev, const float *value_dev,
                             const uint8_t *done_post_dev);

/* Zero-copy rollouts: device pointers of transition slot t of the on-policy buffer, ptrs[6] = {obs f32 [E,A,SMAX],
 * action i32 [E,A], value f32 [E,A], reward f64 [E,A] (raw; normalised / clipped when the returns are computed), done before
 * the step u8 [E], done after the step u8 [E]}.  A caller that lets tsc_model_forward_sample write action / value and
 * tsc_env_step write reward / done / the next observation (slot t + 1; slot n_step exists for that, and is copied to slot
 * 0 by tsc_model_apply_grads) straight into the slots has nothing left for tsc_model_add_transition to do. */
int tsc_model_rollout_slot(tsc_model *m, int32_t t, void *ptrs[6]);

/* IA2C.backward part 1 (agents/models.py:174-183 -> utils.py:202-228 -> policies.py:41-57,138-152):
 * n-step returns/advantages (float64, bootstrap R_boot dev f32 [E,A], ignored where the last
 * transition was terminal), BPTT through the n_step-unrolled LSTM from the saved backward state,
 * loss, gradients.  Gradients land in the contiguous buffer tsc_model_grad_buffer() returns
 * (same layout as the parameters) so the caller can all-reduce it over RCCL. */
int tsc_model_compute_grads(tsc_model *m, const float *R_boot_dev, double entropy_beta);
int tsc_model_grad_buffer(tsc_model *m, float **grad_dev, int64_t *count);

/* IA2C.backward part 2 (policies.py:57-61): per-agent clip_by_global_norm(max_grad_norm) on
 * grad * grad_scale, TF1 RMSPropOptimizer step, states_bw <- states_fw (policies.py:153),
 * buffer reset carrying the last done (utils.py:227).  stats_host (nullable): per agent
 * {policy_loss, value_loss, entropy_loss, grad_norm} float64 [A,4]. */
int tsc_model_apply_grads(tsc_model *m, double lr, double grad_scale, double *stats_host);

/* The PPO update (opt-in; no reference counterpart: the reference takes one RMSProp step per rollout): K epochs over the rollout in
 * the buffer under the clipped surrogate (Schulman et al. 2017) with GAE(lambda) advantages (Schulman et al. 2016).  Epoch k of a
 * rollout is  tsc_model_compute_grads_ppo(.., epoch = k) -> [all-reduce of the gradient buffer] -> tsc_model_apply_grads_ex(..,
 * end_of_rollout = (k == K - 1)).
 *   epoch 0: advantages and returns from the rollout's stored values, once per rollout -- gae_lambda = 1: the n-step returns of
 *     tsc_model_compute_grads, bit for bit; otherwise, in float64 with r the normalised / clipped reward, d the POST-step done and
 *     v_T = R_boot:  delta_t = r_t + gamma v_{t+1} (1 - d_{t+1}) - v_t,  A_t = delta_t + gamma lambda (1 - d_{t+1}) A_{t+1},
 *     R_t = A_t + v_t, both cast to float32; no advantage normalisation.  The epoch also records logp_old[n][a] =
 *     log(clip(pi(a_n), 1e-10, 1)) (float32 [n_step * E][A], allocated by the first call).  The parameters are the rollout's, so
 *     ratio = 1 and the gradient is that of tsc_model_compute_grads; the rollout's activation cache is used when it is valid.
 *   epoch k > 0: re-evaluates the forward from the saved backward state over the stored obs / done with the CURRENT parameters
 *     (the LSTM start state stays the rollout-time one); R_boot is ignored (may be null).  Fails (tsc_last_error) unless epoch 0
 *     ran on the same rollout, i.e. since the last end-of-rollout apply, tsc_model_compute_grads, tsc_model_reset or
 *     tsc_model_set_params (each of them invalidates the advantages, the start state or logp_old of the rollout).
 *   loss, per agent over its N = n_step * E samples:  -mean(min(ratio A, clip(ratio, 1 - clip_eps, 1 + clip_eps) A))
 *     + 0.5 value_coef mean((R - v)^2) - entropy_beta mean(entropy),  ratio = exp(logp - logp_old); value and entropy terms as in
 *     tsc_model_compute_grads, with the current parameters.  A sample's policy gradient is -A ratio / N through logp, and zero
 *     where the clipped branch is the smaller one (A > 0 and ratio > 1 + clip_eps, or A < 0 and ratio < 1 - clip_eps) or pi is
 *     below the 1e-10 clamp.  No minibatches, no value clipping, no KL early stopping.
 * clip_eps > 0, 0 < gae_lambda <= 1.  stats_host of the following apply: policy_loss is the surrogate term. */
int tsc_model_compute_grads_ppo(tsc_model *m, const float *R_boot_dev, double entropy_beta, double clip_eps, double gae_lambda,
                                int32_t epoch);
/* tsc_model_apply_grads with the end-of-rollout bookkeeping (states_bw <- states_fw, done[0] <- done[n_step], obs[0] <-
 * obs[n_step] of a zero-copy rollout) only when end_of_rollout != 0: a PPO epoch that is not the last one must leave them
 * alone, the next epoch's re-forward reads all three.  tsc_model_apply_grads is the end_of_rollout = 1 case. */
int tsc_model_apply_grads_ex(tsc_model *m, double lr, double grad_scale, double *stats_host, int32_t end_of_rollout);
/* Per agent, of the last tsc_model_compute_grads_ppo: {share of the samples whose policy gradient the clip removed,
 * mean(logp_old - logp) (the approximate KL divergence from the rollout's policy)} float64 [A,2].  Host pointer.  Synchronises. */
int tsc_model_ppo_stats(tsc_model *m, double *out_host);

/* Tuning aid for the fused rollout forward: like tsc_env_debug_clock (phase stamps of one workgroup in
 * [0,63), per-workgroup 100 MHz start / end from index 64). */
int tsc_model_debug_clock(tsc_model *m, int32_t enable, int64_t *stamps_host, int32_t count);

/* Debug / parity access: the float32 returns and advantages [n_step, E, A] the last
 * tsc_model_compute_grads() fed to the loss (agents/utils.py:223-224). Synchronises. */
int tsc_model_get_returns(tsc_model *m, float *Rs_host, float *Advs_host);

/* Debug / parity access to the training activations of agent-tower g, rows [row0, row0 + nrows) of the
 * [n_step * E] sample axis (row = t * E + e): what = 0 X1 [H], 1 gates i|f|o|u (dz after compute_grads) [256],
 * 2 h [64], 3 c [64], 4 masked h_prev [64], 5 dH [64].  After n_step tsc_model_forward_sample calls with
 * t_slot = 0..n_step-1 these are the rows the fused forward cached for the update.  Synchronises. */
int tsc_model_debug_read(tsc_model *m, int32_t what, int32_t g, int64_t row0, int64_t nrows, float *out_host);

/* ---- IQL: replaces IQL (agents/models.py:264-376) + LRQPolicy / DeepQPolicy (agents/policies.py:285-389) +
 *      ReplayBuffer (agents/utils.py:231-263) + the TF1 runtime (Adam) ------------------------------------------- */

typedef struct tsc_iql_cfg {
    int32_t n_agent, s_max, a_max;
    const int32_t *n_wave;    /* [A] wave inputs = n_s - n_w  (DeepQPolicy's n_s, agents/models.py:301) */
    const int32_t *n_wait;    /* [A] wait inputs (n_w)                                                  */
    const int32_t *n_act;     /* [A] actions (n_a)                                                      */
    int32_t kind;             /* 0 = LRQPolicy (model_type 'lr'), 1 = DeepQPolicy ('dqn')               */
    int32_t n_fc0, n_h;       /* num_fc, num_h (dqn; the wait FC is n_fc0 / 4 wide, policies.py:359)     */
    int32_t batch_size;       /* minibatch rows per env instance (= n_step, agents/models.py:275)        */
    int32_t buffer_size;      /* replay ring per env instance and agent                                  */
    double gamma, reward_norm, reward_clip, max_grad_norm;
} tsc_iql_cfg;

typedef struct tsc_iql tsc_iql;

/* Parameter layout, `stride` floats per agent:  dqn: W1[s_max][H1] | b1[H1] | W2[H1][H2] | b2[H2] | Wq[H2][8] | bq[8]
 * (H1 = n_fc0 + n_fc0/4, W1 block-diagonal q_fcw | q_fct over the obs in env order);  lr: Wq[s_max][8] | bq[8].
 * out[] = {A, stride, H1, H2, off_W1, off_b1, off_W2, off_b2, off_Wq, off_bq, out_pad(8), kind}. */
int tsc_iql_create(const tsc_iql_cfg *cfg, int32_t n_env, int32_t device, tsc_iql **out);
int tsc_iql_destroy(tsc_iql *h);
int tsc_iql_set_stream(tsc_iql *h, void *hip_stream);
int tsc_iql_layout(tsc_iql *h, int64_t out[12]);
int tsc_iql_set_params(tsc_iql *h, const float *params_host);
int tsc_iql_get_params(tsc_iql *h, float *params_host);
int tsc_iql_get_opt_state(tsc_iql *h, float *m_host, float *v_host, int64_t *adam_t);   /* Adam moments + step count */
int tsc_iql_set_opt_state(tsc_iql *h, const float *m_host, const float *v_host, int64_t adam_t);

/* IQL.forward (agents/models.py:332-348).  obs: dev f32 [E,A,SMAX]; q: dev f32 [E,A,AMAX] (padded actions 0);
 * action: dev i32 [E,A].  mode 0 = argmax ('act'), 1 = 'explore' (u0 < eps ? floor(u1 * n_a) : argmax),
 * 2 = stochastic (qs / sum(qs) -> np.random.choice).  Uniforms: u_s = U(seed, step, 2 * (e * A + a) + s), the
 * counter-based generator of tsc_model_sample. */
int tsc_iql_forward(tsc_iql *h, const float *obs_dev, float *q_dev, int32_t *action_dev, int32_t mode, double eps,
                    uint64_t seed, uint64_t step);

/* IQL.add_transition (agents/models.py:354-361): reward / reward_norm, clip, append (obs, a, r, next_obs, done) to
 * every instance's ring (slot = transitions so far % buffer_size).  reward: dev f64 [E,A]; done: dev u8 [E]. */
int tsc_iql_add_transition(tsc_iql *h, const float *obs_dev, const int32_t *action_dev, const double *reward_dev,
                           const float *next_obs_dev, const uint8_t *done_dev);
int tsc_iql_replay_size(tsc_iql *h, int64_t *size, int64_t *cum_size);       /* ReplayBuffer.size / cum_size */

/* One minibatch step of IQL.backward (agents/models.py:319-330 -> policies.py:305-328), first half: draw batch_size
 * distinct transitions per (instance, agent) -- Floyd's algorithm on U(seed, update_index, (e * A + a) * B + i) --
 * and leave the gradient of mean((Q(s)[a] - stop_grad(done ? r : r + gamma max Q(s')))^2) over the E * batch_size rows
 * of every agent in the contiguous buffer tsc_iql_grad_buffer() returns (parameter layout). */
int tsc_iql_compute_grads(tsc_iql *h, uint64_t seed, uint64_t update_index);
/* The same with the caller's draw instead of the built-in one: idx dev i32 [E, A, batch_size], every entry a ring slot
 * in [0, replay size) -- what ReplayBuffer.sample_transition's random.sample picked (agents/utils.py:252-258); an entry
 * outside that range is clamped into it (never an out-of-bounds read; validate on the host if it matters).  Lets a
 * host that owns the sampling (or a recorded reference run, tests/test_refnet_iql_gpu.py) drive the update. */
int tsc_iql_compute_grads_at(tsc_iql *h, const int32_t *idx_dev);
int tsc_iql_grad_buffer(tsc_iql *h, float **grad_dev, int64_t *count);
/* ... second half: per-agent clip_by_global_norm(max_grad_norm) on grad * grad_scale, TF1 AdamOptimizer step
 * (beta1 .9, beta2 .999, epsilon 1e-8).  stats_host (nullable): per agent {loss, grad_norm} float64 [A,2]. */
int tsc_iql_apply_grads(tsc_iql *h, double lr, double grad_scale, double *stats_host);
/* Debug / parity access: the replay indices [E, A, batch_size] of the last tsc_iql_compute_grads. Synchronises. */
int tsc_iql_debug_batch(tsc_iql *h, int32_t *idx_host);
/* Which learner the handle runs: *fused = 1 when tsc_iql_forward / tsc_iql_compute_grads are the one-kernel DeepQPolicy path
 * (csrc/tsc_iql_fused.h: num_fc 128, num_h 64, s_max <= 48 -- the reference's configurations), 0 for the grouped-GEMM path
 * (IQL-LR, other widths, or TSC_IQL_FUSED=0 in the environment when the handle was created). */
int tsc_iql_path(tsc_iql *h, int32_t *fused);
/* Target network / Double DQN (opt-in; the reference has neither: agents/policies.py:315-318 bootstraps from the network it updates).
 * period = N > 0 arms the handle: a frozen copy theta- of the parameters evaluates the bootstrap value,
 *   double_q = 0:  y = done ? r : r + gamma max_{j < n_a} Q_theta-(s')[j]
 *   double_q = 1:  a* = argmax_{j < n_a} Q_theta(s')[j] (first maximum, np.argmax);  y = done ? r : r + gamma Q_theta-(s')[a*]
 * and the loss stays mean((Q_theta(s)[a] - stop_grad(y))^2).  theta- <- theta when the handle is armed, after every N-th Adam step
 * counted by adam_t (tsc_iql_apply_grads; a device-to-device copy on the handle's stream behind the Adam kernel), and on
 * tsc_iql_sync_target; tsc_iql_set_params does NOT touch it.  The first arming allocates theta- [A][stride] and what the path needs of the
 * per-row targets and picks [A][E * batch_size].  period = 0 disarms: the handle launches what a handle that was never armed launches (double_q must
 * be 0 then -- Double DQN without a target network is the reference's loss under another name).  tsc_iql_compute_grads / _at and
 * tsc_iql_apply_grads keep their signatures; on the fused path an armed step is two launches, the targets (forward only) and the
 * gradient with one row set. */
int tsc_iql_set_target(tsc_iql *h, int32_t period, int32_t double_q);
int tsc_iql_sync_target(tsc_iql *h);                                      /* theta- <- theta (armed handles) */
int tsc_iql_set_target_params(tsc_iql *h, const float *params_host);      /* theta- of an armed handle: checkpoints, tests */
int tsc_iql_get_target_params(tsc_iql *h, float *params_host);
/* Debug / parity access: y [A][E * batch_size] of the last tsc_iql_compute_grads on an armed handle and (nullable) a* of the same
 * rows, -1 unless double_q.  Fused path: the y the target kernel wrote and the gradient kernel read.  Grouped-GEMM path: the device
 * keeps the bootstrap value q1 (max or picked target value) and iql_td_kernel forms y in registers, so y is restated here on the
 * host from the device's q1, reward and done rows with the kernel's float32 expression -- what is checked there is q1 and a*.
 * Synchronises. */
int tsc_iql_debug_targets(tsc_iql *h, float *y_host, int32_t *astar_host);
/* Prioritized experience replay (opt-in; proportional, Schaul et al. 2016; the reference samples uniformly).  Every ring (e, a) keeps a
 * stored priority q[s] >= 0 per slot -- already (|delta| + eps)^alpha, float32, laid out prio[E][A][cap] -- and a running maximum
 * qmax[e][a] that starts at 1.  On an armed handle
 *   tsc_iql_add_transition   sets q[slot] = qmax[e][a] in every ring (iql_per_add_kernel behind iql_add_kernel);
 *   tsc_iql_compute_grads    draws stratified, proportional, with replacement (iql_per_sample_kernel): C[k] = sum_{s <= k} q[s] over the
 *       filled slots in float64, total = C[size - 1]; pick i of ring p = e A + a has the target t_i = (i + U(seed, update_index,
 *       p batch_size + i)) total / batch_size (U: the counter-based uniform of the Floyd draw) and is the smallest k with C[k] > t_i,
 *       clamped to the last slot with q > 0; a slot with q = 0 or >= size is never picked;
 *   the importance weight of a row is w_i = (size q[k_i] / total)^-beta in float64 (product, quotient, pow), divided by the largest of the
 *       ring's own batch_size weights and stored as float32 in w[A][E * batch_size]; loss = (1 / R) sum w delta^2, dLoss/dQ[a] = 2 w delta / R
 *       with delta = Q(s)[a] - y exactly as without it, under any tsc_iql_set_target setting;
 *   at the end of tsc_iql_compute_grads / _at (nothing from the all-reduce is needed) q[k] = (float)pow((double)|delta| + eps, alpha) for
 *       every sampled row and qmax rises to the largest such value; a ring's picks are written in order, so the last pick of a slot drawn
 *       twice stays;
 *   tsc_iql_compute_grads_at takes the caller's indices as given (clamped as before), forms the weights from the priorities of those slots by the
 *       same formula (a slot with q = 0 takes the ring's largest weight) and writes back as above.
 * On the fused path an armed step always takes the two-launch route of tsc_iql_set_target (without a target network the targets come from
 * the parameters themselves).  The sampler stages one whole ring in LDS: arming refuses buffer_size > TSC_IQL_PER_MAX_BUFFER.
 * alpha >= 0, eps > 0.  The first arming allocates prio / qmax / w / td, with q = 1 on filled slots and qmax = 1; arming with another alpha,
 * or again after a disarm, resets them.  enable = 0 disarms: back to the Floyd draw and the kernels of a handle that was never armed. */
#define TSC_IQL_PER_MAX_BUFFER 4096
int tsc_iql_set_per(tsc_iql *h, int32_t enable, double alpha, double eps);
int tsc_iql_set_per_beta(tsc_iql *h, double beta);              /* beta in [0, 1]; default 1 */
/* prio [E][A][cap], qmax [E][A] of an armed handle.  set: tests; every value finite and >= 0, every ring with at least one positive value among
 * its filled slots.  Both synchronise. */
int tsc_iql_get_priorities(tsc_iql *h, float *prio_host, float *qmax_host);
int tsc_iql_set_priorities(tsc_iql *h, const float *prio_host, const float *qmax_host);
/* Debug / parity access: w and |delta| [A][E * batch_size] of the last tsc_iql_compute_grads / _at on an armed handle.  Synchronises. */
int tsc_iql_debug_per(tsc_iql *h, float *w_host, float *td_host);
/* Dueling Q-network head for IQL-DNN (opt-in; Wang et al. 2016; the reference's head is plain).  The parameter layout does not change: with
 * out[0..7] = X2 Wq + bq the head's eight outputs as every kernel computes them, column 7 of Wq | bq becomes the value stream and
 *   A_j = out[j] (j < n_a),  V = out[7],  Q[j] = V + A_j - (1 / n_a) sum_{k < n_a} A_k   (j < n_a).
 * Q replaces out[0 .. n_a) wherever a Q value is used: the greedy / epsilon-greedy / stochastic action choice, q_out (padding stays 0, V
 * is never exposed), max_j Q(s'), Double DQN's a* (first maximum of the combined online values, evaluated on the combined target values),
 * Q(s)[a] in the TD error and the |delta| prioritized replay stores.  The loss stays mean(w (Q(s)[a] - stop_grad(y))^2) under every
 * tsc_iql_set_target / tsc_iql_set_per setting.  Backward, with g = dLoss/dQ[a] of the row: dOut[j] = g (delta_ja - 1 / n_a) for j < n_a,
 * dOut[7] = g, dOut[j] = 0 for n_a <= j < 7 (those columns of the gradient stay exactly zero), so dX2 = relu'(X2) g (Wq[:, a] + u) with
 * u = Wq[:, 7] - (1 / n_a) sum_{k < n_a} Wq[:, k], and dWq | dbq contract X2 | 1 against the dense dOut.
 * enable = 1 arms; it refuses kind = 0 (a linear Q with a value column spans the same functions) and any n_act[a] > 7 (never clamped), and
 * touches neither parameters nor optimizer state.  The first arming allocates |delta| and a weight vector of ones [A][E * batch_size] (the
 * dueling kernels always take weights) and, on the fused path, the per-row targets.  On the fused path a dueling step always takes the
 * two-launch route of tsc_iql_set_target, as prioritized replay does.  enable = 0 disarms: the handle launches what a handle that was never
 * armed launches.  tsc_iql_forward, tsc_iql_compute_grads / _at and tsc_iql_apply_grads keep their signatures; tsc_iql_debug_targets also
 * answers on a dueling handle without a target network (a* = -1 unless double_q). */
int tsc_iql_set_dueling(tsc_iql *h, int32_t enable);
int tsc_iql_get_dueling(tsc_iql *h, int32_t *enabled);          /* 1 while the dueling head is armed */
/* Multi-step (n-step) returns (opt-in; Sutton 1988, the n-step component of Rainbow; the reference bootstraps after one control step).
 * Nothing changes at tsc_iql_add_transition: the window of a sampled row is walked at sample time over the rewards and done flags of its
 * ring.  For a sampled slot s of instance e, agent a, with the newest slot w = (cum - 1) mod cap:
 *   j = s; G = 0; c = 1; k = 0
 *   repeat:  G += c r[e][j][a];  c *= gamma;  k += 1;  stop if done[e][j] or j == w or k == n;  j = (j + 1) mod cap
 *   y = done[e][j] ? G : G + c Qsel(next_obs[e][j][a])                              (c = gamma^k, 1 <= k <= n)
 * Qsel is whatever the handle is armed with (max of the net being updated, max of the frozen copy, Double DQN's pick, each on the combined
 * values of a dueling handle).  The window never runs past an episode end nor past the newest transition -- a row cut by the newest slot
 * bootstraps early with its own gamma^k -- and n >= cap is harmless (the walk meets w before it returns to s).  G and c are accumulated in
 * float64 over the ring's float32 rewards and rounded to float32 once per row.  Q(s)[a], the action, the importance weight and the
 * priority write-back stay those of slot s; with prioritized replay |delta| is taken against the n-step target.  k = 1 on every row is the
 * one-step target.  PRECONDITION (not checked): between two done flags, consecutive slots of a ring hold consecutive steps of one
 * trajectory -- a caller who feeds tsc_iql_add_transition by hand must keep that.
 * 1 <= n <= TSC_IQL_MAX_RETURN_STEPS, refused outside; n = 1 disarms: the handle launches what a handle that was never armed launches.  May
 * be called at any time; the rings are untouched.  The first arming allocates the pre-pass outputs [A][E * batch_size] and, on the fused
 * path, the per-row targets; an armed step runs iql_nstep_kernel (profile id iql_nstep) behind the draw and, on the fused path, always
 * takes the two-launch route of tsc_iql_set_target.  tsc_iql_debug_targets also answers on a return-steps handle. */
#define TSC_IQL_MAX_RETURN_STEPS 32
int tsc_iql_set_return_steps(tsc_iql *h, int32_t n);
int tsc_iql_get_return_steps(tsc_iql *h, int32_t *n);
/* Debug / parity access: the pre-pass outputs of the last tsc_iql_compute_grads / _at with return_steps > 1 -- the bootstrap slot j
 * [E][A][batch_size] (the layout of tsc_iql_debug_batch) and G, gamma^k, k [A][E * batch_size].  Refused before the first such step.
 * Synchronises. */
int tsc_iql_debug_nstep(tsc_iql *h, int32_t *slot_host, float *ret_host, float *disc_host, int32_t *k_host);
/* Parameter sharing across like-shaped agents (opt-in; no reference counterpart; INTEGRATION.md "Parameter sharing"; the Q-learners'
 * twin of tsc_model_set_sharing).  class_of_host [A]: class ids in [0, A); agents with the same id form a class and must have equal
 * (n_wave, n_wait, n_act), so that their rows of the [A][stride] layout have the same layout, rowrange mask and action count.  Refused
 * (tsc_last_error names the agents, nothing changes): an id out of range, two agents of one class with unequal dims, a stride that is
 * no multiple of 4.  On arming, the lowest-index member's parameters, both Adam moments and -- where a target network is armed -- the
 * frozen copy are copied to the other members (device to device), with the side effects of tsc_iql_set_params; the Adam step count is
 * the handle's already.  From then on tsc_iql_apply_grads first replaces every member's gradient slice [a * stride, (a + 1) * stride)
 * by the class mean (share_reduce_kernel: float64 sums in ascending member order, times the float64 1 / k, one rounding to float32;
 * inside the iql_adam profile scope, behind the caller's all-reduce) and then runs the unchanged norm + clip + Adam: the members see
 * the same gradient, norm, parameters and moments and stay bit-identical; stats[a][1] is the class's norm for every member, stats[a][0]
 * stays the member's own loss.  The rings, the draw, the priorities and their write-back, the n-step windows and the forward stay per
 * agent.  Classes of one agent are never read or written.  While armed, tsc_iql_set_params, tsc_iql_set_opt_state and
 * tsc_iql_set_target_params refuse a host buffer in which two members of a class differ (the first differing pair is named; nothing
 * is uploaded); tsc_iql_set_target / tsc_iql_sync_target copy theta and so keep the members equal by themselves.  The order of arming
 * relative to tsc_iql_set_target, tsc_iql_set_per, tsc_iql_set_dueling and tsc_iql_set_return_steps does not matter.  class_of_host =
 * null disarms and leaves everything as it is.  Synchronises.  (tsc_version 124) */
int tsc_iql_set_sharing(tsc_iql *h, const int32_t *class_of_host);
/* The class ids tsc_iql_set_sharing was given; a disarmed handle reports every agent in its own class (class_of_host[a] = a). */
int tsc_iql_get_sharing(tsc_iql *h, int32_t *class_of_host);
/* Parity hook: the class-mean reduce alone, on the gradient buffer (tsc_iql_grad_buffer), on the handle's stream.  A no-op when
 * disarmed. */
int tsc_iql_share_grads(tsc_iql *h);
/* Measurement hook of the fused learner (tools/bench_iql.py --stamps): enable != 0 allocates the stamp buffer; the next
 * tsc_iql_compute_grads then records, for every workgroup, its start / end on the 100-MHz wall clock ([64 + 2 b],
 * [64 + 2 b + 1]) and -- in a measurement build with -DTSC_IQL_STAMPS (tools/build_variant.sh; the stamps' branches are kept
 * out of the product kernel) -- for workgroup 0 eleven shader-clock stamps per wavefront around the phases of its third 64-row
 * chunk ([16 w + k], csrc/tsc_iql_fused.h QSTAMP).  On an armed handle (tsc_iql_set_target) the target kernel's workgroups leave
 * their start / end behind the gradient kernel's ([64 + 2 W + 2 b], W = workgroups).  stamps_host (nullable) receives
 * min(count, 64 + 4 x workgroups) values; count < 0 is refused.  enable = 0 detaches the buffer: the kernels stop stamping, what
 * was recorded stays readable.  Synchronises. */
int tsc_iql_debug_clock(tsc_iql *h, int32_t enable, int64_t *stamps_host, int32_t count);

/* Test hook: the grouped fp32 MFMA GEMM used by every layer.  form: 0 = NN, 1 = TN; epi as
 * csrc/tsc_gemm.h.  All pointers device; strides in elements.  A non-null split-K workspace lets
 * the TN form cut its reduction into deterministic chunks (as the weight-gradient GEMMs do). */
int tsc_gemm_grouped_f32(int32_t form, int32_t epi, int32_t groups, int32_t M, int32_t N, int32_t K,
                         const float *A, int64_t sA, int32_t lda, const float *B, int64_t sB, int32_t ldb,
                         float *C, int64_t sC, int32_t ldc, const float *bias, const float *aux,
                         const int16_t *rowrange, float *colsum, float *splitk_ws, int64_t ws_floats,
                         float *splitk_wsc, int64_t wsc_floats, void *hip_stream);

/* Test hook: the LSTM weight-gradient pass of the update on caller-supplied DEVICE inputs.  X1 [G][N][H], Hp [G][N][64],
 * dZ [G][N][256] -> out [G][H + 64 + 1][256] = [X1 | Hp]^T dZ ; colsum(dZ) per tower, over S row splits added in split
 * order.  H is one of 128 / 160 / 192 / 224.  split != 0 runs dwxh_split_kernel, 0 the exact-f32 dwxh_kernel.  Synchronises. */
int tsc_dwxh_f32(int32_t H, int64_t N, int32_t G, int32_t S, const float *X1, const float *Hp, const float *dZ, float *out,
                 int32_t split);

/* Test hook: the first-layer pass of the LSTM update on caller-supplied DEVICE inputs.  dZ [G][N][256], X1 [G][N][H] (the relu
 * mask: X1 > 0), Wx [G][H][256], obs [N][G / 2][SMAX] (towers 2a and 2a + 1 read agent a), ftm [G / 2][H / 16] (bit t: feature
 * tile t of dW1 has a structural non-zero in the column unit), rowrange [G / 2][SMAX][2] (hidden columns [lo, hi) an obs row
 * feeds) -> out [G][SMAX + 1][H] = dW1 = obs^T dX1 inside the structure | db1 = colsum(dX1), dX1 = (dZ Wx^T) * [X1 > 0], over S
 * row splits added in split order.  H is one of 128 / 160 / 192 / 224, SMAX a multiple of 4 up to 64, G even.  split != 0 runs
 * dx1w1_split_kernel, 0 the exact-f32 dx1w1_kernel2.  Synchronises.  (tsc_version 122) */
int tsc_dx1w1_f32(int32_t H, int64_t N, int32_t G, int32_t S, int32_t SMAX, const float *dZ, const float *X1, const float *Wx,
                  const float *obs, const int32_t *ftm, const int16_t *rowrange, float *out, int32_t split);

#ifdef __cplusplus
}
#endif
#endif /* TSC_H_ */
