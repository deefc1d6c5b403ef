// tsc_iql.hip -- independent Q-learning agents (IQL-LR / IQL-DNN) on gfx950.
//
// Replaces, for all agents of all env instances at once:
//   IQL.forward ............ agents/models.py:332-348  (epsilon-greedy over per-agent Q nets)
//   IQL.add_transition ..... agents/models.py:354-361  (reward norm / clip) + ReplayBuffer (agents/utils.py:231-263)
//   IQL.backward ........... agents/models.py:319-330  -> QPolicy.prepare_loss (agents/policies.py:305-328):
//                            loss = mean((Q(s)[a] - stop_grad(done ? r : r + gamma max Q(s')))^2) with the SAME network for
//                            Q(s') (no target network), tf.clip_by_global_norm per agent, tf.train.AdamOptimizer
//   LRQPolicy / DeepQPolicy  agents/policies.py:343-389: q = fc(S -> n_a)  /
//                            [relu(fc(wave -> n_fc0)), relu(fc(wait -> n_fc0/4))] -> relu(fc(. -> n_h)) -> fc(-> n_a)
//
// Batched over E env instances the way the A2C learner is: every instance keeps its own ring of `buffer_size`
// transitions per agent; one minibatch step draws `batch_size` distinct transitions from EVERY instance's ring
// (counter-based Floyd sampling, one draw per (instance, agent)) and the loss is the mean over the E * batch_size rows of
// an agent -- E = 1 is the reference.  Parameters, gradients and both Adam moments share one flat layout per agent
//   DQN: W1[SMAX][H1] | b1[H1] | W2[H1][H2] | b2[H2] | Wq[H2][8] | bq[8]     (W1 block-diagonal: wave rows -> columns
//        [0, n_fc0), wait rows -> [n_fc0, H1); structural zeros kept zero by the row-range mask on its gradient)
//   LR : Wq[SMAX][8] | bq[8]
// so the gradient buffer is one contiguous all-reduce.  Every contraction runs on the grouped fp32 MFMA GEMM of
// tsc_gemm.h (groups = agents); the element-wise pieces (sampling, gather, TD target, Adam) are small HBM-bound kernels.
#include "tsc_common.h"
#include "tsc_gemm.h"
#include "tsc_share.h"
#include "../../include/tsc.h"

#include <cassert>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

using tsc::GemmArgs;
constexpr int kQ = 8;              // padded action width (n_a <= 8)

struct QLayout {
    int A, SMAX, AMAX, H1, H2, dqn;
    long long stride, oW1, ob1, oW2, ob2, oWq, obq;
};

// a replay index clamped into the filled part [0, size) of its ring: a caller-supplied draw never reads out of bounds
__device__ __forceinline__ int iql_ring_slot(int s, int size) { return s < 0 ? 0 : s >= size ? size - 1 : s; }

// IQL.forward (agents/models.py:332-348): mode 0 = argmax, 1 = explore (np.random.random() < eps -> randint), 2 = stochastic
// (qs / sum(qs) -> np.random.choice).  One thread per (instance, agent); q rows come from the Q GEMM.  (iql_fused_act_kernel states the same
// rule over registers: one shared function changed that kernel's register allocation, so the rule stays written in both.)
__global__ void iql_act_kernel(const float *Q, const int *n_act, int E, int A, int AMAX, int mode, double eps,
                               unsigned long long seed, unsigned long long step, float *q_out, int *action) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * A) return;
    const int e = idx / A, a = idx % A, na = n_act[a];
    const float *q = Q + ((long long)a * E + e) * kQ;
    for (int k = 0; k < AMAX; ++k) q_out[(long long)idx * AMAX + k] = k < na ? q[k] : 0.f;
    int best = 0;
    for (int k = 1; k < na; ++k) if (q[k] > q[best]) best = k;          // np.argmax: first maximum
    int act = best;
    if (mode == 1) {
        const double u0 = uniform01(seed, step, 2ull * idx), u1 = uniform01(seed, step, 2ull * idx + 1);
        if (u0 < eps) { act = (int)(u1 * (double)na); if (act >= na) act = na - 1; }
    } else if (mode == 2) {
        double s = 0.0;
        for (int k = 0; k < na; ++k) s += (double)q[k];
        const double u = uniform01(seed, step, 2ull * idx);
        double c = 0.0, tot = 0.0;
        for (int k = 0; k < na; ++k) tot += (double)q[k] / s;
        act = na - 1;
        for (int k = 0; k < na; ++k) { c += (double)q[k] / s; if (u < c / tot) { act = k; break; } }
    }
    action[idx] = act;
}

// ReplayBuffer.add_transition for slot `slot` of every instance's ring; rewards normalised / clipped in float64
// (agents/models.py:355-358) and stored as the float32 the TF placeholder holds.
__global__ void iql_add_kernel(int E, int A, int SMAX, long long cap, long long slot, const float *obs, const int *action,
                               const double *reward, const float *next_obs, const uint8_t *done, double rnorm, double rclip,
                               float *r_obs, float *r_next, int *r_act, float *r_rew, uint8_t *r_done) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)A * SMAX;
    if (i < (long long)E * per) {
        const long long e = i / per, j = i % per;
        r_obs[(e * cap + slot) * per + j] = obs[i];
        r_next[(e * cap + slot) * per + j] = next_obs[i];
    }
    if (i < (long long)E * A) {
        const long long e = i / A, a = i % A;
        double r = reward[i];
        if (rnorm != 0.0) r = r / rnorm;
        if (rclip != 0.0) r = fmin(fmax(r, -rclip), rclip);
        r_rew[(e * cap + slot) * A + a] = (float)r;
        r_act[(e * cap + slot) * A + a] = action[i];
    }
    if (i < E) r_done[i * cap + slot] = done[i];
}

// random.sample(buffer, batch_size) per (instance, agent) (agents/utils.py:251-253), as Floyd's algorithm on the
// documented counter-based uniform: for i in [0, B): j = size - B + i; t = floor(U * (j + 1)); pick t, or j if t was
// picked before.  idx [E][A][B].
__global__ void iql_sample_kernel(int E, int A, int B, long long size, unsigned long long seed, unsigned long long upd, int *idx) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E * A) return;
    int *out = idx + (long long)p * B;
    for (int i = 0; i < B; ++i) {
        const long long j = size - B + i;
        const double u = uniform01(seed, upd, (unsigned long long)p * B + i);
        long long t = (long long)(u * (double)(j + 1));
        if (t > j) t = j;
        bool seen = false;
        for (int q = 0; q < i; ++q) seen |= out[q] == (int)t;
        out[i] = seen ? (int)j : (int)t;
    }
}
// the same draw for a compile-time batch size (the reference's 20, config/config_iql*.ini): the picks stay in registers instead of
// being re-read from the index buffer for every membership test (16.5 -> ~ 5 us at E = 1024)
template <int BB>
__global__ void iql_sample_fixed_kernel(int E, int A, long long size, unsigned long long seed, unsigned long long upd, int *idx) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E * A) return;
    int pk[BB];
#pragma unroll
    for (int i = 0; i < BB; ++i) {
        const long long j = size - BB + i;
        const double u = uniform01(seed, upd, (unsigned long long)p * BB + i);
        long long t = (long long)(u * (double)(j + 1));
        if (t > j) t = j;
        bool seen = false;
#pragma unroll
        for (int q = 0; q < i; ++q) seen |= pk[q] == (int)t;
        pk[i] = seen ? (int)j : (int)t;
    }
    int *out = idx + (long long)p * BB;
#pragma unroll
    for (int i = 0; i < BB; ++i) out[i] = pk[i];
}

// minibatch rows of agent a: row = e * B + i  <-  transition idx[e][a][i] of instance e
// (a caller-supplied index outside the filled part [0, size) of the ring is clamped into it: no out-of-bounds read)
// S and the action are those of the sampled slot (idx), S1 and done those of the bootstrap slot (boot): idx itself on a one-step handle,
// ns_slot of a return-steps one.  The row's reward is ret[row], its return G, or with ret == nullptr the sampled slot's stored reward.
__global__ void iql_gather_kernel(int E, int A, int SMAX, int B, long long cap, int size, const int *idx, const int *boot, const float *ret,
                                  const float *r_obs, const float *r_next, const int *r_act, const float *r_rew, const uint8_t *r_done,
                                  float *S, float *S1, int *act, float *rew, uint8_t *done) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int q4 = SMAX >> 2;
    const long long R = (long long)E * B, tot = (long long)A * R * q4;
    if (i < tot) {
        const int c = (int)(i % q4);
        const long long row = (i / q4) % R, a = i / ((long long)q4 * R);
        const long long e = row / B, at = (e * A + a) * B + row % B;
        const int s = iql_ring_slot(idx[at], size), j = iql_ring_slot(boot[at], size);
        reinterpret_cast<float4 *>(S)[i] = *reinterpret_cast<const float4 *>(r_obs + ((e * cap + s) * A + a) * SMAX + 4 * c);
        reinterpret_cast<float4 *>(S1)[i] = *reinterpret_cast<const float4 *>(r_next + ((e * cap + j) * A + a) * SMAX + 4 * c);
    }
    if (i < (long long)A * R) {
        const long long row = i % R, a = i / R, e = row / B, at = (e * A + a) * B + row % B;
        const int s = iql_ring_slot(idx[at], size), j = iql_ring_slot(boot[at], size);
        act[i] = r_act[(e * cap + s) * A + a];
        rew[i] = ret ? ret[i] : r_rew[(e * cap + s) * A + a];
        done[i] = r_done[e * cap + j];
    }
}

// q1 = max_k Q(s')[k] over the agent's actions (agents/policies.py:315-316)
__global__ void iql_qmax_kernel(const float *Q, const int *n_act, long long R, int A, float *q1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * R) return;
    const int na = n_act[i / R];
    const float *q = Q + i * kQ;
    float m = q[0];
    for (int k = 1; k < na; ++k) m = fmaxf(m, q[k]);
    q1[i] = m;
}

// Double DQN (tsc_iql_set_target, double_q): a* = first maximum of the ONLINE net's Q(s') (np.argmax), q1 = the TARGET net's Q(s')[a*]
__global__ void iql_qsel_kernel(const float *Qon, const float *Qtg, const int *n_act, long long R, int A, float *q1, int *astar) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * R) return;
    const int na = n_act[i / R];
    const float *q = Qon + i * kQ;
    int best = 0;
    for (int k = 1; k < na; ++k) if (q[k] > q[best]) best = k;
    q1[i] = Qtg[i * kQ + best];
    astar[i] = best;
}

// The TD kernels' per-agent loss sum, stats[a][0] += l of row i -- logging only (policies.py:330-337): rows of one agent are contiguous, a
// wave may straddle two agents -> per-lane atomics are avoided by reducing only when the whole wave belongs to one agent
__device__ __forceinline__ void td_loss_sum(float l, int a, long long i, long long R, int A, double *stats) {
    const int a0 = __shfl(a, 0, 64);
    const bool uni = __all(a == a0 || i >= (long long)A * R);
    if (uni) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) l += __shfl_down(l, o, 64);
        if ((threadIdx.x & 63) == 0 && l != 0.f) atomicAdd(&stats[a0 * 2], (double)l);
    } else if (l != 0.f) {
        atomicAdd(&stats[a * 2], (double)l);
    }
}

// tq = done ? r : r + gamma q1 ; loss = mean((q0 - tq)^2) ; dQ[k] = 2 (q0 - tq) / R at k = a   (agents/policies.py:317-318)
// The options of a route, each a pointer that is nullptr when the option is off (uniform over the grid, so no wave diverges on them):
struct TdOpts {
    const float *w;         // prioritized replay: the row's importance weight -- loss = mean(w (q0 - tq)^2), dQ[k] = 2 w (q0 - tq) / R; else 1
    const float *disc;      // multi-step returns: the row's own discount gamma^k (rew is then its return G); else the scalar gamma
    float *td;              // |delta| out; else no store
    const int *n_act;       // dueling head, Q the combined values: the DENSE dQ row the head's backward needs -- g (delta_ja - 1 / n_a) for
                            // j < n_a, g at the value column 7, 0 between; else the sparse row.  (Dueling is always weighted: w = 1 on every
                            // row when prioritized replay is off.)
};
__global__ void iql_td_kernel(const float *Q, const float *q1, const int *act, const float *rew, const uint8_t *done, TdOpts o, long long R,
                              int A, float gamma, float *dQ, double *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float l = 0.f;
    int a = 0;
    if (i < (long long)A * R) {
        a = (int)(i / R);
        const float r = rew[i];
        const float tq = done[i] ? r : r + (o.disc ? o.disc[i] : gamma) * q1[i];
        const int k0 = act[i];
        const float d = Q[i * kQ + k0] - tq;
        float g;
        if (o.w) {
            const float wi = o.w[i];
            g = 2.0f * d * wi / (float)R;
            l = d * d * wi / (float)R;
        } else {
            g = 2.0f * d / (float)R;
            l = d * d / (float)R;
        }
        float row[kQ];
        if (o.n_act) {
            const int na = o.n_act[a];
            const float inv_na = 1.f / (float)na;
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                const float off = k < na ? -inv_na : k == kQ - 1 ? 1.f : 0.f;
                row[k] = g * (k == k0 ? 1.f + off : off);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kQ; ++k) row[k] = k == k0 ? g : 0.f;
        }
        reinterpret_cast<float4 *>(dQ + i * kQ)[0] = make_float4(row[0], row[1], row[2], row[3]);
        reinterpret_cast<float4 *>(dQ + i * kQ)[1] = make_float4(row[4], row[5], row[6], row[7]);
        if (o.td) o.td[i] = fabsf(d);
    }
    td_loss_sum(l, a, i, R, A, stats);
}

// ---- dueling head (tsc_iql_set_dueling; Wang et al. 2016), grouped-GEMM path ----------------------------------------------------
// The head's eight outputs of a row, out = X2 Wq + bq as q_forward leaves them, in place:  Q[j] = V + A_j - (1 / n_a) sum_{k < n_a} A_k for
// j < n_a with A = out[0 .. n_a) and V = out[7]; columns >= n_a stay (every reader masks them with k < n_a).  Q [A][rows][8].
__global__ void iql_duel_combine_kernel(float *Q, const int *n_act, long long rows, int A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * rows) return;
    const int na = n_act[i / rows];
    float *q = Q + i * kQ;
    float s = 0.f;
    for (int k = 0; k < na; ++k) s += q[k];
    const float base = q[kQ - 1] - s * (1.f / (float)na);
    for (int k = 0; k < na; ++k) q[k] = base + q[k];
}

__global__ void iql_fill_kernel(float *x, long long n, float v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

// ---- multi-step returns (tsc_iql_set_return_steps; Sutton 1988, the n-step component of Rainbow) ---------------------------------
// The window of every sampled row, walked over the ring at sample time (INTEGRATION.md "Multi-step returns"): from the sampled slot s,
//   j = s; G = 0; c = 1; k = 0;  repeat { G += c r[e][j][a]; c *= gamma; ++k; stop at done[e][j], j == w or k == n; j = (j + 1) mod cap }
// with w the newest slot of the rings.  G and c are float64 (the build forbids contraction: one rounding per product and per sum, the
// oracle's), rounded to float32 once per row.  ns_slot [E][A][B] (idx layout) = j, ns_ret | ns_disc | ns_k [A][R] = G | gamma^k | k.
// One thread per row in idx order: the draw and ns_slot move as whole cache lines, the three [A][R] rows in runs of B.  The k <= n reward
// reads of a row are 4-byte gathers at stride A inside the cap x A floats of its instance's ring, and the done bytes lie inside the ring's
// cap bytes -- the B rows of a ring and the A rings of an instance, neighbours in this order, meet in the same lines of L2.  s is
// clamped like the gather's, so j stays inside [0, size): j only moves forward to w, and w = size - 1 while the ring is unfilled.
__global__ void iql_nstep_kernel(int E, int A, int B, long long cap, int size, int w, int n, double gamma, const int *__restrict__ idx,
                                 const float *__restrict__ r_rew, const uint8_t *__restrict__ r_done, int *__restrict__ ns_slot,
                                 float *__restrict__ ns_ret, float *__restrict__ ns_disc, int *__restrict__ ns_k) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)E * A * B) return;
    const int b = (int)(t % B);
    const long long p = t / B, e = p / A, a = p % A;
    const float *rew = r_rew + e * cap * A + a;
    const uint8_t *dn = r_done + e * cap;
    int j = iql_ring_slot(idx[t], size), k = 0;
    double G = 0.0, c = 1.0;
    for (;;) {
        G += c * (double)rew[(long long)j * A];
        c *= gamma;
        ++k;
        if (dn[j] || j == w || k >= n) break;
        j = j + 1 == (int)cap ? 0 : j + 1;
    }
    const long long row = a * ((long long)E * B) + e * B + b;
    ns_slot[t] = j;
    ns_ret[row] = (float)G;
    ns_disc[row] = (float)c;
    ns_k[row] = k;
}

// ---- prioritized replay (tsc_iql_set_per; proportional, Schaul et al. 2016) -----------------------------------------------------
// Stored priorities prio [E][A][cap] (already (|delta| + eps)^alpha, contiguous per ring: the sampler reads one whole ring at a time)
// and the rings' running maxima qmax [E][A].

// inclusive prefix sum of one double per lane over the wavefront, on the DPP data path (the simulator's scan, csrc/tsc_env.hip:
// row_shr within the four 16-lane rows, then row_bcast:15 / :31); a lane without a source lane adds the identity's bits, 0.0
template <int ctrl, int rows>
__device__ __forceinline__ double per_dpp_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, ctrl, rows, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), ctrl, rows, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double per_wave_scan_add(double v) {
    v += per_dpp_f64<0x111, 0xF>(v); v += per_dpp_f64<0x112, 0xF>(v); v += per_dpp_f64<0x114, 0xF>(v); v += per_dpp_f64<0x118, 0xF>(v);
    v += per_dpp_f64<0x142, 0xA>(v); v += per_dpp_f64<0x143, 0xC>(v);
    return v;
}
__device__ __forceinline__ double per_shfl_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)(unsigned)(unsigned long long)b, lane, 64), hi = __shfl((int)((unsigned long long)b >> 32), lane, 64);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

constexpr int kPerWaves = 4;       // rings per workgroup of the sampler: one wavefront each
// LDS image of one ring: lane l owns the contiguous slots [l K, (l + 1) K), K = ceil(size / 64), at row stride K | 1 (odd: the 64 lanes'
// walks over their own blocks fall on distinct banks)
__host__ __device__ inline int per_block_len(int size) { return (size + 63) >> 6; }
__host__ __device__ inline int per_wave_floats(int cap) { return 64 * (per_block_len(cap) | 1); }

// The stratified proportional draw of one minibatch, one wavefront per ring p = e A + a:
//   C[k] = sum_{s <= k} q[s] over the filled slots (float64), total = C[size - 1];
//   pick i: t = (i + U(seed, upd, p B + i)) total / B; the smallest k with C[k] > t, clamped to the last slot with q > 0;
//   w_i = (size q[k] / total)^-beta (float64: product, quotient, pow), divided by the largest of the ring's B weights.
// The ring comes in with coalesced loads into LDS; every lane sums its block; the 64 block sums go through the wavefront scan; lane i < B
// finds the lane whose block holds its target (the number of lanes whose inclusive sum is <= t), then walks that block.
// given != 0: idx is the caller's draw (tsc_iql_compute_grads_at), clamped into the filled part like the gather's; only w is formed
// (a slot with q = 0, which no draw of ours can produce, takes the ring's largest weight).
__global__ void __launch_bounds__(64 * kPerWaves) iql_per_sample_kernel(int E, int A, int B, long long cap, int size, double beta,
                                                                        unsigned long long seed, unsigned long long upd, int given,
                                                                        const float *__restrict__ prio, int *__restrict__ idx,
                                                                        float *__restrict__ w) {
    extern __shared__ __attribute__((aligned(16))) float per_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * kPerWaves + wave;
    const bool live = p < (long long)E * A;
    const int K = per_block_len(size), Ks = K | 1;
    float *sm = per_smem + wave * per_wave_floats((int)cap);
    const float *ring = prio + (live ? p : 0) * cap;
    // slot g -> block g / K: g < 4096 and K <= 64 (TSC_IQL_PER_MAX_BUFFER), so with M = ceil(2^20 / K) the error M K - 2^20 < K gives
    // g (M K - 2^20) < 2^18 < 2^20 and (g M) >> 20 is the exact quotient, in 32 bits -- no integer division per slot
    const unsigned M = ((1u << 20) + (unsigned)K - 1) / (unsigned)K;
    if (live)
        for (int g0 = 0; g0 < size; g0 += 256) {      // four coalesced requests in flight per lane before the first LDS write
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int g = g0 + 64 * u + lane; v[u] = ring[g < size ? g : size - 1]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = g0 + 64 * u + lane, blk = (int)(((unsigned)g * M) >> 20);
                if (g < size) sm[blk * Ks + (g - blk * K)] = v[u];
            }
        }
    __syncthreads();
    const int lo = lane * K, cnt = size - lo < 0 ? 0 : size - lo < K ? size - lo : K;
    const float *mine = sm + lane * Ks;
    double bsum = 0.0;
    if (live)
        for (int s = 0; s < cnt; ++s) bsum += (double)mine[s];
    const double incl = per_wave_scan_add(bsum);
    const double total = per_shfl_f64(incl, 63);
    const unsigned long long pos = __ballot(bsum > 0.0);
    const int last_lane = pos ? 63 - __clzll((long long)pos) : 0;       // the last block with mass
    int k = 0;
    if (given) {
        if (live && lane < B) {
            k = iql_ring_slot(idx[p * B + lane], size);
        }
    } else {
        const double t = ((double)lane + uniform01(seed, upd, (unsigned long long)p * B + lane)) * total / (double)B;
        int j = 0;
        for (int l = 0; l < 64; ++l) j += per_shfl_f64(incl, l) <= t ? 1 : 0;
        if (j > last_lane) j = last_lane;           // t == total after rounding: the last slot with q > 0
        const int jlo = j * K, jcnt = size - jlo < K ? size - jlo : K;
        double c = per_shfl_f64(incl, j > 0 ? j - 1 : 0);           // C of the slot before the block: what the lane search compared with
        if (j == 0) c = 0.0;
        const float *blk = sm + j * Ks;
        int hit = -1, lastpos = 0;
        for (int s = 0; s < jcnt; ++s) {
            const float q = blk[s];
            c += (double)q;
            if (q > 0.f) lastpos = s;
            if (hit < 0 && q > 0.f && c > t) hit = s;
        }
        k = jlo + (hit < 0 ? lastpos : hit);
    }
    const bool on = live && lane < B;
    const int kb = (int)(((unsigned)k * M) >> 20);
    const float qk = sm[kb * Ks + (k - kb * K)];
    double wi = 0.0;
    if (on && qk > 0.f) wi = pow((double)size * (double)qk / total, -beta);
    double wmax = wi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, per_shfl_f64(wmax, lane ^ o));
    if (on) {
        const long long e = p / A, a = p % A;
        if (!given) idx[p * B + lane] = k;
        w[a * ((long long)E * B) + e * B + lane] = (wi > 0.0 && wmax > 0.0) ? (float)(wi / wmax) : 1.0f;
    }
}

// priority write-back: q[k] = (float)pow(|delta| + eps, alpha) of every sampled row, qmax rises to the largest.  One thread per ring walks
// its B picks in order, so a slot drawn twice has no write race: the later pick's value stays.
__global__ void iql_per_update_kernel(int E, int A, int B, long long cap, int size, double alpha, double eps, const int *__restrict__ idx,
                                      const float *__restrict__ td, float *__restrict__ prio, float *__restrict__ qmax) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)E * A) return;
    const long long e = p / A, a = p % A;
    const float *d = td + a * ((long long)E * B) + e * B;
    float m = qmax[p];
    for (int i = 0; i < B; ++i) {
        const int k = iql_ring_slot(idx[p * B + i], size);
        const float v = (float)pow((double)d[i] + eps, alpha);
        prio[p * cap + k] = v;
        m = fmaxf(m, v);
    }
    qmax[p] = m;
}

// a new transition enters every ring at its running maximum (also where it overwrites an old one)
__global__ void iql_per_add_kernel(long long rings, long long cap, long long slot, const float *__restrict__ qmax, float *__restrict__ prio) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < rings) prio[p * cap + slot] = qmax[p];
}

// arming: q = 1 on the filled slots, 0 behind them; qmax = 1
__global__ void iql_per_init_kernel(long long rings, long long cap, long long size, float *__restrict__ prio, float *__restrict__ qmax) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rings * cap) prio[i] = i % cap < size ? 1.0f : 0.0f;
    if (i < rings) qmax[i] = 1.0f;
}

__global__ void iql_transpose_kernel(const float *params, QLayout L, float *W2T, float *WqT) {
    // W2T[a][n][k] = W2[a][k][n]  (H2 x H1) ; WqT[a][n][k] = Wq[a][k][n]  (8 x H2)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p2 = (long long)L.H1 * L.H2, pq = (long long)L.H2 * kQ;
    if (i < p2 * L.A) {
        const long long a = i / p2, r = i % p2;
        const int n = (int)(r / L.H1), k = (int)(r % L.H1);
        W2T[i] = params[a * L.stride + L.oW2 + (long long)k * L.H2 + n];
    }
    if (i < pq * L.A) {
        const long long a = i / pq, r = i % pq;
        const int n = (int)(r / L.H2), k = (int)(r % L.H2);
        WqT[i] = params[a * L.stride + L.oWq + (long long)k * kQ + n];
    }
}

constexpr int kNormSlices = 8;     // an agent's squared norm is summed in 8 slices (one workgroup each), folded in slice order by the readers
__global__ void iql_norm_kernel(const float *grad, long long per_agent, double gscale, double *norm2) {
    __shared__ double red[256];
    const int a = blockIdx.x / kNormSlices, sl = blockIdx.x % kNormSlices;
    const float *gp = grad + (long long)a * per_agent;
    const long long lo = per_agent * sl / kNormSlices, hi = per_agent * (sl + 1) / kNormSlices;
    double s = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) { const double v = (double)gp[i] * gscale; s += v * v; }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) norm2[blockIdx.x] = red[0];
}
__device__ __forceinline__ double iql_norm2_of(const double *norm2, long long a) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kNormSlices; ++k) s += norm2[a * kNormSlices + k];
    return s;
}

// tf.train.AdamOptimizer (TF 1.12 defaults beta1 .9, beta2 .999, epsilon 1e-8):
//   lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= lr_t m / (sqrt(v) + eps)
__global__ void iql_adam_kernel(float *w, float *m1, float *m2, const float *grad, long long per_agent, long long total,
                                const double *norm2, float gscale, float clip, float lr_t) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float nrm = (float)sqrt(iql_norm2_of(norm2, i / per_agent));
    float g = grad[i] * gscale;
    if (clip > 0.f) g = g * (clip / fmaxf(nrm, clip));
    const float m = 0.9f * m1[i] + (1.0f - 0.9f) * g;
    const float v = 0.999f * m2[i] + (1.0f - 0.999f) * g * g;
    m1[i] = m; m2[i] = v;
    w[i] = w[i] - lr_t * m / (sqrtf(v) + 1e-8f);
}

}  // namespace

#include "tsc_iql_fused.h"

namespace {

// The fused path's launch plan (the role of Plan in tsc_model.hip): which instantiation serves each role and the dynamic LDS it is
// launched with, filled once at create and only read afterwards.  make<NM1>() is the only place that spells an instantiation: a new
// variant is a member here, a set() line there, and a branch of the route in iql_compute_grads.  set() is the only way a member gets
// its kernel, and it lists the kernel in entries[] as it does so: create's LDS opt-in walks that list, so it cannot miss one.
template <class... Args>
struct QKernel {
    void (*fn)(QFusedArgs, Args...) = nullptr;
    int lds = 0;                  // dynamic LDS bytes
    void launch(unsigned grid, hipStream_t st, const QFusedArgs &fa, Args... args) const {
        hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, st, fa, args...);
    }
};
struct QPlan {
    QKernel<const float *, int, double, unsigned long long, unsigned long long, int, float *, float *, int *> act;
    QKernel<> grad;                                           // one launch: Q(s') from the parameters, inside the kernel
    QKernel<const float *> grad_y;                            // the rows' TD targets come from target[]
    QKernel<const float *, const float *, float *> grad_yw;   // ... and their importance weights; |delta| out
    QKernel<const float *, float *, int *> target[2];         // [0] max, [1] Double DQN (two weight images)
    // the dueling head's (tsc_iql_set_dueling): always the two-launch route, the gradient always with weights (1 without prioritized replay)
    QKernel<const float *, int, double, unsigned long long, unsigned long long, int, float *, float *, int *, QDuel> act_duel;
    QKernel<const float *, const float *, float *, QDuel> grad_duel;
    QKernel<const float *, float *, int *, QDuel> target_duel[2];
    // multi-step returns (tsc_iql_set_return_steps): the target kernels with the rows' return and discount; launched with idx = the bootstrap slots
    QKernel<const float *, float *, int *, QNStep> target_n[2];
    QKernel<const float *, float *, int *, QDuel, QNStep> target_duel_n[2];
    int S = 0, cps = 0;           // row splits per agent (workgroups = A S); 64-row chunks per split
    struct Entry { const void *fn; int lds; } entries[16] = {};    // (fourteen in use)
    int n_entries = 0;

    template <class... Args> void set(QKernel<Args...> &k, void (*fn)(QFusedArgs, Args...), int lds) {
        k.fn = fn; k.lds = lds;
        assert(n_entries < 16);
        entries[n_entries++] = {(const void *)fn, lds};
    }
    template <int NM1> static QPlan make() {
        constexpr int fwd = QFusedLds<NM1>::fwd_floats * 4, grd = QFusedLds<NM1>::grad_floats * 4;
        QPlan P;
        P.set(P.act, iql_fused_act_kernel<NM1, 8>, fwd);
        P.set(P.grad, iql_fused_grad_kernel<NM1, 8>, grd);
        P.set(P.grad_y, iql_fused_grad_kernel<NM1, 8, true, false, const float *>, grd);
        P.set(P.grad_yw, iql_fused_grad_kernel<NM1, 8, true, true, const float *, const float *, float *>, grd);
        P.set(P.target[0], iql_fused_target_kernel<NM1, 8, false>, fwd);
        P.set(P.target[1], iql_fused_target_kernel<NM1, 8, true>, 2 * fwd);
        P.set(P.act_duel, iql_fused_act_kernel<NM1, 8, QDuel>, fwd);
        P.set(P.grad_duel, iql_fused_grad_kernel<NM1, 8, true, true, const float *, const float *, float *, QDuel>, QFusedLds<NM1>::duel_floats * 4);
        P.set(P.target_duel[0], iql_fused_target_kernel<NM1, 8, false, QDuel>, fwd);
        P.set(P.target_duel[1], iql_fused_target_kernel<NM1, 8, true, QDuel>, 2 * fwd);
        P.set(P.target_n[0], iql_fused_target_kernel<NM1, 8, false, QNStep>, fwd);
        P.set(P.target_n[1], iql_fused_target_kernel<NM1, 8, true, QNStep>, 2 * fwd);
        P.set(P.target_duel_n[0], iql_fused_target_kernel<NM1, 8, false, QDuel, QNStep>, fwd);
        P.set(P.target_duel_n[1], iql_fused_target_kernel<NM1, 8, true, QDuel, QNStep>, 2 * fwd);
        return P;
    }
};

}  // namespace

struct tsc_iql {
    QLayout lay{};
    int E = 0, B = 0, device = 0;
    long long cap = 0, cum = 0;   // ring capacity / transitions added so far (per instance)
    double gamma = 0, rnorm = 0, rclip = 0, max_norm = 0;
    long long adam_t = 0;
    hipStream_t stream = nullptr;
    tsc::DeviceBufs bufs;           // every device buffer of the handle (a pointer below stays null until its path allocates it)
    int *n_act = nullptr;
    int16_t *rowrange = nullptr;  // [A][SMAX][2]
    float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr, *W2T = nullptr, *WqT = nullptr;
    float *r_obs = nullptr, *r_next = nullptr, *r_rew = nullptr; int *r_act = nullptr; uint8_t *r_done = nullptr;
    int *idx = nullptr;
    float *S = nullptr, *S1 = nullptr, *rew = nullptr, *q1 = nullptr; int *act = nullptr; uint8_t *done = nullptr;
    float *X1 = nullptr, *X2 = nullptr, *Q = nullptr, *dQ = nullptr, *dX2 = nullptr;
    float *Qe = nullptr;          // [A][E][8] q rows of the acting forward
    float *X1e = nullptr, *X2e = nullptr;
    double *norm2 = nullptr, *stats = nullptr;
    float *ws = nullptr, *wsc = nullptr; size_t ws_floats = 0, wsc_floats = 0;
    long long nparam = 0;
    // fused DeepQPolicy learner (tsc_iql_fused.h): 0 = grouped-GEMM path, 8 / 10 = first-layer column tiles of the plan's instantiations
    int fused = 0;
    QPlan plan;
    int *n_wave = nullptr, *n_wait = nullptr;
    float *fws = nullptr, *fwsl = nullptr;
    long long *dbg = nullptr, *dbg_buf = nullptr;     // the stamp buffer the kernels see (null while tsc_iql_debug_clock is off) / its allocation
    // target network (tsc_iql_set_target): refresh period in Adam steps (0 = none: the reference's loss), Double DQN on top of it
    int tgt_period = 0, tgt_double = 0;
    float *tparams = nullptr, *y = nullptr, *Q2 = nullptr;      // the frozen copy [A][stride]; per-row TD targets [A][R] (fused path); the online net's Q(s') (grouped path, double_q)
    int *astar = nullptr;         // [A][R] Double DQN's picks
    bool y_valid = false;         // a compute_grads ran on the armed handle
    // prioritized replay (tsc_iql_set_per): stored priorities [E][A][cap], running maxima [E][A], importance weights and |delta| [A][R]
    int per = 0;
    double per_alpha = 0, per_eps = 0, per_beta = 1.0;
    float *prio = nullptr, *qmax = nullptr, *w = nullptr, *td = nullptr;
    bool per_valid = false;       // a compute_grads ran on the handle while prioritized replay was armed
    // dueling head (tsc_iql_set_dueling): column 7 of Wq | bq is the value stream; the weights of a step without prioritized replay [A][R], all 1
    int duel = 0;
    float *w_one = nullptr;
    // multi-step returns (tsc_iql_set_return_steps): the horizon n (1 = the reference's one-step target) and iql_nstep_kernel's outputs --
    // bootstrap slots [E][A][B] (idx layout), returns G, discounts gamma^k and horizons k [A][R]
    int nstep = 1;
    int *ns_slot = nullptr, *ns_k = nullptr;
    float *ns_ret = nullptr, *ns_disc = nullptr;
    bool ns_valid = false;        // a compute_grads ran on the handle while return_steps > 1
    std::vector<int> n_act_host;
    // parameter sharing (tsc_iql_set_sharing)
    std::vector<int32_t> dims;          // [A][3] n_wave, n_wait, n_act as given to create
    std::vector<int32_t> share_class;   // [A] the caller's class ids; empty: disarmed
    std::vector<std::vector<int>> share_lists;  // classes with >= 2 members, ascending agent indices
    int *share_members = nullptr, *share_off = nullptr;     // device: the lists back to back, [n_lists + 1] offsets into them
    double *share_invk = nullptr;       // device: [n_lists] 1 / members
};

namespace {

int qgemm(tsc_iql *h, bool tn, int epi, int M, int N, int K, const float *A, long long sA, int lda, const float *B, long long sB,
          int ldb, float *C, long long sC, int ldc, const float *bias, long long sBias, const float *aux, long long sAux,
          int ldaux, const int16_t *rr, long long sRR, float *colsum, long long sColsum) {
    GemmArgs a;
    a.A = A; a.B = B; a.C = C; a.bias = bias; a.aux = aux; a.rr = rr; a.colsum = colsum;
    a.sA = sA; a.sB = sB; a.sC = sC; a.sBias = sBias; a.sAux = sAux; a.sRR = sRR; a.sColsum = sColsum;
    a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldaux = ldaux; a.M = M; a.N = N; a.K = K; a.gdivA = 1;
    tsc::plan_splitk(a, h->lay.A, tn ? h->ws : nullptr, h->wsc, h->ws_floats, h->wsc_floats);
    tsc::launch_gemm_dyn(tn, epi, a, h->lay.A, h->stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// Q(S) for `rows` rows per agent: S [A][rows][SMAX] -> X1, X2 (DQN) -> Q [A][rows][8]
int q_forward(tsc_iql *h, const float *P, const float *S, long long sS, int ldS, long long rows, float *X1, float *X2, float *Q) {
    const QLayout &L = h->lay;
    if (!L.dqn)
        return qgemm(h, false, tsc::EPI_BIAS, (int)rows, kQ, L.SMAX, S, sS, ldS, P + L.oWq, L.stride, kQ, Q, rows * kQ, kQ,
                     P + L.obq, L.stride, nullptr, 0, 0, nullptr, 0, nullptr, 0);
    if (qgemm(h, false, tsc::EPI_BIAS_RELU, (int)rows, L.H1, L.SMAX, S, sS, ldS, P + L.oW1, L.stride, L.H1, X1, rows * L.H1, L.H1,
              P + L.ob1, L.stride, nullptr, 0, 0, nullptr, 0, nullptr, 0)) return 1;
    if (qgemm(h, false, tsc::EPI_BIAS_RELU, (int)rows, L.H2, L.H1, X1, rows * L.H1, L.H1, P + L.oW2, L.stride, L.H2, X2, rows * L.H2,
              L.H2, P + L.ob2, L.stride, nullptr, 0, 0, nullptr, 0, nullptr, 0)) return 1;
    return qgemm(h, false, tsc::EPI_BIAS, (int)rows, kQ, L.H2, X2, rows * L.H2, L.H2, P + L.oWq, L.stride, kQ, Q, rows * kQ, kQ,
                 P + L.obq, L.stride, nullptr, 0, 0, nullptr, 0, nullptr, 0);
}

QFusedArgs fused_args(const tsc_iql *h, long long size) {
    const QLayout &L = h->lay;
    QFusedArgs fa;
    fa.params = h->params; fa.n_act = h->n_act; fa.n_wave = h->n_wave; fa.n_wait = h->n_wait; fa.idx = h->idx;
    fa.r_obs = h->r_obs; fa.r_next = h->r_next; fa.r_rew = h->r_rew; fa.r_act = h->r_act; fa.r_done = h->r_done;
    fa.E = h->E; fa.A = L.A; fa.B = h->B; fa.SMAX = L.SMAX; fa.size = (int)size; fa.cap = h->cap; fa.R = (long long)h->E * h->B;
    fa.gamma = (float)h->gamma; fa.S = h->plan.S; fa.cps = h->plan.cps; fa.ws = h->fws; fa.wsl = h->fwsl;
    fa.dbg = h->dbg;
    fa.stride = L.stride; fa.oW1 = L.oW1; fa.ob1 = L.ob1; fa.oW2 = L.oW2; fa.ob2 = L.ob2; fa.oWq = L.oWq; fa.obq = L.obq;
    return fa;
}

// transitions in the filled part of every ring
long long replay_size(const tsc_iql *h) { return h->cum < h->cap ? h->cum : h->cap; }

// theta- <- theta on the handle's stream
hipError_t freeze_params(tsc_iql *h) {
    return hipMemcpyAsync(h->tparams, h->params, sizeof(float) * h->nparam, hipMemcpyDeviceToDevice, h->stream);
}

// a buffer its first user allocates (a failed allocation leaves the pointer null, and the next call asks again)
template <class T> hipError_t alloc_once(tsc_iql *h, T **field, long long count, bool zero = true) {
    return *field ? hipSuccess : h->bufs.alloc(field, count, zero);
}

// dueling handles: the head's outputs Q [A][rows][8] -> combined values, in place, behind the q_forward that wrote them
void duel_combine(tsc_iql *h, float *Q, long long rows) {
    const long long n = (long long)h->lay.A * rows;
    hipLaunchKernelGGL(iql_duel_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, Q, h->n_act, rows, h->lay.A);
}

size_t per_sample_lds(const tsc_iql *h) { return sizeof(float) * kPerWaves * per_wave_floats((int)h->cap); }

// Parameter sharing armed: a host buffer in the parameter layout must hold bit-identical slices for the members of a class.
// Returns 0, or 1 with the first differing pair named (what = the calling function and, where it takes several, the buffer).
int share_check_host(const tsc_iql *h, const float *p, const char *what) {
    const long long per_agent = h->lay.stride;
    for (const std::vector<int> &cls : h->share_lists)
        for (size_t j = 1; j < cls.size(); ++j) {
            const float *p0 = p + cls[0] * per_agent, *p1 = p + cls[j] * per_agent;
            if (memcmp(p0, p1, sizeof(float) * per_agent) == 0) continue;
            long long i = 0;
            while (memcmp(p0 + i, p1 + i, sizeof(float)) == 0) ++i;
            return tsc::fail("%s: parameter sharing is armed and agents %d and %d of one class differ (first at offset %lld of the agent's "
                             "slice: %.9g vs %.9g)", what, cls[0], cls[j], i, (double)p0[i], (double)p1[i]);
        }
    return 0;
}

// parameter sharing armed: every class member's gradient slice <- the class mean (share_reduce_kernel, tsc_share.h)
void launch_share_reduce(tsc_iql *h) {
    if (h->share_lists.empty()) return;
    const long long per_agent = h->lay.stride;
    hipLaunchKernelGGL(share_reduce_kernel, dim3((unsigned)((per_agent / 4 + 255) / 256), (unsigned)h->share_lists.size()), dim3(256), 0,
                       h->stream, h->grads, per_agent, h->share_members, h->share_off, h->share_invk);
}

}  // namespace

extern "C" {

int tsc_iql_create(const tsc_iql_cfg *cfg, int32_t n_env, int32_t device, tsc_iql **out) {
    if (!cfg || !out || n_env <= 0) return tsc::fail("tsc_iql_create: bad arguments");
    if (cfg->a_max > kQ) return tsc::fail("tsc_iql_create: a_max %d > %d", cfg->a_max, kQ);
    if (cfg->s_max % 4) return tsc::fail("tsc_iql_create: s_max must be a multiple of 4");
    if (cfg->kind != 0 && cfg->kind != 1) return tsc::fail("tsc_iql_create: kind must be 0 (lr) or 1 (dqn)");
    if (cfg->batch_size <= 0 || cfg->batch_size > 64 || cfg->buffer_size < cfg->batch_size)
        return tsc::fail("tsc_iql_create: need 0 < batch_size <= 64 <= buffer_size");
    TSC_HIP(hipSetDevice(device));
    tsc_iql *h = new tsc_iql();
    tsc::CreateGuard<tsc_iql, tsc_iql_destroy> guard(h);        // an error return below frees the handle and its buffers
    h->device = device; h->E = n_env; h->B = cfg->batch_size; h->cap = cfg->buffer_size;
    h->gamma = cfg->gamma; h->rnorm = cfg->reward_norm; h->rclip = cfg->reward_clip; h->max_norm = cfg->max_grad_norm;
    QLayout &L = h->lay;
    L.A = cfg->n_agent; L.SMAX = cfg->s_max; L.AMAX = cfg->a_max; L.dqn = cfg->kind;
    bool any_wait = false;
    for (int a = 0; a < L.A; ++a) any_wait |= cfg->n_wait[a] > 0;
    const int ft = any_wait ? cfg->n_fc0 / 4 : 0;            // q_fct width: n_fc0 / 4 (agents/policies.py:359)
    L.H1 = L.dqn ? cfg->n_fc0 + ft : 0; L.H2 = L.dqn ? cfg->n_h : 0;
    if (L.dqn && (L.H1 % 4 || L.H2 % 4)) return tsc::fail("tsc_iql_create: hidden widths must be multiples of 4");
    if (L.dqn) {
        L.oW1 = 0; L.ob1 = (long long)L.SMAX * L.H1; L.oW2 = L.ob1 + L.H1; L.ob2 = L.oW2 + (long long)L.H1 * L.H2;
        L.oWq = L.ob2 + L.H2; L.obq = L.oWq + (long long)L.H2 * kQ;
    } else {
        L.oW1 = L.ob1 = L.oW2 = L.ob2 = 0; L.oWq = 0; L.obq = (long long)L.SMAX * kQ;
    }
    L.stride = L.obq + kQ;
    h->nparam = L.stride * L.A;
    std::vector<int16_t> rr((size_t)L.A * L.SMAX * 2, 0);
    for (int a = 0; a < L.A; ++a) {
        const int nw = cfg->n_wave[a], nt = cfg->n_wait[a];
        if (nw + nt > L.SMAX) return tsc::fail("tsc_iql_create: agent %d obs wider than s_max", a);
        for (int j = 0; j < L.SMAX; ++j) {
            int lo = 0, hi = 0;
            if (j < nw) { lo = 0; hi = cfg->n_fc0; }
            else if (j < nw + nt) { lo = cfg->n_fc0; hi = cfg->n_fc0 + ft; }
            rr[((size_t)a * L.SMAX + j) * 2] = (int16_t)lo; rr[((size_t)a * L.SMAX + j) * 2 + 1] = (int16_t)hi;
        }
    }
    TSC_HIP(h->bufs.upload(&h->rowrange, rr.data(), rr.size()));
    TSC_HIP(h->bufs.upload(&h->n_act, cfg->n_act, L.A));
    h->n_act_host.assign(cfg->n_act, cfg->n_act + L.A);
    h->dims.resize((size_t)L.A * 3);
    for (int a = 0; a < L.A; ++a) {
        h->dims[(size_t)a * 3] = cfg->n_wave[a]; h->dims[(size_t)a * 3 + 1] = cfg->n_wait[a]; h->dims[(size_t)a * 3 + 2] = cfg->n_act[a];
    }
    const long long E = n_env, A = L.A, R = E * h->B, per = A * L.SMAX;
    TSC_HIP(h->bufs.alloc(&h->params, h->nparam, true)); TSC_HIP(h->bufs.alloc(&h->grads, h->nparam, true));
    TSC_HIP(h->bufs.alloc(&h->m1, h->nparam, true)); TSC_HIP(h->bufs.alloc(&h->m2, h->nparam, true));
    TSC_HIP(h->bufs.alloc(&h->r_obs, E * h->cap * per, true)); TSC_HIP(h->bufs.alloc(&h->r_next, E * h->cap * per, true));
    TSC_HIP(h->bufs.alloc(&h->r_rew, E * h->cap * A, true)); TSC_HIP(h->bufs.alloc(&h->r_act, E * h->cap * A, true)); TSC_HIP(h->bufs.alloc(&h->r_done, E * h->cap, true));
    TSC_HIP(h->bufs.alloc(&h->idx, E * A * h->B, true));
    TSC_HIP(h->bufs.alloc(&h->Qe, A * E * kQ, true));
    TSC_HIP(h->bufs.alloc(&h->norm2, A * kNormSlices, true)); TSC_HIP(h->bufs.alloc(&h->stats, A * 2, true));
    // The fused DeepQPolicy learner (tsc_iql_fused.h) is built for the reference's widths (config/config_iqld_*.ini: num_fc 128,
    // num_h 64 -> H1 = 160 with wait inputs, 128 without) and observations of at most 48 features; anything else, IQL-LR, and
    // TSC_IQL_FUSED=0 (the A/B switch of tests/test_iql_gpu.py) take the grouped-GEMM path.
    TSC_HIP(h->bufs.upload(&h->n_wave, cfg->n_wave, L.A));
    TSC_HIP(h->bufs.upload(&h->n_wait, cfg->n_wait, L.A));
    {
        const char *sw = getenv("TSC_IQL_FUSED");
        const bool want = !(sw && sw[0] == '0');
        int max_wave = 0, max_wait = 0;
        for (int a = 0; a < L.A; ++a) {
            max_wave = cfg->n_wave[a] > max_wave ? cfg->n_wave[a] : max_wave;
            max_wait = cfg->n_wait[a] > max_wait ? cfg->n_wait[a] : max_wait;
        }
        // with a wait part the kernel keeps two 16-feature groups of W1 per column tile in registers (tsc_iql_fused.h QW1)
        const bool fits = L.H1 == 128 || (L.H1 == 160 && max_wave <= 32 && max_wait <= 16);
        if (want && L.dqn && cfg->n_fc0 == 128 && L.H2 == kFH2 && L.SMAX <= kFSF && fits) h->fused = L.H1 / 16;
    }
    if (h->fused && R >= ((long long)1 << 31) / 64) h->fused = 0;       // the fused kernel indexes rows and chunks in 32 bits
    if (h->fused) {
        switch (h->fused) {
            case 8: h->plan = QPlan::make<8>(); break;
            case 10: h->plan = QPlan::make<10>(); break;
            default: return tsc::fail("tsc_iql_create: no fused instantiation for %d first-layer column tiles", h->fused);
        }
        // row splits per agent: one workgroup per CU (the kernel holds its gradient tiles in registers over its whole slice)
        const long long nchunks = (R + 63) / 64;
        long long S = 256 / A;
        if (S < 1) S = 1;
        if (S > nchunks) S = nchunks;
        h->plan.cps = (int)((nchunks + S - 1) / S);
        h->plan.S = (int)((nchunks + h->plan.cps - 1) / h->plan.cps);
        TSC_HIP(h->bufs.alloc(&h->fws, (long long)h->plan.S * A * L.stride, true)); TSC_HIP(h->bufs.alloc(&h->fwsl, (long long)h->plan.S * A, true));
        for (int k = 0; k < h->plan.n_entries; ++k)
            TSC_HIP(hipFuncSetAttribute(h->plan.entries[k].fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->plan.entries[k].lds));
    } else {
        TSC_HIP(h->bufs.alloc(&h->S, A * R * L.SMAX, true)); TSC_HIP(h->bufs.alloc(&h->S1, A * R * L.SMAX, true));
        TSC_HIP(h->bufs.alloc(&h->rew, A * R, true)); TSC_HIP(h->bufs.alloc(&h->q1, A * R, true)); TSC_HIP(h->bufs.alloc(&h->act, A * R, true)); TSC_HIP(h->bufs.alloc(&h->done, A * R, true));
        TSC_HIP(h->bufs.alloc(&h->Q, A * R * kQ, true)); TSC_HIP(h->bufs.alloc(&h->dQ, A * R * kQ, true));
        if (L.dqn) {
            TSC_HIP(h->bufs.alloc(&h->X1, A * R * L.H1, true)); TSC_HIP(h->bufs.alloc(&h->X2, A * R * L.H2, true)); TSC_HIP(h->bufs.alloc(&h->dX2, A * R * L.H2, true));
            TSC_HIP(h->bufs.alloc(&h->X1e, A * E * L.H1, true)); TSC_HIP(h->bufs.alloc(&h->X2e, A * E * L.H2, true));
            TSC_HIP(h->bufs.alloc(&h->W2T, A * L.H1 * L.H2, true)); TSC_HIP(h->bufs.alloc(&h->WqT, A * L.H2 * kQ, true));
        }
        h->ws_floats = (size_t)16 << 20; h->wsc_floats = (size_t)1 << 18;
        TSC_HIP(h->bufs.alloc(&h->ws, h->ws_floats, true)); TSC_HIP(h->bufs.alloc(&h->wsc, h->wsc_floats, true));
    }
    *out = guard.release();
    return 0;
}

int tsc_iql_destroy(tsc_iql *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;                                    // (h->bufs frees the device buffers)
    return 0;
}

int tsc_iql_set_stream(tsc_iql *h, void *s) {
    if (!h) return tsc::fail("null handle");
    h->stream = (hipStream_t)s;
    return 0;
}

int tsc_iql_layout(tsc_iql *h, int64_t out[12]) {
    if (!h || !out) return tsc::fail("tsc_iql_layout: bad arguments");
    const QLayout &L = h->lay;
    const int64_t v[12] = {L.A, L.stride, L.H1, L.H2, L.oW1, L.ob1, L.oW2, L.ob2, L.oWq, L.obq, kQ, L.dqn};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return 0;
}

int tsc_iql_set_params(tsc_iql *h, const float *p) {
    if (!h || !p) return tsc::fail("tsc_iql_set_params: bad arguments");
    if (share_check_host(h, p, "tsc_iql_set_params")) return 1;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(h->params, p, sizeof(float) * h->nparam, hipMemcpyHostToDevice));
    return 0;
}
int tsc_iql_get_params(tsc_iql *h, float *p) {
    if (!h || !p) return tsc::fail("tsc_iql_get_params: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(p, h->params, sizeof(float) * h->nparam, hipMemcpyDeviceToHost));
    return 0;
}
int tsc_iql_get_opt_state(tsc_iql *h, float *m, float *v, int64_t *t) {
    if (!h || !m || !v || !t) return tsc::fail("tsc_iql_get_opt_state: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(m, h->m1, sizeof(float) * h->nparam, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(v, h->m2, sizeof(float) * h->nparam, hipMemcpyDeviceToHost));
    *t = h->adam_t;
    return 0;
}
int tsc_iql_set_opt_state(tsc_iql *h, const float *m, const float *v, int64_t t) {
    if (!h || !m || !v || t < 0) return tsc::fail("tsc_iql_set_opt_state: bad arguments");
    if (share_check_host(h, m, "tsc_iql_set_opt_state (first moments)") || share_check_host(h, v, "tsc_iql_set_opt_state (second moments)")) return 1;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(h->m1, m, sizeof(float) * h->nparam, hipMemcpyHostToDevice));
    TSC_HIP(hipMemcpy(h->m2, v, sizeof(float) * h->nparam, hipMemcpyHostToDevice));
    h->adam_t = t;
    return 0;
}

int tsc_iql_forward(tsc_iql *h, const float *obs, float *q_out, int32_t *action, int32_t mode, double eps, uint64_t seed,
                    uint64_t step) {
    if (!h || !obs || !q_out || !action || mode < 0 || mode > 2) return tsc::fail("tsc_iql_forward: bad arguments");
    const QLayout &L = h->lay;
    if (h->fused) {
        QFusedArgs fa = fused_args(h, 0);
        tsc::ProfScope ps(tsc::KID_IQL_ACT, h->stream);
        const unsigned grid = (unsigned)(L.A * ((h->E + 63) / 64));
        if (h->duel)
            h->plan.act_duel.launch(grid, h->stream, fa, obs, (int)mode, eps, (unsigned long long)seed, (unsigned long long)step, L.AMAX, h->Qe,
                                    q_out, action, QDuel{});
        else
            h->plan.act.launch(grid, h->stream, fa, obs, (int)mode, eps, (unsigned long long)seed, (unsigned long long)step, L.AMAX, h->Qe,
                               q_out, action);
        TSC_HIP(hipGetLastError());
        return 0;
    }
    // obs [E][A][SMAX]: agent a's rows start at a * SMAX with row stride A * SMAX
    if (q_forward(h, h->params, obs, L.SMAX, L.A * L.SMAX, h->E, h->X1e, h->X2e, h->Qe)) return tsc::fail("tsc_iql_forward: gemm launch failed");
    if (h->duel) duel_combine(h, h->Qe, h->E);
    const int tot = h->E * L.A;
    hipLaunchKernelGGL(iql_act_kernel, dim3((tot + 255) / 256), dim3(256), 0, h->stream, h->Qe, h->n_act, h->E, L.A, L.AMAX,
                       (int)mode, eps, (unsigned long long)seed, (unsigned long long)step, q_out, action);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_iql_add_transition(tsc_iql *h, const float *obs, const int32_t *action, const double *reward, const float *next_obs,
                           const uint8_t *done) {
    if (!h || !obs || !action || !reward || !next_obs || !done) return tsc::fail("tsc_iql_add_transition: bad arguments");
    const QLayout &L = h->lay;
    const long long n = (long long)h->E * L.A * L.SMAX;
    tsc::ProfScope ps(tsc::KID_IQL_ADD, h->stream);
    hipLaunchKernelGGL(iql_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->E, L.A, L.SMAX, h->cap,
                       h->cum % h->cap, obs, action, reward, next_obs, done, h->rnorm, h->rclip, h->r_obs, h->r_next, h->r_act,
                       h->r_rew, h->r_done);
    TSC_HIP(hipGetLastError());
    ps.stop();
    if (h->per) {       // the new transition enters every ring at the ring's running maximum
        tsc::ProfScope pp(tsc::KID_IQL_PER_ADD, h->stream);
        const long long rings = (long long)h->E * L.A;
        hipLaunchKernelGGL(iql_per_add_kernel, dim3((unsigned)((rings + 255) / 256)), dim3(256), 0, h->stream, rings, h->cap, h->cum % h->cap,
                           h->qmax, h->prio);
        TSC_HIP(hipGetLastError());
    }
    h->cum += 1;
    return 0;
}

int tsc_iql_replay_size(tsc_iql *h, int64_t *size, int64_t *cum) {
    if (!h || !size || !cum) return tsc::fail("tsc_iql_replay_size: bad arguments");
    *size = replay_size(h); *cum = h->cum;
    return 0;
}

static int iql_compute_grads(tsc_iql *h, uint64_t seed, uint64_t update_index, const int32_t *idx_dev);

// prioritized replay: the priorities of the sampled slots follow the TD errors the gradient kernels left in td (nothing from the all-reduce)
static int iql_grads_then_priorities(tsc_iql *h, uint64_t seed, uint64_t update_index, const int32_t *idx_dev) {
    const int rc = iql_compute_grads(h, seed, update_index, idx_dev);
    if (rc || !h->per) return rc;
    const long long rings = (long long)h->E * h->lay.A, size = replay_size(h);
    tsc::ProfScope ps(tsc::KID_IQL_PER_UPDATE, h->stream);
    hipLaunchKernelGGL(iql_per_update_kernel, dim3((unsigned)((rings + 127) / 128)), dim3(128), 0, h->stream, h->E, h->lay.A, h->B, h->cap,
                       (int)size, h->per_alpha, h->per_eps, h->idx, h->td, h->prio, h->qmax);
    TSC_HIP(hipGetLastError());
    h->per_valid = true;
    return 0;
}

int tsc_iql_compute_grads(tsc_iql *h, uint64_t seed, uint64_t update_index) {
    return iql_grads_then_priorities(h, seed, update_index, nullptr);
}

int tsc_iql_compute_grads_at(tsc_iql *h, const int32_t *idx_dev) {
    if (!idx_dev) return tsc::fail("tsc_iql_compute_grads_at: null index buffer");
    return iql_grads_then_priorities(h, 0, 0, idx_dev);
}

static int iql_compute_grads(tsc_iql *h, uint64_t seed, uint64_t update_index, const int32_t *idx_dev) {
    if (!h) return tsc::fail("null handle");
    const QLayout &L = h->lay;
    const long long size = replay_size(h);
    if (size < h->B) return tsc::fail("tsc_iql_compute_grads: replay holds %lld < batch_size %d transitions", size, h->B);
    hipStream_t st = h->stream;
    const long long E = h->E, A = L.A, R = E * h->B;
    // the route of this call (arming can change between calls); both paths below read these names and nothing else
    const bool given = idx_dev != nullptr;                   // the draw: the caller's, else prioritized (per), else Floyd's
    const bool per = h->per != 0;                            // importance weights in, |delta| out
    const bool armed = h->tgt_period > 0;                    // Q(s') from the frozen copy
    const bool dbl = armed && h->tgt_double;                 // ... at the online net's first maximum
    const float *tp = armed ? h->tparams : h->params;        // the net behind the TD targets
    const bool duel = h->duel != 0;                          // dueling head: combined Q everywhere, dense dQ
    const bool nstep = h->nstep > 1;                         // multi-step returns: s', done, G and gamma^k of the row's window
    const bool two_launch = armed || per || duel || nstep;   // fused path: the TD targets in a launch of their own, else inside the gradient's
    TSC_HIP(hipMemsetAsync(h->stats, 0, sizeof(double) * A * 2, st));
    if (given) {        // (e.g. the reference's random.sample); the gather clamps every index into [0, size)
        TSC_HIP(hipMemcpyAsync(h->idx, idx_dev, sizeof(int) * E * A * h->B, hipMemcpyDeviceToDevice, st));
    }
    if (per) {          // the proportional draw and its importance weights; on the caller's draw only the weights
        tsc::ProfScope ps(tsc::KID_IQL_PER_SAMPLE, st);
        hipLaunchKernelGGL(iql_per_sample_kernel, dim3((unsigned)((E * A + kPerWaves - 1) / kPerWaves)), dim3(64 * kPerWaves),
                           per_sample_lds(h), st, (int)E, (int)A, h->B, h->cap, (int)size, h->per_beta,
                           (unsigned long long)seed, (unsigned long long)update_index, given ? 1 : 0, h->prio, h->idx, h->w);
        TSC_HIP(hipGetLastError());
    } else if (!given) {
        tsc::ProfScope ps(tsc::KID_IQL_SAMPLE, st);
        if (h->B == 20)
            hipLaunchKernelGGL(iql_sample_fixed_kernel<20>, dim3((unsigned)((E * A + 127) / 128)), dim3(128), 0, st, (int)E, (int)A, size,
                               (unsigned long long)seed, (unsigned long long)update_index, h->idx);
        else
            hipLaunchKernelGGL(iql_sample_kernel, dim3((unsigned)((E * A + 127) / 128)), dim3(128), 0, st, (int)E, (int)A, h->B, size,
                               (unsigned long long)seed, (unsigned long long)update_index, h->idx);
    }
    if (nstep) {        // the window of every sampled row, behind the draw: bootstrap slot, return, discount
        tsc::ProfScope ps(tsc::KID_IQL_NSTEP, st);
        const long long rows = E * A * h->B;
        hipLaunchKernelGGL(iql_nstep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (int)E, (int)A, h->B, h->cap, (int)size,
                           (int)((h->cum - 1) % h->cap), h->nstep, h->gamma, h->idx, h->r_rew, h->r_done, h->ns_slot, h->ns_ret, h->ns_disc,
                           h->ns_k);
        TSC_HIP(hipGetLastError());
        h->ns_valid = true;
    }
    if (armed || duel || nstep) h->y_valid = true;
    if (h->fused) {
        const QPlan &P = h->plan;
        const QFusedArgs fa = fused_args(h, size);
        const unsigned grid = (unsigned)(A * P.S);
        if (two_launch) {       // the TD targets from tp (forward only), then the gradient with one row set
            // (prioritized replay always takes this route; without a target network tp is the parameters themselves)
            {
                tsc::ProfScope ps(tsc::KID_IQL_TARGET, st);
                if (nstep) {    // s' and done at the bootstrap slot: the target kernel finds its slot through idx
                    QFusedArgs fn = fa;
                    fn.idx = h->ns_slot;
                    const QNStep ns{h->ns_ret, h->ns_disc};
                    if (duel) P.target_duel_n[dbl].launch(grid, st, fn, tp, h->y, h->astar, QDuel{}, ns);
                    else P.target_n[dbl].launch(grid, st, fn, tp, h->y, h->astar, ns);
                } else if (duel) P.target_duel[dbl].launch(grid, st, fa, tp, h->y, h->astar, QDuel{});
                else P.target[dbl].launch(grid, st, fa, tp, h->y, h->astar);
            }
            TSC_HIP(hipGetLastError());
            tsc::ProfScope ps(tsc::KID_IQL_GRAD, st);
            if (duel) P.grad_duel.launch(grid, st, fa, h->y, per ? h->w : h->w_one, h->td, QDuel{});
            else if (per) P.grad_yw.launch(grid, st, fa, h->y, h->w, h->td);
            else P.grad_y.launch(grid, st, fa, h->y);
        } else {
            tsc::ProfScope ps(tsc::KID_IQL_GRAD, st);
            P.grad.launch(grid, st, fa);
        }
        TSC_HIP(hipGetLastError());
        tsc::ProfScope ps(tsc::KID_IQL_REDUCE, st);
        hipLaunchKernelGGL(iql_fused_reduce_kernel, dim3((unsigned)((L.stride + 255) / 256), (unsigned)A), dim3(256), 0, st, h->fws, h->fwsl,
                           (int)A, P.S, L.stride, L.ob1, L.H1, h->rowrange, L.SMAX, h->grads, h->stats);
        TSC_HIP(hipGetLastError());
        return 0;
    }
    const long long tot = A * R * (L.SMAX / 4);
    // multi-step returns: s' and done at the bootstrap slot, the row's return in place of its reward
    hipLaunchKernelGGL(iql_gather_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (int)E, (int)A, L.SMAX, h->B, h->cap,
                       (int)size, h->idx, nstep ? h->ns_slot : h->idx, nstep ? h->ns_ret : nullptr, h->r_obs, h->r_next, h->r_act, h->r_rew,
                       h->r_done, h->S, h->S1, h->act, h->rew, h->done);
    TSC_HIP(hipGetLastError());
    // Q(s') first (its activations are not needed afterwards), then Q(s) with the activations the backward pass reads
    // (armed: Q(s') comes from the frozen copy; Double DQN adds the online net's Q(s'), whose first maximum picks the target's value)
    if (q_forward(h, tp, h->S1, R * L.SMAX, L.SMAX, R, h->X1, h->X2, h->Q)) return tsc::fail("gemm launch failed");
    if (duel) duel_combine(h, h->Q, R);
    if (dbl) {
        if (q_forward(h, h->params, h->S1, R * L.SMAX, L.SMAX, R, h->X1, h->X2, h->Q2)) return tsc::fail("gemm launch failed");
        if (duel) duel_combine(h, h->Q2, R);
        hipLaunchKernelGGL(iql_qsel_kernel, dim3((unsigned)((A * R + 255) / 256)), dim3(256), 0, st, h->Q2, h->Q, h->n_act, R, (int)A, h->q1, h->astar);
    } else {
        hipLaunchKernelGGL(iql_qmax_kernel, dim3((unsigned)((A * R + 255) / 256)), dim3(256), 0, st, h->Q, h->n_act, R, (int)A, h->q1);
    }
    if (q_forward(h, h->params, h->S, R * L.SMAX, L.SMAX, R, h->X1, h->X2, h->Q)) return tsc::fail("gemm launch failed");
    if (duel) duel_combine(h, h->Q, R);
    // the route's options (TdOpts): weights, the rows' own discounts gamma^k, |delta| out, the dueling head's dense dQ row
    const TdOpts td{per ? h->w : duel ? h->w_one : nullptr, nstep ? h->ns_disc : nullptr, per || duel ? h->td : nullptr,
                    duel ? h->n_act : nullptr};
    hipLaunchKernelGGL(iql_td_kernel, dim3((unsigned)((A * R + 255) / 256)), dim3(256), 0, st, h->Q, h->q1, h->act, h->rew, h->done, td, R,
                       (int)A, (float)h->gamma, h->dQ, h->stats);
    TSC_HIP(hipGetLastError());
    float *g = h->grads;
    if (!L.dqn) {
        // dWq = S^T dQ, dbq = colsum(dQ); padded obs columns are zero, so their rows of dWq are exactly zero
        if (qgemm(h, true, tsc::EPI_NONE, L.SMAX, kQ, (int)R, h->S, R * L.SMAX, L.SMAX, h->dQ, R * kQ, kQ, g + L.oWq, L.stride, kQ, nullptr, 0,
                  nullptr, 0, 0, nullptr, 0, g + L.obq, L.stride)) return tsc::fail("gemm failed");
        return 0;
    }
    const long long pt = (long long)L.H1 * L.H2 > (long long)L.H2 * kQ ? (long long)L.H1 * L.H2 : (long long)L.H2 * kQ;
    hipLaunchKernelGGL(iql_transpose_kernel, dim3((unsigned)((pt * A + 255) / 256)), dim3(256), 0, st, h->params, L, h->W2T, h->WqT);
    // dWq = X2^T dQ (+ dbq)
    if (qgemm(h, true, tsc::EPI_NONE, L.H2, kQ, (int)R, h->X2, R * L.H2, L.H2, h->dQ, R * kQ, kQ, g + L.oWq, L.stride, kQ, nullptr, 0, nullptr, 0,
              0, nullptr, 0, g + L.obq, L.stride)) return tsc::fail("gemm failed");
    // dX2 = (dQ Wq^T) * (X2 > 0)
    if (qgemm(h, false, tsc::EPI_MASK_POS, (int)R, L.H2, kQ, h->dQ, R * kQ, kQ, h->WqT, (long long)L.H2 * kQ, L.H2, h->dX2, R * L.H2, L.H2,
              nullptr, 0, h->X2, R * L.H2, L.H2, nullptr, 0, nullptr, 0)) return tsc::fail("gemm failed");
    // dW2 = X1^T dX2 (+ db2)
    if (qgemm(h, true, tsc::EPI_NONE, L.H1, L.H2, (int)R, h->X1, R * L.H1, L.H1, h->dX2, R * L.H2, L.H2, g + L.oW2, L.stride, L.H2, nullptr, 0,
              nullptr, 0, 0, nullptr, 0, g + L.ob2, L.stride)) return tsc::fail("gemm failed");
    // dX1 = (dX2 W2^T) * (X1 > 0), in place over X1
    if (qgemm(h, false, tsc::EPI_MASK_POS, (int)R, L.H1, L.H2, h->dX2, R * L.H2, L.H2, h->W2T, (long long)L.H1 * L.H2, L.H1, h->X1, R * L.H1,
              L.H1, nullptr, 0, h->X1, R * L.H1, L.H1, nullptr, 0, nullptr, 0)) return tsc::fail("gemm failed");
    // dW1 = S^T dX1 masked to the block-diagonal structure (+ db1)
    if (qgemm(h, true, tsc::EPI_ROWRANGE, L.SMAX, L.H1, (int)R, h->S, R * L.SMAX, L.SMAX, h->X1, R * L.H1, L.H1, g + L.oW1, L.stride, L.H1,
              nullptr, 0, nullptr, 0, 0, h->rowrange, L.SMAX, g + L.ob1, L.stride)) return tsc::fail("gemm failed");
    return 0;
}

int tsc_iql_grad_buffer(tsc_iql *h, float **grad, int64_t *count) {
    if (!h || !grad || !count) return tsc::fail("tsc_iql_grad_buffer: bad arguments");
    *grad = h->grads; *count = h->nparam;
    return 0;
}

int tsc_iql_apply_grads(tsc_iql *h, double lr, double grad_scale, double *stats_host) {
    if (!h) return tsc::fail("null handle");
    const QLayout &L = h->lay;
    hipStream_t st = h->stream;
    tsc::ProfScope ps(tsc::KID_IQL_ADAM, st);          // norm + Adam
    launch_share_reduce(h);                            // parameter sharing armed: class members take the class-mean gradient first
    hipLaunchKernelGGL(iql_norm_kernel, dim3(L.A * kNormSlices), dim3(256), 0, st, h->grads, L.stride, grad_scale, h->norm2);
    h->adam_t += 1;
    const double lr_t = lr * sqrt(1.0 - pow(0.999, (double)h->adam_t)) / (1.0 - pow(0.9, (double)h->adam_t));
    hipLaunchKernelGGL(iql_adam_kernel, dim3((unsigned)((h->nparam + 255) / 256)), dim3(256), 0, st, h->params, h->m1, h->m2, h->grads,
                       L.stride, h->nparam, h->norm2, (float)grad_scale, (float)h->max_norm, (float)lr_t);
    TSC_HIP(hipGetLastError());
    ps.stop();
    // target network: the frozen copy follows after every tgt_period-th Adam step of the handle (a resumed run keeps its phase)
    if (h->tgt_period > 0 && h->adam_t % h->tgt_period == 0) TSC_HIP(freeze_params(h));
    if (stats_host) {
        std::vector<double> s(L.A * 2), n2p((size_t)L.A * kNormSlices), n2(L.A, 0.0);
        TSC_HIP(hipStreamSynchronize(st));
        TSC_HIP(hipMemcpy(s.data(), h->stats, sizeof(double) * L.A * 2, hipMemcpyDeviceToHost));
        TSC_HIP(hipMemcpy(n2p.data(), h->norm2, sizeof(double) * L.A * kNormSlices, hipMemcpyDeviceToHost));
        for (int a = 0; a < L.A; ++a)
            for (int k = 0; k < kNormSlices; ++k) n2[a] += n2p[(size_t)a * kNormSlices + k];
        for (int a = 0; a < L.A; ++a) { stats_host[a * 2] = s[a * 2]; stats_host[a * 2 + 1] = sqrt(n2[a]); }
    }
    return 0;
}

int tsc_iql_set_sharing(tsc_iql *h, const int32_t *class_of) {
    if (!h) return tsc::fail("null handle");
    const QLayout &L = h->lay;
    const auto drop = [h]() {
        h->bufs.release(h->share_members); h->bufs.release(h->share_off); h->bufs.release(h->share_invk);
        h->share_members = h->share_off = nullptr; h->share_invk = nullptr;
        h->share_class.clear(); h->share_lists.clear();
    };
    TSC_HIP(hipSetDevice(h->device));
    if (!class_of) {                                  // disarm: parameters, moments and the frozen copy stay as they are
        TSC_HIP(hipStreamSynchronize(h->stream));
        drop();
        return 0;
    }
    const long long per_agent = L.stride;
    if (per_agent % 4) return tsc::fail("tsc_iql_set_sharing: an agent's slice of %lld floats is not a multiple of 4", per_agent);
    std::string bad;
    for (int a = 0; a < L.A; ++a)
        if (class_of[a] < 0 || class_of[a] >= L.A) bad += (bad.empty() ? "" : ", ") + std::to_string(a) + " (id " + std::to_string(class_of[a]) + ")";
    if (!bad.empty()) return tsc::fail("tsc_iql_set_sharing: class id outside [0, %d) for agent(s) %s", L.A, bad.c_str());
    std::vector<std::vector<int>> by_id(L.A);
    for (int a = 0; a < L.A; ++a) by_id[class_of[a]].push_back(a);          // ascending agent indices
    std::vector<std::vector<int>> lists;
    for (const std::vector<int> &cls : by_id) {
        for (size_t j = 1; j < cls.size(); ++j) {
            const int32_t *d0 = &h->dims[(size_t)cls[0] * 3], *d1 = &h->dims[(size_t)cls[j] * 3];
            if (memcmp(d0, d1, sizeof(int32_t) * 3))
                return tsc::fail("tsc_iql_set_sharing: agents %d and %d of class %d have unequal (n_wave, n_wait, n_act): "
                                 "(%d, %d, %d) vs (%d, %d, %d)", cls[0], cls[j], class_of[cls[0]], d0[0], d0[1], d0[2], d1[0], d1[1], d1[2]);
        }
        if (cls.size() >= 2) lists.push_back(cls);
    }
    if (lists.size() > 65535) return tsc::fail("tsc_iql_set_sharing: %zu classes of two or more agents, at most 65535", lists.size());
    std::vector<int> members, off(1, 0);
    std::vector<double> invk;
    for (const std::vector<int> &cls : lists) {
        members.insert(members.end(), cls.begin(), cls.end());
        off.push_back((int)members.size());
        invk.push_back(1.0 / (double)cls.size());
    }
    TSC_HIP(hipStreamSynchronize(h->stream));
    int *d_members = nullptr, *d_off = nullptr;
    double *d_invk = nullptr;
    hipError_t e = h->bufs.upload(&d_members, members.data(), members.size());
    if (e == hipSuccess) e = h->bufs.upload(&d_off, off.data(), off.size());
    if (e == hipSuccess) e = h->bufs.upload(&d_invk, invk.data(), invk.size());
    // the lowest member's parameters, Adam moments and (target network armed) frozen copy become the class's
    for (const std::vector<int> &cls : lists)
        for (size_t j = 1; j < cls.size() && e == hipSuccess; ++j)
            for (float *buf : {h->params, h->m1, h->m2, h->tgt_period ? h->tparams : (float *)nullptr})
                if (buf && e == hipSuccess)
                    e = hipMemcpy(buf + cls[j] * per_agent, buf + cls[0] * per_agent, sizeof(float) * per_agent, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);       // the copies ran on the null stream: done before the handle's stream goes on
    if (e != hipSuccess) {
        h->bufs.release(d_members); h->bufs.release(d_off); h->bufs.release(d_invk);
        TSC_HIP(e);
    }
    drop();
    h->share_members = d_members; h->share_off = d_off; h->share_invk = d_invk;
    h->share_class.assign(class_of, class_of + L.A);
    h->share_lists = std::move(lists);
    return 0;
}

int tsc_iql_get_sharing(tsc_iql *h, int32_t *class_of) {
    if (!h || !class_of) return tsc::fail("tsc_iql_get_sharing: bad arguments");
    for (int a = 0; a < h->lay.A; ++a) class_of[a] = h->share_class.empty() ? a : h->share_class[a];
    return 0;
}

int tsc_iql_share_grads(tsc_iql *h) {
    if (!h) return tsc::fail("null handle");
    launch_share_reduce(h);
    TSC_HIP(hipGetLastError());
    return 0;
}

int tsc_iql_debug_clock(tsc_iql *h, int32_t enable, int64_t *stamps_host, int32_t count) {
    if (!h) return tsc::fail("null handle");
    if (!h->fused) return tsc::fail("tsc_iql_debug_clock: only the fused learner carries clock stamps");
    if (count < 0) return tsc::fail("tsc_iql_debug_clock: count %d < 0", count);
    TSC_HIP(hipStreamSynchronize(h->stream));
    // [64] phase stamps | start / end of the gradient kernel's workgroups | start / end of the target kernel's (armed handles)
    const size_t n = 64 + 4 * (size_t)h->lay.A * h->plan.S;
    if (enable && !h->dbg_buf) {
        TSC_HIP(h->bufs.alloc(&h->dbg_buf, n, true));
    }
    h->dbg = enable ? h->dbg_buf : nullptr;       // off: the kernels stop stamping; the buffer (and what it holds) stays
    if (stamps_host && h->dbg_buf)
        TSC_HIP(hipMemcpy(stamps_host, h->dbg_buf, sizeof(long long) * ((size_t)count < n ? (size_t)count : n), hipMemcpyDeviceToHost));
    return 0;
}

int tsc_iql_set_target(tsc_iql *h, int32_t period, int32_t double_q) {
    if (!h || period < 0 || (double_q != 0 && double_q != 1)) return tsc::fail("tsc_iql_set_target: bad arguments");
    if (double_q && !period) return tsc::fail("tsc_iql_set_target: double_q needs a target network (period > 0)");
    if (period > 0) {
        const QLayout &L = h->lay;
        const long long AR = (long long)L.A * h->E * h->B;
        TSC_HIP(hipSetDevice(h->device));
        // each buffer when its first user arms
        TSC_HIP(alloc_once(h, &h->tparams, h->nparam));
        if (h->fused) TSC_HIP(alloc_once(h, &h->y, AR));                         // (the grouped path keeps q1, see tsc_iql_debug_targets)
        if (double_q) TSC_HIP(alloc_once(h, &h->astar, AR));
        if (double_q && !h->fused) TSC_HIP(alloc_once(h, &h->Q2, AR * kQ));
        if (!h->tgt_period) TSC_HIP(freeze_params(h));       // armed: the frozen copy starts as the parameters
    }
    if (!period || period != h->tgt_period || double_q != h->tgt_double) h->y_valid = false;
    h->tgt_period = period; h->tgt_double = double_q;
    return 0;
}

int tsc_iql_sync_target(tsc_iql *h) {
    if (!h) return tsc::fail("null handle");
    if (!h->tgt_period) return tsc::fail("tsc_iql_sync_target: no target network (tsc_iql_set_target)");
    TSC_HIP(freeze_params(h));
    return 0;
}

int tsc_iql_set_target_params(tsc_iql *h, const float *p) {
    if (!h || !p) return tsc::fail("tsc_iql_set_target_params: bad arguments");
    if (!h->tgt_period) return tsc::fail("tsc_iql_set_target_params: no target network (tsc_iql_set_target)");
    if (share_check_host(h, p, "tsc_iql_set_target_params")) return 1;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(h->tparams, p, sizeof(float) * h->nparam, hipMemcpyHostToDevice));
    return 0;
}

int tsc_iql_get_target_params(tsc_iql *h, float *p) {
    if (!h || !p) return tsc::fail("tsc_iql_get_target_params: bad arguments");
    if (!h->tgt_period) return tsc::fail("tsc_iql_get_target_params: no target network (tsc_iql_set_target)");
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(p, h->tparams, sizeof(float) * h->nparam, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_iql_debug_targets(tsc_iql *h, float *y_host, int32_t *astar_host) {
    if (!h || !y_host) return tsc::fail("tsc_iql_debug_targets: bad arguments");
    if ((!h->tgt_period && !h->duel && h->nstep <= 1) || !h->y_valid) return tsc::fail("tsc_iql_debug_targets: no tsc_iql_compute_grads on an armed handle yet");
    const size_t AR = (size_t)h->lay.A * h->E * h->B;
    TSC_HIP(hipStreamSynchronize(h->stream));
    if (h->fused) {
        TSC_HIP(hipMemcpy(y_host, h->y, sizeof(float) * AR, hipMemcpyDeviceToHost));
    } else {
        // the grouped path keeps q1 (what iql_td_kernel reads): the same float32 expression on the host
        std::vector<float> q1(AR), rew(AR), disc;
        std::vector<uint8_t> done(AR);
        if (h->nstep > 1) {     // a return-steps handle: rew holds G, done the bootstrap slot's flag, and the discount is the row's gamma^k
            disc.resize(AR);
            TSC_HIP(hipMemcpy(disc.data(), h->ns_disc, sizeof(float) * AR, hipMemcpyDeviceToHost));
        }
        TSC_HIP(hipMemcpy(q1.data(), h->q1, sizeof(float) * AR, hipMemcpyDeviceToHost));
        TSC_HIP(hipMemcpy(rew.data(), h->rew, sizeof(float) * AR, hipMemcpyDeviceToHost));
        TSC_HIP(hipMemcpy(done.data(), h->done, AR, hipMemcpyDeviceToHost));
        const float gamma = (float)h->gamma;
        for (size_t i = 0; i < AR; ++i) {
            const float bootstrap = (disc.empty() ? gamma : disc[i]) * q1[i];
            y_host[i] = done[i] ? rew[i] : rew[i] + bootstrap;
        }
    }
    if (astar_host) {
        if (h->tgt_double) TSC_HIP(hipMemcpy(astar_host, h->astar, sizeof(int32_t) * AR, hipMemcpyDeviceToHost));
        else for (size_t i = 0; i < AR; ++i) astar_host[i] = -1;
    }
    return 0;
}

int tsc_iql_set_per(tsc_iql *h, int32_t enable, double alpha, double eps) {
    if (!h) return tsc::fail("null handle");
    if (!enable) { h->per = 0; h->per_valid = false; return 0; }       // back to Floyd sampling and the kernels of an unarmed handle
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return tsc::fail("tsc_iql_set_per: alpha %g must be >= 0", alpha);
    if (!(eps > 0.0) || !std::isfinite(eps)) return tsc::fail("tsc_iql_set_per: eps %g must be > 0", eps);
    if (h->cap > TSC_IQL_PER_MAX_BUFFER)
        return tsc::fail("tsc_iql_set_per: buffer_size %lld > TSC_IQL_PER_MAX_BUFFER (%d): the sampler stages a whole ring in LDS", h->cap,
                         TSC_IQL_PER_MAX_BUFFER);
    const QLayout &L = h->lay;
    const long long rings = (long long)h->E * L.A, AR = rings * h->B, size = replay_size(h);
    TSC_HIP(hipSetDevice(h->device));
    const bool first = !h->prio || !h->qmax;
    TSC_HIP(alloc_once(h, &h->prio, rings * h->cap, false));
    TSC_HIP(alloc_once(h, &h->qmax, rings, false));
    TSC_HIP(alloc_once(h, &h->w, AR));
    TSC_HIP(alloc_once(h, &h->td, AR));
    if (h->fused) TSC_HIP(alloc_once(h, &h->y, AR));
    TSC_HIP(hipFuncSetAttribute((const void *)iql_per_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)per_sample_lds(h)));
    // priorities are powers of alpha, so another alpha starts over; so does arming again after a disarm (slots filled meanwhile have none)
    if (first || !h->per || alpha != h->per_alpha) {
        const long long n = rings * h->cap;
        hipLaunchKernelGGL(iql_per_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, rings, h->cap, size, h->prio, h->qmax);
        TSC_HIP(hipGetLastError());
        h->per_valid = false;
    }
    h->per = 1; h->per_alpha = alpha; h->per_eps = eps;
    return 0;
}

int tsc_iql_set_per_beta(tsc_iql *h, double beta) {
    if (!h) return tsc::fail("null handle");
    if (!(beta >= 0.0 && beta <= 1.0)) return tsc::fail("tsc_iql_set_per_beta: beta %g outside [0, 1]", beta);
    h->per_beta = beta;
    return 0;
}

int tsc_iql_get_priorities(tsc_iql *h, float *prio_host, float *qmax_host) {
    if (!h || !prio_host || !qmax_host) return tsc::fail("tsc_iql_get_priorities: bad arguments");
    if (!h->per) return tsc::fail("tsc_iql_get_priorities: prioritized replay is not armed (tsc_iql_set_per)");
    const size_t rings = (size_t)h->E * h->lay.A;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(prio_host, h->prio, sizeof(float) * rings * h->cap, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(qmax_host, h->qmax, sizeof(float) * rings, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_iql_set_priorities(tsc_iql *h, const float *prio_host, const float *qmax_host) {
    if (!h || !prio_host || !qmax_host) return tsc::fail("tsc_iql_set_priorities: bad arguments");
    if (!h->per) return tsc::fail("tsc_iql_set_priorities: prioritized replay is not armed (tsc_iql_set_per)");
    const size_t rings = (size_t)h->E * h->lay.A, cap = (size_t)h->cap, size = (size_t)replay_size(h);
    for (size_t p = 0; p < rings; ++p) {
        bool mass = size == 0;
        for (size_t s = 0; s < cap; ++s) {
            const float q = prio_host[p * cap + s];
            if (!(q >= 0.f) || !std::isfinite(q)) return tsc::fail("tsc_iql_set_priorities: ring %zu slot %zu: priority %g is not a finite value >= 0", p, s, (double)q);
            mass |= s < size && q > 0.f;
        }
        if (!(qmax_host[p] >= 0.f) || !std::isfinite(qmax_host[p])) return tsc::fail("tsc_iql_set_priorities: ring %zu: qmax %g is not a finite value >= 0", p, (double)qmax_host[p]);
        if (!mass) return tsc::fail("tsc_iql_set_priorities: ring %zu has no positive priority among its %zu filled slots", p, size);
    }
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(h->prio, prio_host, sizeof(float) * rings * cap, hipMemcpyHostToDevice));
    TSC_HIP(hipMemcpy(h->qmax, qmax_host, sizeof(float) * rings, hipMemcpyHostToDevice));
    return 0;
}

int tsc_iql_debug_per(tsc_iql *h, float *w_host, float *td_host) {
    if (!h || !w_host || !td_host) return tsc::fail("tsc_iql_debug_per: bad arguments");
    if (!h->per || !h->per_valid) return tsc::fail("tsc_iql_debug_per: no tsc_iql_compute_grads with prioritized replay armed yet (tsc_iql_set_per)");
    const size_t AR = (size_t)h->lay.A * h->E * h->B;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(w_host, h->w, sizeof(float) * AR, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(td_host, h->td, sizeof(float) * AR, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_iql_set_dueling(tsc_iql *h, int32_t enable) {
    if (!h || (enable != 0 && enable != 1)) return tsc::fail("tsc_iql_set_dueling: bad arguments");
    if (enable != h->duel) h->y_valid = false;
    if (!enable) { h->duel = 0; return 0; }       // back to the kernels of a handle that was never armed
    const QLayout &L = h->lay;
    if (!L.dqn) return tsc::fail("tsc_iql_set_dueling: kind must be 1 (dqn); a linear Q with a value column spans the same functions");
    for (int a = 0; a < L.A; ++a)
        if (h->n_act_host[a] > kQ - 1)
            return tsc::fail("tsc_iql_set_dueling: agent %d has %d actions > %d: column %d of the head is the value stream", a, h->n_act_host[a],
                             kQ - 1, kQ - 1);
    const long long AR = (long long)L.A * h->E * h->B;
    TSC_HIP(hipSetDevice(h->device));
    if (!h->w_one) {
        TSC_HIP(h->bufs.alloc(&h->w_one, AR, false));
        hipLaunchKernelGGL(iql_fill_kernel, dim3((unsigned)((AR + 255) / 256)), dim3(256), 0, h->stream, h->w_one, AR, 1.0f);
        TSC_HIP(hipGetLastError());
    }
    TSC_HIP(alloc_once(h, &h->td, AR));
    if (h->fused) TSC_HIP(alloc_once(h, &h->y, AR));
    h->duel = 1;
    return 0;
}

int tsc_iql_get_dueling(tsc_iql *h, int32_t *enabled) {
    if (!h || !enabled) return tsc::fail("tsc_iql_get_dueling: bad arguments");
    *enabled = h->duel;
    return 0;
}

int tsc_iql_set_return_steps(tsc_iql *h, int32_t n) {
    if (!h) return tsc::fail("null handle");
    if (n < 1 || n > TSC_IQL_MAX_RETURN_STEPS)
        return tsc::fail("tsc_iql_set_return_steps: n %d outside [1, %d]", n, TSC_IQL_MAX_RETURN_STEPS);
    if (n != h->nstep) { h->y_valid = false; h->ns_valid = false; }
    if (n == 1) { h->nstep = 1; return 0; }        // back to the kernels of a handle that was never armed
    const long long AR = (long long)h->lay.A * h->E * h->B;
    TSC_HIP(hipSetDevice(h->device));
    TSC_HIP(alloc_once(h, &h->ns_slot, AR));
    TSC_HIP(alloc_once(h, &h->ns_ret, AR));
    TSC_HIP(alloc_once(h, &h->ns_disc, AR));
    TSC_HIP(alloc_once(h, &h->ns_k, AR));
    if (h->fused) TSC_HIP(alloc_once(h, &h->y, AR));
    h->nstep = n;
    return 0;
}

int tsc_iql_get_return_steps(tsc_iql *h, int32_t *n) {
    if (!h || !n) return tsc::fail("tsc_iql_get_return_steps: bad arguments");
    *n = h->nstep;
    return 0;
}

int tsc_iql_debug_nstep(tsc_iql *h, int32_t *slot_host, float *ret_host, float *disc_host, int32_t *k_host) {
    if (!h || !slot_host || !ret_host || !disc_host || !k_host) return tsc::fail("tsc_iql_debug_nstep: bad arguments");
    if (h->nstep <= 1 || !h->ns_valid)
        return tsc::fail("tsc_iql_debug_nstep: no tsc_iql_compute_grads with return_steps > 1 yet (tsc_iql_set_return_steps)");
    const size_t AR = (size_t)h->lay.A * h->E * h->B;
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(slot_host, h->ns_slot, sizeof(int32_t) * AR, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(ret_host, h->ns_ret, sizeof(float) * AR, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(disc_host, h->ns_disc, sizeof(float) * AR, hipMemcpyDeviceToHost));
    TSC_HIP(hipMemcpy(k_host, h->ns_k, sizeof(int32_t) * AR, hipMemcpyDeviceToHost));
    return 0;
}

int tsc_iql_path(tsc_iql *h, int32_t *fused) {
    if (!h || !fused) return tsc::fail("tsc_iql_path: bad arguments");
    *fused = h->fused ? 1 : 0;
    return 0;
}

int tsc_iql_debug_batch(tsc_iql *h, int32_t *idx_host) {
    if (!h || !idx_host) return tsc::fail("tsc_iql_debug_batch: bad arguments");
    TSC_HIP(hipStreamSynchronize(h->stream));
    TSC_HIP(hipMemcpy(idx_host, h->idx, sizeof(int) * (size_t)h->E * h->lay.A * h->B, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
