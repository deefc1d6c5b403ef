// Shared host-side helpers for the tsc C-ABI library: error plumbing, the owner of a handle's device buffers, kernel timing.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

namespace tsc {

inline char *err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return 1;
}

#define TSC_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return tsc::fail("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

// A create function's handle until it is handed out: an error return on the way destroys it (and the device buffers it owns);
// the error text stays in the thread's buffer (the destroy functions do not write it).
template <class H, int (*Destroy)(H *)>
struct CreateGuard {
    H *h;
    explicit CreateGuard(H *h_) : h(h_) {}
    CreateGuard(const CreateGuard &) = delete;
    CreateGuard &operator=(const CreateGuard &) = delete;
    ~CreateGuard() { if (h) (void)Destroy(h); }
    H *release() { H *t = h; h = nullptr; return t; }
};

// The device allocations of one handle (tsc_env, tsc_model, tsc_iql): every buffer is registered the moment it exists and freed
// with the handle, or earlier by release().  A call that fails frees what it allocated and leaves *field as it was.  `Mem` is the
// four device calls; tests/device_bufs_check.cpp runs the bookkeeping over host stubs.
struct HipMem {
    static hipError_t malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t zero(void *p, size_t bytes) { return hipMemset(p, 0, bytes); }
    static hipError_t copy(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    static void free(void *p) { (void)hipFree(p); }
};

template <class Mem>
struct DeviceBufsT {
    std::vector<void *> owned;
    DeviceBufsT() = default;
    DeviceBufsT(const DeviceBufsT &) = delete;
    DeviceBufsT &operator=(const DeviceBufsT &) = delete;
    ~DeviceBufsT() { for (void *p : owned) Mem::free(p); }

    template <class T> hipError_t alloc(T **field, size_t count, bool zero) {
        return make(field, count, [&](void *d) { return zero ? Mem::zero(d, sizeof(T) * count) : hipSuccess; });
    }
    // count == 0: one element, nothing copied (a kernel argument that is never read, but not null)
    template <class T> hipError_t upload(T **field, const std::remove_const_t<T> *src, size_t count) {
        return make(field, count ? count : 1, [&](void *d) { return count ? Mem::copy(d, src, sizeof(T) * count) : hipSuccess; });
    }
    void release(const void *p) {               // null, or not one of ours: nothing
        for (auto it = owned.begin(); p && it != owned.end(); ++it)
            if (*it == p) { Mem::free(*it); owned.erase(it); return; }
    }

private:
    template <class T, class Fill> hipError_t make(T **field, size_t count, Fill fill) {
        void *d = nullptr;
        hipError_t e = Mem::malloc(&d, sizeof(T) * count);
        if (e != hipSuccess) return e;
        owned.push_back(d);
        e = fill(d);
        if (e != hipSuccess) release(d);
        else *field = (T *)d;
        return e;
    }
};
using DeviceBufs = DeviceBufsT<HipMem>;

// ---- per-kernel timing with HIP events (bench.py's live roofline figure) -------------------------
// Off by default.  When on, launch sites bracket their kernel with two events on the launch stream;
// tsc_profile_read() synchronises and folds the elapsed times per kernel id.  An event pair costs a few
// microseconds of serialisation between dependent kernels (5 % of the rollout when every launch is bracketed), so
// the per-control-step kernels are SAMPLED: every `stride`-th launch of a kernel id is timed, all are counted, and
// the reported total is average x launches.
enum KernelId : int {
    KID_ENV_STEP = 0, KID_FC_GEMM, KID_ZX_GEMM, KID_LSTM_FWD, KID_HEAD_FWD, KID_SAMPLE, KID_ADD_TRANS,
    KID_RETURNS, KID_HEAD_BWD, KID_LSTM_BWD, KID_DWO_GEMM, KID_DWH_GEMM, KID_DWX_GEMM, KID_DX1_GEMM,
    KID_DW1_GEMM, KID_GRADNORM, KID_RMSPROP, KID_TRANSPOSE, KID_FINGERPRINT, KID_FUSED_FWD,
    KID_IQL_ACT, KID_IQL_GRAD, KID_IQL_REDUCE, KID_IQL_SAMPLE, KID_IQL_ADD, KID_IQL_ADAM, KID_IQL_TARGET,
    KID_IQL_PER_SAMPLE, KID_IQL_PER_UPDATE, KID_IQL_PER_ADD, KID_IQL_NSTEP, KID_PRESSURE, KID_PRESSURE_REWARD, KID_ACTUATED, KID_DEMAND,
    KID_GAE, KID_HEAD_BWD_PPO, KID_COUNT
};

struct ProfState {
    bool on = false;
    unsigned long long only = ~0ull;              // bit k: kernel id k is timed (tsc_profile_select); the others are only counted
    int stride = 1;                               // time every stride-th launch of the per-control-step kernels
    long long seq[KID_COUNT] = {0};               // all launches
    struct Rec { int id; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double total_ms[KID_COUNT] = {0};
    long long count[KID_COUNT] = {0};
};
ProfState &prof();          // defined in tsc_env.hip

struct ProfScope {
    int id; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(int id_, hipStream_t st_) : id(id_), st(st_) {
        ProfState &p = prof();
        if (!p.on) return;
        const bool per_step = id == KID_ENV_STEP || id == KID_FUSED_FWD || id == KID_ADD_TRANS || id == KID_FINGERPRINT ||
                              id == KID_SAMPLE || id == KID_IQL_ACT || id == KID_IQL_ADD || id == KID_IQL_PER_ADD || id == KID_PRESSURE || id == KID_PRESSURE_REWARD || id == KID_ACTUATED;
        if (p.seq[id]++ % (per_step ? p.stride : 1) != 0) return;
        if (!((p.only >> id) & 1ull)) return;
        auto get = [&]() { hipEvent_t e; if (!p.pool.empty()) { e = p.pool.back(); p.pool.pop_back(); } else { (void)hipEventCreate(&e); } return e; };
        a = get(); b = get();
        (void)hipEventRecord(a, st);
    }
    void stop() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        prof().recs.push_back({id, a, b});
        a = nullptr;
    }
    ~ProfScope() { stop(); }
};

}  // namespace tsc

// base + 32-bit byte offset: with a workgroup-uniform base the compiler uses the scalar-base addressing mode
// (one VGPR per address instead of a 64-bit pair that tends to be spilled when many addresses are live)
template <class T> __device__ __forceinline__ T ldg(const T *base, unsigned byte_off) {
    return *(const T *)((const char *)base + byte_off);
}
template <class T> __device__ __forceinline__ void stg(T *base, unsigned byte_off, T v) {
    *(T *)((char *)base + byte_off) = v;
}

// the counter-based uniform tsc_model_sample documents, U(seed, step, idx) in [0, 1): the one definition behind every device draw
// (action sampling of both learners, Floyd and prioritized replay sampling)
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ double uniform01(unsigned long long seed, unsigned long long step, unsigned long long idx) {
    const unsigned long long h = splitmix64(splitmix64(seed ^ (step * 0xD1B54A32D192ED03ull)) + idx);
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

