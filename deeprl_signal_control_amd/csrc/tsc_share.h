// Parameter sharing: the class-mean reduce of both learners (tsc_model.hip tsc_model_set_sharing, tsc_iql.hip tsc_iql_set_sharing) --
// one body, instantiated in each translation unit that includes this header (internal linkage).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Parameter sharing (tsc_model_set_sharing, tsc_iql_set_sharing): every member of a class takes the class mean of the members' gradient
// slices, in place.
// Grid (ceil(per_agent / 4 / 256), classes with >= 2 members); a thread owns one 16-byte column of four floats: it loads the column
// of every member (members[off[c] .. off[c + 1]), ascending agent indices), adds in float64 in that order, multiplies by the float64
// inv_k[c] = 1 / k, rounds once to float32 and stores the result to every member.  It reads all of its inputs before it writes
// any, and no other thread touches them: no atomics, no LDS, deterministic.  per_agent % 4 == 0 (checked when sharing is armed).
__global__ void __launch_bounds__(256) share_reduce_kernel(float *__restrict__ grads, long long per_agent, const int *__restrict__ members,
                                                           const int *__restrict__ off, const double *__restrict__ inv_k) {
    const long long i = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i >= per_agent) return;
    const int c = blockIdx.y, lo = off[c], hi = off[c + 1];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int j = lo; j < hi; ++j) {
        const float4 v = *(const float4 *)(grads + (long long)members[j] * per_agent + i);
        s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
    }
    const double ik = inv_k[c];
    const float4 r = make_float4((float)(s0 * ik), (float)(s1 * ik), (float)(s2 * ik), (float)(s3 * ik));
    for (int j = lo; j < hi; ++j) *(float4 *)(grads + (long long)members[j] * per_agent + i) = r;
}

}  // namespace
