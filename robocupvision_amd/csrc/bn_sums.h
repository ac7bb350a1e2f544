// The BatchNorm partial sums that kernel epilogues accumulate per lane: THE definition of RCV_STATS_FWD / BWD_ENC / BWD_DEC.
//   v = the four consecutive channels the lane has just stored, e = the stored tensor the gradient passes through (epi_aux),
//   e0 / e1 / mu = rows 0 / 1 / 2 of the producer's constants (epi_c).
//   forward:           s1 += v,  s2 += v * v
//   encoder backward:  s1 += v,  s2 += v * (e - mu)
//   decoder backward:  g = e * e0 + e1 > 0 ? v : 0 (the ReLU between the BatchNorm and the consumer),  then the encoder's sums of g
// Accumulators are float[4] (conv kernels: one set per 16-channel block) or float4 (pointwise kernels).  Results are pinned bit for
// bit across the users (tests/test_gpu_kernels.py::test_epilogue_statistics_exact): keep the expressions and the fmaf order.
// float4 operands are passed by value: by reference the callers' code is scheduled differently (scripts/isa_diff.sh).
#pragma once
#include "rcv_internal.h"

__device__ __forceinline__ float4 bn_relu_mask(float4 v, float4 e, float4 e0, float4 e1) {
  return make_float4(fmaf(e.x, e0.x, e1.x) > 0.f ? v.x : 0.f, fmaf(e.y, e0.y, e1.y) > 0.f ? v.y : 0.f,
                     fmaf(e.z, e0.z, e1.z) > 0.f ? v.z : 0.f, fmaf(e.w, e0.w, e1.w) > 0.f ? v.w : 0.f);
}

__device__ __forceinline__ void bn_sums_fwd(float (&s1)[4], float (&s2)[4], float4 v) {
  s1[0] += v.x; s1[1] += v.y; s1[2] += v.z; s1[3] += v.w;
  s2[0] = fmaf(v.x, v.x, s2[0]); s2[1] = fmaf(v.y, v.y, s2[1]); s2[2] = fmaf(v.z, v.z, s2[2]); s2[3] = fmaf(v.w, v.w, s2[3]);
}
__device__ __forceinline__ void bn_sums_bwd_enc(float (&s1)[4], float (&s2)[4], float4 v, float4 e, float4 mu) {
  s1[0] += v.x; s1[1] += v.y; s1[2] += v.z; s1[3] += v.w;
  s2[0] = fmaf(v.x, e.x - mu.x, s2[0]); s2[1] = fmaf(v.y, e.y - mu.y, s2[1]);
  s2[2] = fmaf(v.z, e.z - mu.z, s2[2]); s2[3] = fmaf(v.w, e.w - mu.w, s2[3]);
}
__device__ __forceinline__ void bn_sums_bwd_dec(float (&s1)[4], float (&s2)[4], float4 v, float4 e, float4 e0,
                                                float4 e1, float4 mu) {
  bn_sums_bwd_enc(s1, s2, bn_relu_mask(v, e, e0, e1), e, mu);
}

__device__ __forceinline__ void bn_sums_bwd_enc(float4& s1, float4& s2, float4 v, float4 e, float4 mu) {
  s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
  s2.x = fmaf(v.x, e.x - mu.x, s2.x); s2.y = fmaf(v.y, e.y - mu.y, s2.y);
  s2.z = fmaf(v.z, e.z - mu.z, s2.z); s2.w = fmaf(v.w, e.w - mu.w, s2.w);
}

// Sum of each of the N values of s1 / s2 over the 16 lanes of a group (xor 1, 2, 4, 8 stays inside it), in a fixed order; every lane
// ends with the sums.  One call covers all the accumulators of a lane (a [WM][4] array is passed as its 4 * WM contiguous floats):
// with the loop over the channel blocks left to the caller the compiler schedules the shuffles differently.
template <int N>
__device__ __forceinline__ void bn_reduce16(float* s1, float* s2) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float u = s1[i], v = s2[i];
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) { u += __shfl_xor(u, sh); v += __shfl_xor(v, sh); }
    s1[i] = u; s2[i] = v;
  }
}
