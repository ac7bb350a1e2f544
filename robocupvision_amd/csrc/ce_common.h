// The per-pixel pieces and the reductions of the weighted cross entropy, shared by the kernels that form a loss from logits still in
// registers (small_kernels.hip: cls_fwd_kernel<CE>, the training-step kernel, ce_norm_kernel, ce_finalize_kernel; cls_valid.hip: the
// validation tails and their fold), so that each of them rounds and sums as the others do.
#pragma once
#include "rcv_internal.h"

#define CE_MAX_C 8

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh);
  return v;
}

// weight of a pixel's label: a label outside [0, C) (e.g. -100) is ignored, like NLLLoss's ignore_index
__device__ __forceinline__ float ce_label_weight(int tg, int C, const float* __restrict__ cw) {
  return (unsigned)tg < (unsigned)C ? (cw ? cw[tg] : 1.f) : 0.f;
}
// first maximum in class order (torch.max): strict '>', a NaN never wins
template <int NC>
__device__ __forceinline__ float ce_first_max(const float (&lg)[NC], int C, int& am) {
  float mx = -INFINITY;
  am = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) if (c < C && lg[c] > mx) { mx = lg[c]; am = c; }
  return mx;
}
// the logit of the pixel's label (a label outside [0, C) has none: 0, and its weight is 0 too)
template <int NC>
__device__ __forceinline__ float ce_target_logit(const float (&lg)[NC], int C, int tg) {
  float vt = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) if (c == tg && c < C) vt = lg[c];
  return vt;
}
// one pixel's share of the three sums, from the maximum of its logits, the label's logit and se = sum_c exp(lg[c] - mx)
// (OK: double in cls_fwd_kernel; the step kernel counts in an int, exact as well and a register less)
template <class OK>
__device__ __forceinline__ void ce_pixel_sums(float mx, float vt, float se, int am, int tg, int C, const float* __restrict__ cw,
                                              double& a_nll, double& a_w, OK& a_ok) {
  const float wt = ce_label_weight(tg, C, cw);
  const float nll = (mx - vt) + logf(se);
  a_nll += (double)(wt * nll);
  a_w += (double)wt;
  a_ok += (am == tg) ? OK(1) : OK(0);
}
// a workgroup's partial row: wave shuffles, then the waves through LDS in index order, rounded to float once.  w_row: the row's
// sum of weights where ce_norm_kernel has formed it already (the same sum in the same order), in place of a_w
__device__ __forceinline__ void ce_store_row(double a_nll, double a_w, double a_ok, float* __restrict__ row, const float* __restrict__ w_row = nullptr) {
  __shared__ double sh[3][4];
  a_nll = wave_sum_d(a_nll); a_w = wave_sum_d(a_w); a_ok = wave_sum_d(a_ok);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = a_nll; sh[1][wv] = a_w; sh[2][wv] = a_ok; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[threadIdx.x][i];
    row[threadIdx.x] = (w_row && threadIdx.x == 1) ? w_row[0] : (float)t;
  }
}

// the partial rows of a loss -> loss_out[4] = { sum w*nll / sum w, sum w, #correct, sum w*nll }: threads strided over the rows, wave
// shuffles, the waves in index order (one workgroup)
__device__ __forceinline__ void ce_finalize_body(const float* __restrict__ part, int n_part, float* __restrict__ loss_out) {
  __shared__ double sh[3][4];
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n_part; i += blockDim.x) {
    s[0] += (double)part[(size_t)i * 3 + 0]; s[1] += (double)part[(size_t)i * 3 + 1]; s[2] += (double)part[(size_t)i * 3 + 2];
  }
  const int wv = threadIdx.x >> 6;
  for (int j = 0; j < 3; ++j) { s[j] = wave_sum_d(s[j]); if ((threadIdx.x & 63) == 0) sh[j][wv] = s[j]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < 3; ++j) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t[j] += sh[j][i];
    loss_out[0] = (float)(t[0] / t[1]);
    loss_out[1] = (float)t[1];
    loss_out[2] = (float)t[2];
    loss_out[3] = (float)t[0];
  }
}

// number of workgroups used by the reducing stream kernels (deterministic function of the shape)
static inline int reduce_grid(const rcv_handle* h, size_t work_items, int block) {
  size_t g = (work_items + block - 1) / block;
  const size_t cap = (size_t)h->num_cus * 4;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
