// LabelProp in training mode (model.py:563-567, labelPropTrain.py:162-215): the tail of the network and the batch assembly.
//
// The tail is  logits = W . v + b  with  v[c] = relu(t[c]*c0[c] + c1[c]) + (c < rch ? f(r[c]) : 0):  t = upConv3's stored
// pre-BatchNorm output (16 channels NHWC), r = `pre`'s stored conv output read through its load transform, rch = 8.  The ReLU of
// upConv3 is taken BEFORE the skip is added (the out-of-place form of `x[:,0:8] = x[:,0:8] + top`), so its backward mask is
// t*c0 + c1 > 0.  Inference runs the same forward as RCV_OP_CLS_FWD (cls_fwd16_kernel<true>, small_kernels.hip); here are
//   * RCV_OP_LP_TAIL_FWD, the training forward, with or without the weighted cross entropy fused in (RCV_F_FUSED_CE),
//   * RCV_OP_LP_TAIL_BWD, its backward, from a logits-gradient tensor or (RCV_F_FUSED_CE) from the re-formed soft-max,
//   * RCV_OP_LP_BATCH, the batch assembly of the training script.
// All three are HBM-bound streams.  FOUR lanes share a pixel, one 16-byte channel quad each (as cls_fwd16_kernel: every load / store
// instruction of a wave covers 1 KB of consecutive memory); the logits are formed by ONE expression and butterfly order in all of
// them (lp_logit), so the logits the backward re-forms are the forward's bits and the fused-loss path equals the logits-gradient
// path bit for bit.  A workgroup walks chunks of 256 consecutive pixels (chunk = blockIdx.x + k * gridDim.x): the pixel set of a
// workgroup -- and with it every loss partial row -- is that of ce_fwd_kernel.  Reductions: per-lane sums, shuffles across the 16
// lanes of a wave that own the same channel quad, the 4 waves through LDS in fixed order, one partial row per workgroup, then the
// fixed-order kernels the 8-channel classifier uses (ce_finalize_kernel, rows_reduce_kernel); no float atomics.
#include "rcv_internal.h"

#define LP_MAX_OUT 8
#define LP_CIN 16

__device__ __forceinline__ float4 lp_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void lp_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// sum over the lanes of a wave that own the same channel quad (lane & 3)
__device__ __forceinline__ float quad_lane_sum(float v) {
#pragma unroll
  for (int sh = 32; sh >= 4; sh >>= 1) v += __shfl_xor(v, sh);
  return v;
}
__device__ __forceinline__ double lp_wave_sum_d(double v) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh);
  return v;
}

// per-lane constants of the load transforms: channel quad q of t (scale s, shift h) and of the skip tensor (s2, h2)
struct LpConsts {
  float4 s, h, s2, h2;
  bool has_skip;
};
__device__ __forceinline__ LpConsts lp_consts(const float* __restrict__ tc, const float* __restrict__ rc, int mode2, int rch, int q) {
  LpConsts k;
  k.s = lp_ld4(tc + 4 * q); k.h = lp_ld4(tc + LP_CIN + 4 * q);
  k.s2 = make_float4(1.f, 1.f, 1.f, 1.f); k.h2 = make_float4(0.f, 0.f, 0.f, 0.f);
  k.has_skip = 4 * q < rch;
  if (k.has_skip && mode2 != RCV_LOAD_PLAIN) { k.s2 = lp_ld4(rc + 4 * q); k.h2 = lp_ld4(rc + rch + 4 * q); }
  return k;
}

// v = relu(bn(t)) + f(r) for this lane's channel quad (the arithmetic of cls_fwd16_kernel<true>)
__device__ __forceinline__ float4 lp_form_v(float4 a, const LpConsts& k, const float* __restrict__ r, size_t p, int rch, int q, int mode2) {
  a.x = fmaxf(fmaf(a.x, k.s.x, k.h.x), 0.f); a.y = fmaxf(fmaf(a.y, k.s.y, k.h.y), 0.f);
  a.z = fmaxf(fmaf(a.z, k.s.z, k.h.z), 0.f); a.w = fmaxf(fmaf(a.w, k.s.w, k.h.w), 0.f);
  if (k.has_skip) {
    float4 b = lp_ld4(r + p * rch + 4 * q);
    if (mode2 != RCV_LOAD_PLAIN) {
      b.x = fmaf(b.x, k.s2.x, k.h2.x); b.y = fmaf(b.y, k.s2.y, k.h2.y); b.z = fmaf(b.z, k.s2.z, k.h2.z); b.w = fmaf(b.w, k.s2.w, k.h2.w);
      if (mode2 == RCV_LOAD_AFFINE_RELU) { b.x = fmaxf(b.x, 0.f); b.y = fmaxf(b.y, 0.f); b.z = fmaxf(b.z, 0.f); b.w = fmaxf(b.w, 0.f); }
    }
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  return a;
}

// logit c of the pixel this lane shares with its three neighbours: quad partial, two butterfly steps, bias (cls_fwd16_kernel's order)
__device__ __forceinline__ float lp_logit(float4 v, const float* __restrict__ ws, int c, int q) {
  const float* wc = ws + c * LP_CIN + 4 * q;
  float u = fmaf(v.x, wc[0], fmaf(v.y, wc[1], fmaf(v.z, wc[2], v.w * wc[3])));
  u += __shfl_xor(u, 1);
  u += __shfl_xor(u, 2);
  return u + ws[LP_MAX_OUT * LP_CIN + c];
}

// ------------------------------------------------------------------------------------------
// forward: NCHW logits; CE: + loss partial rows [gridDim.x][3] (sum w*nll, sum w, #correct) and the arg-max plane
// ------------------------------------------------------------------------------------------
template <bool CE>
__global__ __launch_bounds__(256) void lp_tail_fwd_kernel(const float* __restrict__ t, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ out, int N, int HW, int COUT, const float* __restrict__ tc,
                                                             const float* __restrict__ r, const float* __restrict__ rc, int mode2, int rch,
                                                             const int64_t* __restrict__ target, const float* __restrict__ cw,
                                                             float* __restrict__ part, uint8_t* __restrict__ argmax) {
  __shared__ float ws[LP_MAX_OUT * LP_CIN + LP_MAX_OUT];
  __shared__ double sh[3][4];
  for (int e = threadIdx.x; e < LP_MAX_OUT * LP_CIN; e += blockDim.x) ws[e] = e < COUT * LP_CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < LP_MAX_OUT; e += blockDim.x) ws[LP_MAX_OUT * LP_CIN + e] = (bias && e < COUT) ? bias[e] : 0.f;
  __syncthreads();
  const int q = threadIdx.x & 3, sub = threadIdx.x >> 2;
  const LpConsts k = lp_consts(tc, rc, mode2, rch, q);
  double a_nll = 0.0, a_w = 0.0, a_ok = 0.0;
  const size_t total = (size_t)N * HW;
  for (size_t chunk = blockIdx.x; chunk * 256 < total; chunk += gridDim.x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t p = chunk * 256 + j * 64 + sub;      // the four lanes of a pixel are in or out together: the butterflies stay inside them
      if (p < total) {
        const float4 v = lp_form_v(lp_ld4(t + p * LP_CIN + 4 * q), k, r, p, rch, q, mode2);
        float lg[LP_MAX_OUT];
#pragma unroll
        for (int c = 0; c < LP_MAX_OUT; ++c) lg[c] = lp_logit(v, ws, c, q);
        const size_t n = p / HW, hw = p % HW;
#pragma unroll
        for (int c = 0; c < LP_MAX_OUT; ++c)
          if ((c & 3) == q && c < COUT) out[(n * COUT + c) * HW + hw] = lg[c];
        if (CE && q == 0) {      // the loss terms of ce_fwd_kernel, once per pixel
          float mx = -INFINITY;
          int am = 0;
#pragma unroll
          for (int c = 0; c < LP_MAX_OUT; ++c) if (c < COUT && lg[c] > mx) { mx = lg[c]; am = c; }
          float se = 0.f;
#pragma unroll
          for (int c = 0; c < LP_MAX_OUT; ++c) if (c < COUT) se += expf(lg[c] - mx);
          const int tg = (int)target[p];
          float vt = 0.f;
#pragma unroll
          for (int c = 0; c < LP_MAX_OUT; ++c) if (c == tg) vt = lg[c];
          const float wt = (unsigned)tg < (unsigned)COUT ? (cw ? cw[tg] : 1.f) : 0.f;
          const float nll = (mx - vt) + logf(se);
          a_nll += (double)(wt * nll);
          a_w += (double)wt;
          a_ok += (am == tg) ? 1.0 : 0.0;
          if (argmax) argmax[p] = (uint8_t)am;
        }
      }
    }
  }
  if (!CE) return;
  a_nll = lp_wave_sum_d(a_nll); a_w = lp_wave_sum_d(a_w); a_ok = lp_wave_sum_d(a_ok);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = a_nll; sh[1][wv] = a_w; sh[2][wv] = a_ok; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[threadIdx.x][i];
    part[(size_t)blockIdx.x * 3 + threadIdx.x] = (float)s;
  }
}

// ------------------------------------------------------------------------------------------
// backward: g = W^T . dlogits (16 channels) -> dup (gradient of upConv3's output, with its RCV_STATS_BWD_DEC partial rows) and
// g[0:rch] -> dskip (dense rch-channel NHWC: the skip gradient of `pre`'s output); dW / db partial rows [gridDim.x][COUT*16+COUT].
// CE: dlogits re-formed from the soft-max of the re-formed logits with ce_bwd_kernel's rounding.
// ------------------------------------------------------------------------------------------
template <int COUT, bool CE>
__global__ __launch_bounds__(256) void lp_tail_bwd_kernel(const float* __restrict__ t, const float* __restrict__ dl, const float* __restrict__ w,
                                                          float* __restrict__ dup, float* __restrict__ dskip, const float* __restrict__ tc,
                                                          float* __restrict__ stat_part, float* __restrict__ w_part, int N, int HW,
                                                          const float* __restrict__ r, const float* __restrict__ rc, int mode2, int rch,
                                                          const int64_t* __restrict__ target, const float* __restrict__ cw,
                                                          const float* __restrict__ bias, const float* __restrict__ loss_out,
                                                          const float* __restrict__ grad_out) {
  constexpr int WROW = COUT * LP_CIN + COUT, ROW = WROW + 2 * LP_CIN;
  __shared__ float ws[LP_MAX_OUT * LP_CIN + LP_MAX_OUT];
  __shared__ float red[4][ROW];
  for (int e = threadIdx.x; e < LP_MAX_OUT * LP_CIN; e += blockDim.x) ws[e] = e < COUT * LP_CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < LP_MAX_OUT; e += blockDim.x) ws[LP_MAX_OUT * LP_CIN + e] = (CE && bias && e < COUT) ? bias[e] : 0.f;
  __syncthreads();
  const int q = threadIdx.x & 3, sub = threadIdx.x >> 2;
  const LpConsts k = lp_consts(tc, rc, mode2, rch, q);
  const float4 mean = lp_ld4(tc + 2 * LP_CIN + 4 * q);
  float scale = 0.f;
  if (CE) scale = grad_out[0] / loss_out[1];
  float dw[COUT][4], db[COUT], s1[4], s2[4];
#pragma unroll
  for (int c = 0; c < COUT; ++c) { db[c] = 0.f; dw[c][0] = 0.f; dw[c][1] = 0.f; dw[c][2] = 0.f; dw[c][3] = 0.f; }
#pragma unroll
  for (int j = 0; j < 4; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  const size_t total = (size_t)N * HW;
  for (size_t chunk = blockIdx.x; chunk * 256 < total; chunk += gridDim.x) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const size_t p = chunk * 256 + it * 64 + sub;
      if (p < total) {
        const float4 a = lp_ld4(t + p * LP_CIN + 4 * q);
        const float4 v = lp_form_v(a, k, r, p, rch, q, mode2);
        float g[COUT];
        if (CE) {
          float mx = -INFINITY;
#pragma unroll
          for (int c = 0; c < COUT; ++c) { g[c] = lp_logit(v, ws, c, q); mx = fmaxf(mx, g[c]); }
          float se = 0.f;
#pragma unroll
          for (int c = 0; c < COUT; ++c) { g[c] = expf(g[c] - mx); se += g[c]; }
          const int tg = (int)target[p];
          const float kf = scale * ((unsigned)tg < (unsigned)COUT ? (cw ? cw[tg] : 1.f) : 0.f);
          const float inv = 1.f / se;
#pragma unroll
          for (int c = 0; c < COUT; ++c) g[c] = __fmul_rn(kf, fmaf(g[c], inv, c == tg ? -1.f : 0.f));      // explicit: same rounding as ce_bwd_kernel
        } else {
          const size_t n = p / HW, hw = p % HW;
#pragma unroll
          for (int c = 0; c < COUT; ++c) g[c] = dl[(n * COUT + c) * HW + hw];
        }
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float acc = 0.f;
#pragma unroll
          for (int c = 0; c < COUT; ++c) acc = fmaf(g[c], ws[c * LP_CIN + 4 * q + j], acc);
          d[j] = acc;
        }
        const float4 d4 = make_float4(d[0], d[1], d[2], d[3]);
        lp_st4(dup + p * LP_CIN + 4 * q, d4);
        if (k.has_skip) lp_st4(dskip + p * rch + 4 * q, d4);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < COUT; ++c) {
          db[c] += g[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) dw[c][j] = fmaf(g[c], vv[j], dw[c][j]);
        }
        // BatchNorm-backward sums of upConv3 (RCV_STATS_BWD_DEC): the ReLU mask is that of relu(bn(t)) alone
        const float tv[4] = {a.x, a.y, a.z, a.w};
        const float sc[4] = {k.s.x, k.s.y, k.s.z, k.s.w}, hf[4] = {k.h.x, k.h.y, k.h.z, k.h.w}, mu[4] = {mean.x, mean.y, mean.z, mean.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gm = fmaf(tv[j], sc[j], hf[j]) > 0.f ? d[j] : 0.f;
          s1[j] += gm;
          s2[j] = fmaf(gm, tv[j] - mu[j], s2[j]);
        }
      }
    }
  }
  // block reduction: the 16 lanes of a wave with this lane's channel quad, then the 4 waves through LDS in fixed order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < COUT; ++c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float x = quad_lane_sum(dw[c][j]); if (lane < 4) red[wv][c * LP_CIN + 4 * q + j] = x; }
    const float x = quad_lane_sum(db[c]);      // every lane of a pixel holds the same dlogits: quad 0 books them
    if (lane == 0) red[wv][COUT * LP_CIN + c] = x;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x1 = quad_lane_sum(s1[j]), x2 = quad_lane_sum(s2[j]);
    if (lane < 4) { red[wv][WROW + 4 * q + j] = x1; red[wv][WROW + LP_CIN + 4 * q + j] = x2; }
  }
  __syncthreads();
  const int nw = blockDim.x >> 6;
  for (int e = threadIdx.x; e < ROW; e += blockDim.x) {
    float x = 0.f;
    for (int i = 0; i < nw; ++i) x += red[i][e];
    if (e < WROW) w_part[(size_t)blockIdx.x * WROW + e] = x;
    else stat_part[(size_t)blockIdx.x * 2 * LP_CIN + (e - WROW)] = x;
  }
}

typedef void (*lp_bwd_fn)(const float*, const float*, const float*, float*, float*, const float*, float*, float*, int, int, const float*,
                          const float*, int, int, const int64_t*, const float*, const float*, const float*, const float*);
template <bool CE>
static lp_bwd_fn lp_bwd_pick(int cout) {
  switch (cout) {
    case 1: return lp_tail_bwd_kernel<1, CE>;
    case 2: return lp_tail_bwd_kernel<2, CE>;
    case 3: return lp_tail_bwd_kernel<3, CE>;
    case 4: return lp_tail_bwd_kernel<4, CE>;
    case 5: return lp_tail_bwd_kernel<5, CE>;
    case 6: return lp_tail_bwd_kernel<6, CE>;
    case 7: return lp_tail_bwd_kernel<7, CE>;
    case 8: return lp_tail_bwd_kernel<8, CE>;
  }
  return nullptr;
}

// ------------------------------------------------------------------------------------------
// RCV_OP_LP_BATCH (labelPropTrain.py:162-193, transform.py:172-183): frame pairs -> the two 8-channel samples of each pair, NHWC.
//   sample 2b   = [Ya, Yb, Ya - Yb, labelToPred(label_b)], target label_a;   sample 2b+1 = [Yb, Ya, Yb - Ya, labelToPred(label_a)],
//   target label_b;  Y = channel 0 of a frame; labelToPred = -1 everywhere, +1 at the label's class.  A label outside [0, 5) selects no
//   class (all five channels -1); it is never used as an index.  One thread per pixel of a pair: two 32-byte pixels out.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_batch_kernel(const float* __restrict__ images, const int64_t* __restrict__ labels, float* __restrict__ out,
                                                       int64_t* __restrict__ tgt, int B, int C, int HW) {
  const size_t total = (size_t)B * HW;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t b = e / HW, hw = e % HW;
    const float ya = images[((b * 2 + 0) * C) * HW + hw], yb = images[((b * 2 + 1) * C) * HW + hw];
    const int64_t la = labels[(b * 2 + 0) * HW + hw], lb = labels[(b * 2 + 1) * HW + hw];
    float pa[5], pb[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) { pa[c] = la == (int64_t)c ? 1.f : -1.f; pb[c] = lb == (int64_t)c ? 1.f : -1.f; }
    float* o0 = out + ((b * 2 + 0) * HW + hw) * 8;
    float* o1 = out + ((b * 2 + 1) * HW + hw) * 8;
    lp_st4(o0, make_float4(ya, yb, ya - yb, pb[0]));
    lp_st4(o0 + 4, make_float4(pb[1], pb[2], pb[3], pb[4]));
    lp_st4(o1, make_float4(yb, ya, yb - ya, pa[0]));
    lp_st4(o1 + 4, make_float4(pa[1], pa[2], pa[3], pa[4]));
    tgt[(b * 2 + 0) * HW + hw] = la;
    tgt[(b * 2 + 1) * HW + hw] = lb;
  }
}

static inline int lp_grid(const rcv_handle* h, size_t pixels, int per_cu) {
  size_t g = (pixels + 255) / 256;
  const size_t cap = (size_t)h->num_cus * per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// Every refusal that depends on the SHAPE of a record sits in front of the `query` return (what rcv_op_workspace / the planner
// accepts, the launch accepts); only operand pointers and workspace row counts are checked after it.
int rcv_launch_lp_tail(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const bool fwd = op->kind == RCV_OP_LP_TAIL_FWD, with_ce = (op->flags & RCV_F_FUSED_CE) != 0;
  const int mode2 = op->i[RCV_I_AUX0], rch = op->i[RCV_I_AUX1], stats = op->i[RCV_I_STATS];
  const char* what = fwd ? "labelprop tail" : "labelprop tail backward";
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; }
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W * LP_CIN < 2147483647.0, "%s: shape %d x %d x %d unsupported", what, N, H, W);
  RCV_CHECK_ARG(Cin == LP_CIN && Cout >= 1 && Cout <= LP_MAX_OUT, "%s: %d -> %d channels unsupported (16 input channels, 1..%d classes)", what,
                Cin, Cout, LP_MAX_OUT);
  RCV_CHECK_ARG(op->flags & RCV_F_FUSED_UP, "%s: the input is formed from the decoder block's stored tensors (RCV_F_FUSED_UP expected)", what);
  RCV_CHECK_ARG(rch >= 4 && rch <= LP_CIN && rch % 4 == 0, "%s: %d skip channels unsupported (a multiple of 4, at most %d)", what, rch, LP_CIN);
  RCV_CHECK_ARG(mode2 == RCV_LOAD_PLAIN || mode2 == RCV_LOAD_AFFINE || mode2 == RCV_LOAD_AFFINE_RELU, "%s: skip load mode %d unsupported", what, mode2);
  RCV_CHECK_ARG(fwd ? stats == RCV_STATS_NONE : stats == RCV_STATS_BWD_DEC,
                "%s: statistics kind %d (the backward owes the decoder block its RCV_STATS_BWD_DEC rows, the forward writes none)", what, stats);
  const int g = lp_grid(h, (size_t)N * H * W, 4);      // one partial row per workgroup; the grid of RCV_OP_CE_FWD / RCV_OP_CLS_BWD
  const size_t wrow = (size_t)Cout * LP_CIN + Cout;
  if (query) {
    if (fwd) {
      snprintf(query->label, sizeof(query->label), "lp_tail_fwd<%d>", with_ce ? 1 : 0);
      if (with_ce) { query->n_part = g; query->part_bytes = (size_t)g * 3 * sizeof(float); }
    } else {
      snprintf(query->label, sizeof(query->label), "lp_tail_bwd<%d,%d>", Cout, with_ce ? 1 : 0);
      query->n_part = g;
      query->part_bytes = (size_t)g * (2 * LP_CIN + wrow) * sizeof(float);      // statistics rows [g][2][16], then filter + bias rows
    }
    return RCV_OK;
  }
  const float* r = (const float*)op->p[RCV_P_X3]; const float* rc = (const float*)op->p[RCV_P_X4];
  const int64_t* tgt = (const int64_t*)op->p[RCV_P_IN2]; const float* cw = (const float*)op->p[RCV_P_X0];
  RCV_CHECK_ARG(r && (mode2 == RCV_LOAD_PLAIN || rc) && op->p[RCV_P_W] && op->p[RCV_P_OUT], "%s: null operand", what);
  if (fwd) {
    RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN_C], "%s: null operand", what);
    float* part = (float*)op->p[RCV_P_PART];
    if (with_ce) {
      RCV_CHECK_ARG(tgt && part && op->p[RCV_P_X1], "%s + cross entropy: needs target, workspace, loss_out", what);
      RCV_CHECK_ARG(op->i[RCV_I_NPART] == g, "%s + cross entropy: workspace rows %d != %d", what, op->i[RCV_I_NPART], g);
    }
    hipLaunchKernelGGL(with_ce ? lp_tail_fwd_kernel<true> : lp_tail_fwd_kernel<false>, dim3(g), dim3(256), 0, s, (const float*)op->p[RCV_P_IN],
                       (const float*)op->p[RCV_P_W], (const float*)op->p[RCV_P_BIAS], (float*)op->p[RCV_P_OUT], N, H * W, Cout,
                       (const float*)op->p[RCV_P_IN_C], r, rc, mode2, rch, tgt, cw, part, (uint8_t*)op->p[RCV_P_X2]);
    RCV_HIP(hipGetLastError());
    if (with_ce) return rcv_enqueue_ce_finalize(part, g, (float*)op->p[RCV_P_X1], s);
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN2] && op->p[RCV_P_PART] && op->p[RCV_P_X1] && op->p[RCV_P_EPI_AUX] && op->p[RCV_P_EPI_C] && op->p[RCV_P_IN_AUX],
                "%s: null operand (p[RCV_P_IN_AUX] = the skip gradient)", what);
  RCV_CHECK_ARG(op->i[RCV_I_NPART] == g, "%s: workspace rows %d != %d", what, op->i[RCV_I_NPART], g);
  RCV_CHECK_ARG(!with_ce || (op->p[RCV_P_X5] && op->p[RCV_P_IN2_AUX]), "%s + cross entropy: loss_out / d loss missing", what);
  float* stat_part = (float*)op->p[RCV_P_PART];
  float* w_part = stat_part + (size_t)g * 2 * LP_CIN;
  const lp_bwd_fn kern = with_ce ? lp_bwd_pick<true>(Cout) : lp_bwd_pick<false>(Cout);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, s, (const float*)op->p[RCV_P_EPI_AUX], with_ce ? nullptr : (const float*)op->p[RCV_P_IN2],
                     (const float*)op->p[RCV_P_W], (float*)op->p[RCV_P_OUT], (float*)op->p[RCV_P_IN_AUX], (const float*)op->p[RCV_P_EPI_C],
                     stat_part, w_part, N, H * W, r, rc, mode2, rch, tgt, cw, (const float*)op->p[RCV_P_BIAS], (const float*)op->p[RCV_P_X5],
                     (const float*)op->p[RCV_P_IN2_AUX]);
  RCV_HIP(hipGetLastError());
  // dW -> p[X1] ([Cout][16]), db -> p[X2]
  return rcv_enqueue_rows_reduce(w_part, g, (int)wrow, (float*)op->p[RCV_P_X1], Cout * LP_CIN, (float*)op->p[RCV_P_X2], s);
}

int rcv_launch_lp_batch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_CIN], nClass = op->i[RCV_I_COUT];
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "lp_batch"); }
  RCV_CHECK_ARG(nClass == 5, "labelprop batch: %d classes unsupported (the network's first conv reads 3 + 5 channels)", nClass);
  RCV_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && (double)B * 2.0 * H * W * (C > 8 ? C : 8) < 2147483647.0,
                "labelprop batch: shape %d x 2 x %d x %d x %d unsupported", B, C, H, W);
  if (query) return RCV_OK;
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT] && op->p[RCV_P_X0], "labelprop batch: null operand");
  const int g = lp_grid(h, (size_t)B * H * W, 8);
  hipLaunchKernelGGL(lp_batch_kernel, dim3(g), dim3(256), 0, s, (const float*)op->p[RCV_P_IN], (const int64_t*)op->p[RCV_P_IN2],
                     (float*)op->p[RCV_P_OUT], (int64_t*)op->p[RCV_P_X0], B, C, H * W);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
