// RCV_OP_CLS_CALIB (rcv_cls_calib): the calibration form of the classifier tails -- what a confidence threshold keeps.  The tail of
// RCV_OP_CLS_PROBA (cls_proba.hip) with a count in place of every store: per pixel the class, its softmax confidence and the label
// give one bin of a table predicted class x label x confidence bin, from which the host derives, for every threshold of a sweep at
// once, how many pixels of each class survive, how many of those are right, what they are confused with and whether the confidence
// means anything.  Nothing per pixel is stored.
//
// Source forms 0 (features through the 1x1 classifier, 8 channels a lane per pixel, 16 channels four lanes per pixel, with and without
// RCV_F_FUSED_UP) and 1 (padded NHWC logits) slot for slot as RCV_OP_CLS_PROBA; the logits are formed by the expressions of
// cls_proba.hip's kernels and class and confidence by cls_softmax.h, so the confidence binned here is bit for bit the float
// RCV_OP_CLS_PROBA stores.  Form 2: a stored uint8 class map p[IN] plus a stored fp32 confidence map p[X1] (maps from elsewhere).
//
// Contract, per pixel with class cls, fp32 confidence cf, target t (int64, p[IN2] or NULL), edges fp32[K] in p[X0], K = i[COUNT]:
//   bin = #{ j : cf >= edges[j] } -- a count of K comparisons, so it lies in [0, K] whatever the edges hold; the comparison is the one
//         RCV_OP_CLS_PROBA's pseudo-label gate makes on the stored float
//   q   = (uint32)(cf * 2^26): the product is exact in fp32 and the conversion truncates (cf <= 0 gives 0, cf >= 64 saturates)
//   0 <= t < C (decided on the int64):  state[bin][cls][t] += 1,  state[bin][cls][C + 1] += q
//   otherwise (or no targets):          state[bin][cls][C] += 1,  state[bin][cls][C + 2] += q
//   a NaN confidence counts nowhere; in form 2 neither does a class byte >= C.
// state: int64 [K + 1][C][C + 3] in p[X2], accumulated.  Every sum is an integer sum: a pass is bitwise reproducible whatever the order
// of the atomics, and no fold record is needed.
//
// Shape.  cls_proba.hip's grid and loop (at most 4 workgroups per CU, 256 or 64 pixels per sweep, clamped loads, masked counts).  A
// workgroup keeps the whole table in LDS as 64-bit words for its entire loop (33 * 8 * 11 * 8 = 23232 bytes at K = 32, C = 8), adds
// with LDS integer atomics and at the end adds its non-zero entries to the state with 64-bit global integer atomics.
#include "cls_softmax.h"

#define CC_MAX_EDGES 32
#define CC_TABLE ((CC_MAX_EDGES + 1) * CLS_MAX_OUT * (CLS_MAX_OUT + 3))
#define CC_SCALE 67108864.f            /* 2^26 */

struct CcArgs {
  const int64_t* target;               // int64[N][H][W] or NULL
  const float* edges;                  // fp32[K]
  unsigned long long* state;           // int64[K + 1][C][C + 3], accumulated (two's complement: the unsigned add is the signed one)
  int K, COUT;
};

// table and edges of the workgroup; every thread calls this (ends in a barrier)
__device__ __forceinline__ void cc_init(unsigned long long* __restrict__ tab, float* __restrict__ eds, const CcArgs& a) {
  const int n = (a.K + 1) * a.COUT * (a.COUT + 3);
  for (int e = threadIdx.x; e < n; e += blockDim.x) tab[e] = 0ull;
  if ((int)threadIdx.x < CC_MAX_EDGES) eds[threadIdx.x] = (int)threadIdx.x < a.K ? a.edges[threadIdx.x] : INFINITY;
  __syncthreads();
}

// one pixel's counts; mine: this lane owns pixel p (< total)
__device__ __forceinline__ void cc_count(unsigned long long* __restrict__ tab, const float* __restrict__ eds, const CcArgs& a, size_t p, bool mine,
                                         int am, float cf) {
  if (!mine || !(cf == cf) || am >= a.COUT) return;
  int bin = 0;
#pragma unroll 8
  for (int j = 0; j < a.K; ++j) bin += cf >= eds[j] ? 1 : 0;          // a.K <= CC_MAX_EDGES: bin <= K
  const int64_t t = a.target ? a.target[p] : -1;
  const bool lab = t >= 0 && t < (int64_t)a.COUT;                      // the int64 decides: 2^32 + c is no class
  const int C = a.COUT;
  const uint32_t q = cf <= 0.f ? 0u : (cf >= 64.f ? 0xFFFFFFFFu : (uint32_t)(cf * CC_SCALE));
  const int row = (bin * C + am) * (C + 3);
  const int cnt = row + (lab ? (int)t : C), sum = row + (lab ? C + 1 : C + 2);
  // plain LDS adds: combining the equal entries of a wave first (ballot on the entry, one add through the first lane) measured
  // 5-25 % slower on spread and on single-bin confidences alike
  atomicAdd(&tab[cnt], 1ull);
  atomicAdd(&tab[sum], (unsigned long long)q);
}

// table -> state (the non-zero entries); every thread calls this
__device__ __forceinline__ void cc_flush(const unsigned long long* __restrict__ tab, const CcArgs& a) {
  __syncthreads();
  const int n = (a.K + 1) * a.COUT * (a.COUT + 3);
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const unsigned long long v = tab[e];
    if (v) atomicAdd(&a.state[e], v);
  }
}

// ---- form 0, 8 input channels: a lane per pixel (the logits of cls_proba8_kernel)
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_calib8_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         uint32_t total, const float* __restrict__ tc, const float* __restrict__ r,
                                                         const float* __restrict__ rc, int mode2, int rch, CcArgs a) {
  constexpr int CIN = 8;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ unsigned long long tab[CC_TABLE];
  __shared__ float eds[CC_MAX_EDGES];
  const int COUT = a.COUT;
  for (int e = threadIdx.x; e < COUT * CIN; e += blockDim.x) ws[e] = w[e];
  for (int e = threadIdx.x; e < COUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = bias ? bias[e] : 0.f;
  cc_init(tab, eds, a);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    float v[CIN];
    cls_load_up<CIN, FUSED>(v, x, tc, r, rc, mode2, valid ? p : (size_t)total - 1, rch);
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) {
      lg[c] = 0.f;
      if (c < COUT) {
        float u = ws[CLS_MAX_OUT * CIN + c];
#pragma unroll
        for (int k = 0; k < CIN; ++k) u = fmaf(v[k], ws[c * CIN + k], u);
        lg[c] = u;
      }
    }
    CLS_SOFTMAX(lg, COUT, pr, am, cf)          // float pr[], int am, float cf (cls_softmax.h)
    cc_count(tab, eds, a, p, valid, am, cf);
  }
  cc_flush(tab, a);
}

// ---- form 0, 16 input channels (LabelProp): four lanes per pixel, the butterfly of cls_proba16_kernel; lane 0 of the four owns the pixel
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_calib16_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          uint32_t total, const float* __restrict__ tc, const float* __restrict__ r,
                                                          const float* __restrict__ rc, int mode2, int rch, CcArgs a) {
  constexpr int CIN = 16;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ unsigned long long tab[CC_TABLE];
  __shared__ float eds[CC_MAX_EDGES];
  const int COUT = a.COUT;
  for (int e = threadIdx.x; e < CLS_MAX_OUT * CIN; e += blockDim.x) ws[e] = e < COUT * CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < CLS_MAX_OUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = (bias && e < COUT) ? bias[e] : 0.f;
  cc_init(tab, eds, a);
  const int q = threadIdx.x & 3;
  float4 s = make_float4(1.f, 1.f, 1.f, 1.f), h = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s, h2 = h;
  if (FUSED) {
    s = sld4(tc + 4 * q); h = sld4(tc + CIN + 4 * q);
    if (4 * q < rch && mode2 != RCV_LOAD_PLAIN) { s2 = sld4(rc + 4 * q); h2 = sld4(rc + rch + 4 * q); }
  }
  const bool has_skip = FUSED && 4 * q < rch;
  const size_t stride = (size_t)gridDim.x * 64;
  for (size_t p0 = (size_t)blockIdx.x * 64; p0 < total; p0 += stride) {
    const size_t p = p0 + (threadIdx.x >> 2);
    const bool valid = p < total;
    const size_t pl = valid ? p : (size_t)total - 1;
    float4 f = sld4(x + pl * CIN + 4 * q);
    if (FUSED) {
      f.x = fmaxf(fmaf(f.x, s.x, h.x), 0.f); f.y = fmaxf(fmaf(f.y, s.y, h.y), 0.f);
      f.z = fmaxf(fmaf(f.z, s.z, h.z), 0.f); f.w = fmaxf(fmaf(f.w, s.w, h.w), 0.f);
      if (has_skip) {
        float4 b = sld4(r + pl * rch + 4 * q);
        if (mode2 != RCV_LOAD_PLAIN) {
          b.x = fmaf(b.x, s2.x, h2.x); b.y = fmaf(b.y, s2.y, h2.y); b.z = fmaf(b.z, s2.z, h2.z); b.w = fmaf(b.w, s2.w, h2.w);
          if (mode2 == RCV_LOAD_AFFINE_RELU) { b.x = fmaxf(b.x, 0.f); b.y = fmaxf(b.y, 0.f); b.z = fmaxf(b.z, 0.f); b.w = fmaxf(b.w, 0.f); }
        }
        f.x += b.x; f.y += b.y; f.z += b.z; f.w += b.w;
      }
    }
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) {
      const float* wc = ws + c * CIN + 4 * q;
      float u = fmaf(f.x, wc[0], fmaf(f.y, wc[1], fmaf(f.z, wc[2], f.w * wc[3])));
      u += __shfl_xor(u, 1);
      u += __shfl_xor(u, 2);
      lg[c] = u + ws[CLS_MAX_OUT * CIN + c];
    }
    CLS_SOFTMAX(lg, COUT, pr, am, cf)          // float pr[], int am, float cf (cls_softmax.h)
    cc_count(tab, eds, a, p, valid && q == 0, am, cf);
  }
  cc_flush(tab, a);
}

// ---- form 1: NHWC logits, CP floats per pixel; logit c = x[p][c] + bias[c], as logit_proba_kernel
__global__ __launch_bounds__(256) void logit_calib_kernel(const float* __restrict__ x, const float* __restrict__ bias, uint32_t total, int CP, CcArgs a) {
  __shared__ unsigned long long tab[CC_TABLE];
  __shared__ float eds[CC_MAX_EDGES];
  const int COUT = a.COUT;
  cc_init(tab, eds, a);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    const float* px = x + (valid ? p : (size_t)total - 1) * CP;
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int q = 0; q < CLS_MAX_OUT / 4; ++q) {
      lg[4 * q] = lg[4 * q + 1] = lg[4 * q + 2] = lg[4 * q + 3] = 0.f;
      if (4 * q < COUT) {                      // (COUT <= CP and CP % 4 == 0: the vector stays inside the pixel)
        const float4 u = sld4_nt(px + 4 * q);
        lg[4 * q] = u.x; lg[4 * q + 1] = u.y; lg[4 * q + 2] = u.z; lg[4 * q + 3] = u.w;
      }
    }
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < COUT) lg[c] = lg[c] + (bias ? bias[c] : 0.f);
    CLS_SOFTMAX(lg, COUT, pr, am, cf)          // float pr[], int am, float cf (cls_softmax.h)
    cc_count(tab, eds, a, p, valid, am, cf);
  }
  cc_flush(tab, a);
}

// ---- form 2: a stored uint8 class map and a stored fp32 confidence map
__global__ __launch_bounds__(256) void map_calib_kernel(const uint8_t* __restrict__ cm, const float* __restrict__ conf, uint32_t total, CcArgs a) {
  __shared__ unsigned long long tab[CC_TABLE];
  __shared__ float eds[CC_MAX_EDGES];
  cc_init(tab, eds, a);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    const size_t pl = valid ? p : (size_t)total - 1;
    cc_count(tab, eds, a, p, valid, (int)cm[pl], conf[pl]);
  }
  cc_flush(tab, a);
}

// Every refusal that depends on the shape of the record sits in front of the `query` return; pointers are checked at launch.
int rcv_launch_cls_calib(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int form = op->i[RCV_I_INMODE], K = op->i[RCV_I_COUNT];
  const bool fused = (op->flags & RCV_F_FUSED_UP) != 0;
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "cls_calib"); }
  RCV_CHECK_ARG(form >= 0 && form <= 2, "calibration counts: source form %d unknown (0 = features, 1 = logits, 2 = class map + confidence map)", form);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W < 2147483648.0,
                "calibration counts: %d x %d x %d pixels: every size must be >= 1 and N*H*W < 2^31", N, H, W);
  RCV_CHECK_ARG(Cout >= 1 && Cout <= CLS_MAX_OUT, "calibration counts: %d classes unsupported (1..%d)", Cout, CLS_MAX_OUT);
  RCV_CHECK_ARG(K >= 1 && K <= CC_MAX_EDGES, "calibration counts: %d confidence edges in i[COUNT] (1..%d)", K, CC_MAX_EDGES);
  const int mode2 = op->i[RCV_I_AUX0];
  int rch = Cin;
  if (form == 0) {
    RCV_CHECK_ARG(Cin == 8 || Cin == 16, "calibration counts from features: %d input channels unsupported (8 or 16)", Cin);
    if (fused) {
      if (op->i[RCV_I_AUX1] != 0) rch = op->i[RCV_I_AUX1];
      RCV_CHECK_ARG(rch % 4 == 0 && rch >= 4 && rch <= Cin, "calibration counts from features (fused decoder output): %d skip channels for %d inputs",
                    rch, Cin);
      RCV_CHECK_ARG(mode2 == RCV_LOAD_PLAIN || mode2 == RCV_LOAD_AFFINE || mode2 == RCV_LOAD_AFFINE_RELU,
                    "calibration counts from features: skip load mode %d", mode2);
    }
  } else {
    RCV_CHECK_ARG(!fused, "calibration counts: RCV_F_FUSED_UP belongs to source form 0 (features)");
    if (form == 1)
      RCV_CHECK_ARG(Cin >= Cout && Cin % 4 == 0, "calibration counts from logits: %d floats per pixel for %d classes (a multiple of 4, >= the classes)",
                    Cin, Cout);
  }
  if (query) return RCV_OK;

  const float* x = (const float*)op->p[RCV_P_IN]; const float* w = (const float*)op->p[RCV_P_W]; const float* bias = (const float*)op->p[RCV_P_BIAS];
  const float* tc = (const float*)op->p[RCV_P_IN_C]; const float* r = (const float*)op->p[RCV_P_X3]; const float* rc = (const float*)op->p[RCV_P_X4];
  const float* conf = (const float*)op->p[RCV_P_X1];
  CcArgs a;
  a.target = (const int64_t*)op->p[RCV_P_IN2]; a.edges = (const float*)op->p[RCV_P_X0]; a.state = (unsigned long long*)op->p[RCV_P_X2];
  a.K = K; a.COUT = Cout;
  RCV_CHECK_ARG(x, "calibration counts: null input");
  RCV_CHECK_ARG(a.edges, "calibration counts: null edges (p[X0]: fp32[%d] in device memory)", K);
  RCV_CHECK_ARG(a.state, "calibration counts: null state (p[X2]: int64[%d][%d][%d])", K + 1, Cout, Cout + 3);
  if (form == 0) RCV_CHECK_ARG(w, "calibration counts from features: null classifier weight");
  if (form == 2) RCV_CHECK_ARG(conf, "calibration counts from a class map: null confidence map (p[X1]: fp32[N][H][W])");
  if (fused) RCV_CHECK_ARG(tc && r && (mode2 == RCV_LOAD_PLAIN || rc), "calibration counts from features (fused decoder output): operands missing");
  const size_t total = (size_t)N * H * W;
  // cls_proba.hip's grid: at most 4 workgroups per CU, 256 or 64 pixels per workgroup and sweep
  const int per_wg = (form == 0 && Cin == 16) ? 64 : 256;
  size_t g = (total + per_wg - 1) / per_wg;
  const size_t cap = (size_t)h->num_cus * 4;
  if (g > cap) g = cap;
  const dim3 grid((unsigned)g), block(256);
  const uint32_t tot = (uint32_t)total;
  if (form == 2) hipLaunchKernelGGL(map_calib_kernel, grid, block, 0, s, (const uint8_t*)op->p[RCV_P_IN], conf, tot, a);
  else if (form == 1) hipLaunchKernelGGL(logit_calib_kernel, grid, block, 0, s, x, bias, tot, Cin, a);
  else if (Cin == 16 && fused) hipLaunchKernelGGL((cls_calib16_kernel<true>), grid, block, 0, s, x, w, bias, tot, tc, r, rc, mode2, rch, a);
  else if (Cin == 16) hipLaunchKernelGGL((cls_calib16_kernel<false>), grid, block, 0, s, x, w, bias, tot, tc, r, rc, mode2, rch, a);
  else if (fused) hipLaunchKernelGGL((cls_calib8_kernel<true>), grid, block, 0, s, x, w, bias, tot, tc, r, rc, mode2, rch, a);
  else hipLaunchKernelGGL((cls_calib8_kernel<false>), grid, block, 0, s, x, w, bias, tot, tc, r, rc, mode2, rch, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
