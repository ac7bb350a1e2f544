// RCV_OP_CLS_PROBA (rcv_cls_proba): the softmax form of the classifier tails -- the [softmax] section that closes every net.cfg of the
// robot-side export, and the confidence gate of a pseudo-label (makeLPImages.py writes the arg-max of a prediction as the next
// training target; the loss ignores a target outside [0, C)).  The inference tail of RCV_OP_CLS_LABEL (cls_label.hip) with other
// outputs: source forms 0 (features through the 1x1 classifier, 8 channels a lane per pixel, 16 channels four lanes per pixel, with
// and without RCV_F_FUSED_UP) and 1 (padded NHWC logits of the 3x3 / 5x5 classifier), slot for slot; the logits are formed by the
// expressions of cls_common.h and of cls_label.hip's kernels, so they are bit for bit the logits RCV_OP_CLS_FWD / RCV_OP_NHWC_TO_NCHW
// store.  No logits are stored here.
//
// Arithmetic, fixed as the contract (the one lp_input.hip states for its soft prior; its lines stand in cls_softmax.h, shared with
// cls_calib.hip):
//   m = the first maximum of z in class order (`z_c > m` from -inf; a NaN never wins), cls = its index,
//   e_c = expf(z_c - m),  S = ((e_0 + e_1) + e_2) + ... in class order,  p_c = e_c / S with an IEEE division; no fast intrinsics.
// Outputs, each optional (a NULL slot is not written), at least one required:
//   p[X0]  probabilities fp32 NCHW [N][C][H][W]
//   p[OUT] class map uint8 [N][H][W], bit for bit RCV_OP_CLS_LABEL's
//   p[X1]  confidence fp32 [N][H][W] = p[cls] (the very float stored in p[X0])
//   p[X2]  pseudo-label int64 [N][H][W] = cls if confidence >= f[0], else -100; the comparison runs on the stored fp32 confidence
// NaN: a NaN logit gives whatever the expressions give -- e_c of that class is NaN, so are S and every probability of the pixel; the
// class stays the first maximum of the other logits (class 0 when all are NaN), a NaN confidence passes no threshold (-100), and a
// NaN threshold passes nothing.  Not part of the tested contract.
//
// Shape.  The grid-stride loop of cls_label.hip: every lane of a wave runs every iteration, a pixel index past the end is clamped for
// the loads and masked for the stores.  Probabilities leave per class plane: with a lane per pixel one store instruction covers 64
// neighbouring pixels of one plane (256 contiguous bytes); with four lanes per pixel lane q of the four stores the classes q and
// q + 4, so one instruction covers 16 neighbouring pixels (64 contiguous bytes) of four planes, and 5 classes leave in two
// instructions.  Class bytes, confidences and pseudo-labels leave from the lane that owns the pixel, coalesced along pixels.  No LDS
// beyond the classifier's filter, no atomics; every output element is written once by a fixed lane: deterministic.
#include "cls_softmax.h"

struct CpOut {
  float* prob;          // [N][C][H][W] or NULL
  uint8_t* lab;         // [N][H][W] or NULL
  float* conf;          // [N][H][W] or NULL
  long long* pseudo;    // [N][H][W] or NULL
  float thr;
  uint32_t HW;
};

// The tail of one pixel.  LPP = lanes per pixel (1 or 4; with 4 every lane of the four holds all logits), q = this lane's index among
// them, p = its pixel (< 2^31), valid = p < total.
template <int LPP>
__device__ __forceinline__ void cp_tail(const CpOut& o, const float (&lg)[CLS_MAX_OUT], int COUT, uint32_t p, bool valid, int q) {
  CLS_SOFTMAX(lg, COUT, pr, am, cf)          // float pr[], int am, float cf (cls_softmax.h)
  if (!valid) return;
  if (o.prob) {
    const uint32_t n = p / o.HW, hw = p - n * o.HW;
    float* base = o.prob + (size_t)n * COUT * o.HW + hw;
    if (LPP == 1) {
#pragma unroll
      for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < COUT) base[(size_t)c * o.HW] = pr[c];
    } else {
#pragma unroll
      for (int j = 0; j < CLS_MAX_OUT / 4; ++j) {
        const int c = q + 4 * j;
        float v = pr[4 * j];
#pragma unroll
        for (int k = 1; k < 4; ++k) if (q == k) v = pr[4 * j + k];
        if (c < COUT) base[(size_t)c * o.HW] = v;
      }
    }
  }
  if (LPP == 1 || q == 0) {
    if (o.lab) o.lab[p] = (uint8_t)am;
    if (o.conf) o.conf[p] = cf;
    if (o.pseudo) o.pseudo[p] = cf >= o.thr ? (long long)am : -100ll;
  }
}

// ---- form 0, 8 input channels: a lane per pixel (the logits of cls_label8_kernel)
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_proba8_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         uint32_t total, int COUT, const float* __restrict__ tc, const float* __restrict__ r,
                                                         const float* __restrict__ rc, int mode2, int rch, CpOut o) {
  constexpr int CIN = 8;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  for (int e = threadIdx.x; e < COUT * CIN; e += blockDim.x) ws[e] = w[e];
  for (int e = threadIdx.x; e < COUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = bias ? bias[e] : 0.f;
  __syncthreads();
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
    cp_tail<1>(o, lg, COUT, (uint32_t)p, valid, 0);
  }
}

// ---- form 0, 16 input channels (LabelProp): four lanes per pixel, the butterfly of cls_label16_kernel
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_proba16_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          uint32_t total, int COUT, const float* __restrict__ tc, const float* __restrict__ r,
                                                          const float* __restrict__ rc, int mode2, int rch, CpOut o) {
  constexpr int CIN = 16;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  for (int e = threadIdx.x; e < CLS_MAX_OUT * CIN; e += blockDim.x) ws[e] = e < COUT * CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < CLS_MAX_OUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = (bias && e < COUT) ? bias[e] : 0.f;
  __syncthreads();
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
    float4 a = sld4(x + pl * CIN + 4 * q);
    if (FUSED) {
      a.x = fmaxf(fmaf(a.x, s.x, h.x), 0.f); a.y = fmaxf(fmaf(a.y, s.y, h.y), 0.f);
      a.z = fmaxf(fmaf(a.z, s.z, h.z), 0.f); a.w = fmaxf(fmaf(a.w, s.w, h.w), 0.f);
      if (has_skip) {
        float4 b = sld4(r + pl * rch + 4 * q);
        if (mode2 != RCV_LOAD_PLAIN) {
          b.x = fmaf(b.x, s2.x, h2.x); b.y = fmaf(b.y, s2.y, h2.y); b.z = fmaf(b.z, s2.z, h2.z); b.w = fmaf(b.w, s2.w, h2.w);
          if (mode2 == RCV_LOAD_AFFINE_RELU) { b.x = fmaxf(b.x, 0.f); b.y = fmaxf(b.y, 0.f); b.z = fmaxf(b.z, 0.f); b.w = fmaxf(b.w, 0.f); }
        }
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
    }
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) {
      const float* wc = ws + c * CIN + 4 * q;
      float u = fmaf(a.x, wc[0], fmaf(a.y, wc[1], fmaf(a.z, wc[2], a.w * wc[3])));
      u += __shfl_xor(u, 1);
      u += __shfl_xor(u, 2);
      lg[c] = u + ws[CLS_MAX_OUT * CIN + c];
    }
    cp_tail<4>(o, lg, COUT, (uint32_t)p, valid, q);
  }
}

// ---- form 1: NHWC logits, CP floats per pixel; logit c = x[p][c] + bias[c], as logit_label_kernel
__global__ __launch_bounds__(256) void logit_proba_kernel(const float* __restrict__ x, const float* __restrict__ bias, uint32_t total, int CP, int COUT,
                                                          CpOut o) {
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
    cp_tail<1>(o, lg, COUT, (uint32_t)p, valid, 0);
  }
}

// Every refusal that depends on the shape of the record sits in front of the `query` return; pointers are checked at launch.
int rcv_launch_cls_proba(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int form = op->i[RCV_I_INMODE];
  const bool fused = (op->flags & RCV_F_FUSED_UP) != 0;
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "cls_proba"); }
  RCV_CHECK_ARG(form == 0 || form == 1, "class probabilities: source form %d unknown (0 = features, 1 = logits)", form);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W < 2147483648.0,
                "class probabilities: %d x %d x %d pixels: every size must be >= 1 and N*H*W < 2^31", N, H, W);
  RCV_CHECK_ARG(Cout >= 1 && Cout <= CLS_MAX_OUT, "class probabilities: %d classes unsupported (1..%d)", Cout, CLS_MAX_OUT);
  const int mode2 = op->i[RCV_I_AUX0];
  int rch = Cin;
  if (form == 0) {
    RCV_CHECK_ARG(Cin == 8 || Cin == 16, "class probabilities from features: %d input channels unsupported (8 or 16)", Cin);
    if (fused) {
      if (op->i[RCV_I_AUX1] != 0) rch = op->i[RCV_I_AUX1];
      RCV_CHECK_ARG(rch % 4 == 0 && rch >= 4 && rch <= Cin, "class probabilities from features (fused decoder output): %d skip channels for %d inputs",
                    rch, Cin);
      RCV_CHECK_ARG(mode2 == RCV_LOAD_PLAIN || mode2 == RCV_LOAD_AFFINE || mode2 == RCV_LOAD_AFFINE_RELU,
                    "class probabilities from features: skip load mode %d", mode2);
    }
  } else {
    RCV_CHECK_ARG(!fused, "class probabilities: RCV_F_FUSED_UP belongs to source form 0 (features)");
    RCV_CHECK_ARG(Cin >= Cout && Cin % 4 == 0, "class probabilities from logits: %d floats per pixel for %d classes (a multiple of 4, >= the classes)",
                  Cin, Cout);
  }
  if (query) return RCV_OK;

  const float* x = (const float*)op->p[RCV_P_IN]; const float* w = (const float*)op->p[RCV_P_W]; const float* bias = (const float*)op->p[RCV_P_BIAS];
  const float* tc = (const float*)op->p[RCV_P_IN_C]; const float* r = (const float*)op->p[RCV_P_X3]; const float* rc = (const float*)op->p[RCV_P_X4];
  CpOut o;
  o.prob = (float*)op->p[RCV_P_X0]; o.lab = (uint8_t*)op->p[RCV_P_OUT]; o.conf = (float*)op->p[RCV_P_X1]; o.pseudo = (long long*)op->p[RCV_P_X2];
  o.thr = op->f[0]; o.HW = (uint32_t)H * (uint32_t)W;
  RCV_CHECK_ARG(x, "class probabilities: null input");
  RCV_CHECK_ARG(o.prob || o.lab || o.conf || o.pseudo,
                "class probabilities: no output (p[X0] probabilities, p[OUT] class map, p[X1] confidence, p[X2] pseudo-label: at least one)");
  if (form == 0) RCV_CHECK_ARG(w, "class probabilities from features: null classifier weight");
  if (fused) RCV_CHECK_ARG(tc && r && (mode2 == RCV_LOAD_PLAIN || rc), "class probabilities from features (fused decoder output): operands missing");
  const size_t total = (size_t)N * H * W;
  // cls_label.hip's grid: at most 4 workgroups per CU, 256 or 64 pixels per workgroup and sweep
  const int per_wg = (form == 0 && Cin == 16) ? 64 : 256;
  size_t g = (total + per_wg - 1) / per_wg;
  const size_t cap = (size_t)h->num_cus * 4;
  if (g > cap) g = cap;
  const dim3 grid((unsigned)g), block(256);
  const uint32_t tot = (uint32_t)total;
  if (form == 1) hipLaunchKernelGGL(logit_proba_kernel, grid, block, 0, s, x, bias, tot, Cin, Cout, o);
  else if (Cin == 16 && fused) hipLaunchKernelGGL((cls_proba16_kernel<true>), grid, block, 0, s, x, w, bias, tot, Cout, tc, r, rc, mode2, rch, o);
  else if (Cin == 16) hipLaunchKernelGGL((cls_proba16_kernel<false>), grid, block, 0, s, x, w, bias, tot, Cout, tc, r, rc, mode2, rch, o);
  else if (fused) hipLaunchKernelGGL((cls_proba8_kernel<true>), grid, block, 0, s, x, w, bias, tot, Cout, tc, r, rc, mode2, rch, o);
  else hipLaunchKernelGGL((cls_proba8_kernel<false>), grid, block, 0, s, x, w, bias, tot, Cout, tc, r, rc, mode2, rch, o);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
