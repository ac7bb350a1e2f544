// RCV_OP_CLS_LABEL (rcv_cls_label, rcv_colorize): the inference form of the classifier tails -- detect.py:131-133, and the mask loops of
// tester.py:142-153, makeLPImages.py:95-112, validLabelProp.py:133-144: `_, predClass = torch.max(pred, 1)` and Colorize
// (transform.py:158-170).  No logits are stored and no target is read: a pixel leaves as one class byte and, optionally, three
// colour bytes.  Source forms (rcv.h): 0 = features through the 1x1 classifier (8 channels: a lane per pixel; 16 channels: four lanes
// per pixel, as cls_fwd16_kernel), 1 = the padded NHWC logits of the 3x3 classifier, 2 = a class map (colour only).
//
// The logits of form 0 are formed by the very expressions of cls_fwd_kernel / cls_fwd16_kernel (cls_common.h; explicit fmaf chains,
// the same butterfly), and the class is the first maximum in class order (`lg[c] > mx` from -inf, the rule of cls_fwd_kernel's
// arg-max): the map is bit for bit the arg-max of the logits RCV_OP_CLS_FWD writes.  A NaN never passes `>`; all NaN -> class 0.
//
// Store shapes.  BYTE: the lane that owns a pixel stores one class byte and three colour bytes (a wave instruction covers 64 / 3 x 64
// strided bytes).  QUAD: the lanes of four neighbouring pixels exchange class and colour through the wave (ds_bpermute; the loads stay
// as they are, coalesced per pixel) and four of them store one dword each: the four classes, and the 12 colour bytes as three dwords.
// A group that crosses the end of the tensor, and operands that are not 4-byte aligned, take the byte stores.  Every lane of a wave
// runs every iteration (a pixel index past the end is clamped for the loads and masked for the stores), so the exchange never reads an
// inactive lane.  scripts/bench_detect.py times both shapes.
#include "cls_common.h"

#define CL_PAL 8                         /* palette rows */
/* store shape of a record that leaves the choice to the library (i[RCV_I_COUNT] = 0): the byte stores, until scripts/bench_detect.py
 * has been run on a card (its "tail" lines time both shapes) */
#define CL_DEFAULT_QUAD 0

// s_pal[k] = r | g << 8 | b << 16 of palette row k (LDS), filled by every kernel's prologue
__device__ __forceinline__ void cl_load_palette(uint32_t* s_pal, const uint8_t* __restrict__ pal) {
  if (threadIdx.x < CL_PAL)
    s_pal[threadIdx.x] = pal ? ((uint32_t)pal[3 * threadIdx.x] | ((uint32_t)pal[3 * threadIdx.x + 1] << 8) | ((uint32_t)pal[3 * threadIdx.x + 2] << 16)) : 0u;
}

// first maximum in class order; a NaN never wins (cls_fwd_kernel's rule)
__device__ __forceinline__ int cl_argmax(const float (&lg)[CLS_MAX_OUT], int COUT) {
  float mx = -INFINITY;
  int am = 0;
#pragma unroll
  for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < COUT && lg[c] > mx) { mx = lg[c]; am = c; }
  return am;
}

// Stores of one iteration.  LPP = lanes per pixel (1 or 4); every lane of the wave calls this with its pixel p (p % 4 == (lane / LPP) % 4:
// the launchers keep every stride a multiple of 4 pixels), valid = p < total, cls / rgb = its class and packed colour.
template <int LPP, bool QUAD>
__device__ __forceinline__ void cl_store(uint8_t* __restrict__ lab, uint8_t* __restrict__ col, size_t p, size_t total, bool valid, int cls, uint32_t rgb) {
  const int lane = threadIdx.x & 63;
  const bool owner = LPP == 1 || (lane & (LPP - 1)) == 0;
  bool bytes = valid && owner;
  if (QUAD) {
    const int g0 = lane & ~(4 * LPP - 1), gl = lane & (4 * LPP - 1);
    const uint32_t c0 = __shfl(rgb, g0), c1 = __shfl(rgb, g0 + LPP), c2 = __shfl(rgb, g0 + 2 * LPP), c3 = __shfl(rgb, g0 + 3 * LPP);
    const uint32_t word = (uint32_t)cls & 0xffu;
    const uint32_t l0 = __shfl(word, g0), l1 = __shfl(word, g0 + LPP), l2 = __shfl(word, g0 + 2 * LPP), l3 = __shfl(word, g0 + 3 * LPP);
    const size_t pb = p - (size_t)((lane / LPP) & 3);          // first pixel of this lane's group of four
    const bool full = pb + 3 < total;
    if (full) {
      bytes = false;
      if (gl == 3 && lab) __builtin_nontemporal_store(l0 | (l1 << 8) | (l2 << 16) | (l3 << 24), reinterpret_cast<uint32_t*>(lab + pb));
      if (gl < 3 && col) {
        // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        const uint32_t d = gl == 0 ? (c0 | (c1 << 24)) : gl == 1 ? ((c1 >> 8) | (c2 << 16)) : ((c2 >> 16) | (c3 << 8));
        __builtin_nontemporal_store(d, reinterpret_cast<uint32_t*>(col + 3 * pb) + gl);
      }
    }
  }
  if (bytes) {
    if (lab) __builtin_nontemporal_store((uint8_t)cls, lab + p);
    if (col) {
      __builtin_nontemporal_store((uint8_t)rgb, col + 3 * p);
      __builtin_nontemporal_store((uint8_t)(rgb >> 8), col + 3 * p + 1);
      __builtin_nontemporal_store((uint8_t)(rgb >> 16), col + 3 * p + 2);
    }
  }
}

// ---- form 0, 8 input channels: a lane per pixel (cls_fwd_kernel without its stores)
template <bool FUSED, bool QUAD>
__global__ __launch_bounds__(256) void cls_label8_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         size_t total, int COUT, const float* __restrict__ tc, const float* __restrict__ r,
                                                         const float* __restrict__ rc, int mode2, int rch, uint8_t* __restrict__ lab,
                                                         uint8_t* __restrict__ col, const uint8_t* __restrict__ pal) {
  constexpr int CIN = 8;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ uint32_t s_pal[CL_PAL];
  for (int e = threadIdx.x; e < COUT * CIN; e += blockDim.x) ws[e] = w[e];
  for (int e = threadIdx.x; e < COUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = bias ? bias[e] : 0.f;
  cl_load_palette(s_pal, pal);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    float v[CIN];
    cls_load_up<CIN, FUSED>(v, x, tc, r, rc, mode2, valid ? p : total - 1, rch);
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) {
      if (c < COUT) {
        float u = ws[CLS_MAX_OUT * CIN + c];
#pragma unroll
        for (int k = 0; k < CIN; ++k) u = fmaf(v[k], ws[c * CIN + k], u);
        lg[c] = u;
      }
    }
    const int am = cl_argmax(lg, COUT);
    cl_store<1, QUAD>(lab, col, p, total, valid, am, s_pal[am]);
  }
}

// ---- form 0, 16 input channels (LabelProp): four lanes per pixel; after the two butterfly steps every lane of the four holds all logits
template <bool FUSED, bool QUAD>
__global__ __launch_bounds__(256) void cls_label16_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          size_t total, int COUT, const float* __restrict__ tc, const float* __restrict__ r,
                                                          const float* __restrict__ rc, int mode2, int rch, uint8_t* __restrict__ lab,
                                                          uint8_t* __restrict__ col, const uint8_t* __restrict__ pal) {
  constexpr int CIN = 16;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ uint32_t s_pal[CL_PAL];
  for (int e = threadIdx.x; e < CLS_MAX_OUT * CIN; e += blockDim.x) ws[e] = e < COUT * CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < CLS_MAX_OUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = (bias && e < COUT) ? bias[e] : 0.f;
  cl_load_palette(s_pal, pal);
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
    const size_t pl = valid ? p : total - 1;
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
    const int am = cl_argmax(lg, COUT);
    cl_store<4, QUAD>(lab, col, p, total, valid, am, s_pal[am]);
  }
}

// ---- form 1: NHWC logits, CP floats per pixel (the 3x3 classifier's padded output); logit c = x[p][c] + bias[c], as nhwc_to_nchw_kernel
template <bool QUAD>
__global__ __launch_bounds__(256) void logit_label_kernel(const float* __restrict__ x, const float* __restrict__ bias, size_t total, int CP, int COUT,
                                                          uint8_t* __restrict__ lab, uint8_t* __restrict__ col, const uint8_t* __restrict__ pal) {
  __shared__ uint32_t s_pal[CL_PAL];
  cl_load_palette(s_pal, pal);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    const float* px = x + (valid ? p : total - 1) * CP;
    float lg[CLS_MAX_OUT];
#pragma unroll
    for (int q = 0; q < CLS_MAX_OUT / 4; ++q) {
      if (4 * q < COUT) {                      // (COUT <= CP and CP % 4 == 0: the vector stays inside the pixel)
        const float4 u = sld4_nt(px + 4 * q);
        lg[4 * q] = u.x; lg[4 * q + 1] = u.y; lg[4 * q + 2] = u.z; lg[4 * q + 3] = u.w;
      }
    }
#pragma unroll
    for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < COUT) lg[c] = lg[c] + (bias ? bias[c] : 0.f);
    const int am = cl_argmax(lg, COUT);
    cl_store<1, QUAD>(lab, col, p, total, valid, am, s_pal[am]);
  }
}

// ---- form 2: class map -> colour (transform.py:158-170); a class outside [0, 8) stays black
template <bool QUAD>
__global__ __launch_bounds__(256) void colorize_kernel(const void* __restrict__ cm, int elem_bytes, size_t total, uint8_t* __restrict__ col,
                                                       const uint8_t* __restrict__ pal) {
  __shared__ uint32_t s_pal[CL_PAL];
  cl_load_palette(s_pal, pal);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < total;
    const size_t pl = valid ? p : total - 1;
    const uint64_t v = elem_bytes == 1 ? (uint64_t)((const uint8_t*)cm)[pl] : (uint64_t)((const int64_t*)cm)[pl];
    const uint32_t rgb = v < (uint64_t)CL_PAL ? s_pal[(int)v] : 0u;
    cl_store<1, QUAD>(nullptr, col, p, total, valid, 0, rgb);
  }
}

// Every refusal that depends on the shape of the record sits in front of the `query` return; pointers are checked at launch.
int rcv_launch_cls_label(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int form = op->i[RCV_I_INMODE], shape = op->i[RCV_I_COUNT];
  const bool fused = (op->flags & RCV_F_FUSED_UP) != 0;
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "cls_label"); }
  RCV_CHECK_ARG(form >= 0 && form <= 2, "class map: source form %d unknown (0 = features, 1 = logits, 2 = class map)", form);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W < 2147483648.0, "class map: %d x %d x %d pixels: every size must be >= 1 and N*H*W < 2^31",
                N, H, W);
  RCV_CHECK_ARG(Cout >= 1 && Cout <= CLS_MAX_OUT, "class map: %d classes unsupported (1..%d)", Cout, CLS_MAX_OUT);
  RCV_CHECK_ARG(shape == 0 || shape == 1 || shape == 4, "class map: store shape %d unknown (0 = the library's choice, 1 = bytes, 4 = dwords of four pixels)", shape);
  const int mode2 = op->i[RCV_I_AUX0];
  int rch = Cin;
  if (form == 0) {
    RCV_CHECK_ARG(Cin == 8 || Cin == 16, "class map from features: %d input channels unsupported (8 or 16)", Cin);
    if (fused) {
      if (op->i[RCV_I_AUX1] != 0) rch = op->i[RCV_I_AUX1];
      RCV_CHECK_ARG(rch % 4 == 0 && rch >= 4 && rch <= Cin, "class map from features (fused decoder output): %d skip channels for %d inputs", rch, Cin);
      RCV_CHECK_ARG(mode2 == RCV_LOAD_PLAIN || mode2 == RCV_LOAD_AFFINE || mode2 == RCV_LOAD_AFFINE_RELU, "class map from features: skip load mode %d", mode2);
    }
  } else {
    RCV_CHECK_ARG(!fused, "class map: RCV_F_FUSED_UP belongs to source form 0 (features)");
    if (form == 1)
      RCV_CHECK_ARG(Cin >= Cout && Cin % 4 == 0, "class map from logits: %d floats per pixel for %d classes (a multiple of 4, >= the classes)", Cin, Cout);
    else
      RCV_CHECK_ARG(op->i[RCV_I_INMODE2] == 1 || op->i[RCV_I_INMODE2] == 8, "colour image: class map element size %d unsupported (1 = uint8, 8 = int64)",
                    op->i[RCV_I_INMODE2]);
  }
  RCV_CHECK_ARG(!op->p[RCV_P_X0] || op->p[RCV_P_X1], "class map: a colour image needs the palette (uint8[8][3], device memory)");
  if (query) return RCV_OK;

  const float* x = (const float*)op->p[RCV_P_IN]; const float* w = (const float*)op->p[RCV_P_W]; const float* bias = (const float*)op->p[RCV_P_BIAS];
  uint8_t* lab = (uint8_t*)op->p[RCV_P_OUT]; uint8_t* col = (uint8_t*)op->p[RCV_P_X0]; const uint8_t* pal = (const uint8_t*)op->p[RCV_P_X1];
  const float* tc = (const float*)op->p[RCV_P_IN_C]; const float* r = (const float*)op->p[RCV_P_X3]; const float* rc = (const float*)op->p[RCV_P_X4];
  RCV_CHECK_ARG(x, "class map: null input");
  if (form == 2) { RCV_CHECK_ARG(col, "colour image: null output"); lab = nullptr; }
  else RCV_CHECK_ARG(lab, "class map: null output (uint8[N][H][W])");
  if (form == 0) RCV_CHECK_ARG(w, "class map from features: null classifier weight");
  if (fused) RCV_CHECK_ARG(tc && r && (mode2 == RCV_LOAD_PLAIN || rc), "class map from features (fused decoder output): operands missing");
  const size_t total = (size_t)N * H * W;
  // the dword stores need 4-byte aligned outputs (a group of four pixels starts at a multiple of 4 pixels = 4 / 12 bytes)
  const bool aligned = (((uintptr_t)lab | (uintptr_t)col) & 3) == 0;
  const bool quad = aligned && (shape == 4 || (shape == 0 && CL_DEFAULT_QUAD));
  // at most 4 workgroups per CU; every stride is a multiple of 4 pixels (256 or 64 pixels per workgroup and sweep)
  const int per_wg = (form == 0 && Cin == 16) ? 64 : 256;
  size_t g = (total + per_wg - 1) / per_wg;
  const size_t cap = (size_t)h->num_cus * 4;
  if (g > cap) g = cap;
  const dim3 grid((unsigned)g), block(256);
#define CL_LAUNCH(K, ...)                                                          \
  do {                                                                             \
    if (quad) hipLaunchKernelGGL((K<true>), grid, block, 0, s, __VA_ARGS__);       \
    else hipLaunchKernelGGL((K<false>), grid, block, 0, s, __VA_ARGS__);           \
  } while (0)
#define CL_LAUNCH2(K, F, ...)                                                      \
  do {                                                                             \
    if (quad) hipLaunchKernelGGL((K<F, true>), grid, block, 0, s, __VA_ARGS__);    \
    else hipLaunchKernelGGL((K<F, false>), grid, block, 0, s, __VA_ARGS__);        \
  } while (0)
  if (form == 2) CL_LAUNCH(colorize_kernel, (const void*)x, op->i[RCV_I_INMODE2], total, col, pal);
  else if (form == 1) CL_LAUNCH(logit_label_kernel, x, bias, total, Cin, Cout, lab, col, pal);
  else if (Cin == 16 && fused) CL_LAUNCH2(cls_label16_kernel, true, x, w, bias, total, Cout, tc, r, rc, mode2, rch, lab, col, pal);
  else if (Cin == 16) CL_LAUNCH2(cls_label16_kernel, false, x, w, bias, total, Cout, tc, r, rc, mode2, rch, lab, col, pal);
  else if (fused) CL_LAUNCH2(cls_label8_kernel, true, x, w, bias, total, Cout, tc, r, rc, mode2, rch, lab, col, pal);
  else CL_LAUNCH2(cls_label8_kernel, false, x, w, bias, total, Cout, tc, r, rc, mode2, rch, lab, col, pal);
#undef CL_LAUNCH
#undef CL_LAUNCH2
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
