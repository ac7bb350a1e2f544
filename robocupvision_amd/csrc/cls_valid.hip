// RCV_OP_CLS_VALID (rcv_cls_valid) and RCV_OP_VALID_FOLD (rcv_valid_fold): the validation form of the classifier tails -- valid() of
// train.py:97-178 (trainer.py, labelPropTrain.py, pruner.py alike): `pred = model(imgs)`, `criterion(pred, targets)`, `torch.max(pred, 1)`
// and the mask loops that count (pred, label) pairs per image.  The class, the loss terms and the confusion bin of a pixel are all
// taken from its logits while they are in registers: no logits are stored, the targets are read once.
//
// Source forms as RCV_OP_CLS_LABEL (cls_label.hip): 0 = features through the 1x1 classifier (8 channels: a lane per pixel; 16 channels:
// four lanes per pixel), 1 = the padded NHWC logits of the 3x3 / 5x5 classifier, and 2 = a uint8 class map (counts only, no loss).
//
// Logits: the very expressions of cls_fwd_kernel / cls_fwd16_kernel / nhwc_to_nchw_kernel (cls_common.h; explicit fmaf chains, the same
// butterfly), so the class is bit for bit `predict`'s.  Loss: ce_first_max, ce_target_logit, ce_pixel_sums (ce_common.h), per-thread
// sums in double, rows through ce_store_row.  The lane-per-pixel forms keep ce_fwd_kernel's grid (reduce_grid over the pixels,
// 256 per workgroup), its pixel -> thread mapping and its summation order: their rows are bit for bit the rows RCV_OP_CE_FWD writes from
// the logits RCV_OP_CLS_FWD / RCV_OP_NHWC_TO_NCHW store.  A target outside [0, C) -- decided on the int64 value -- has weight 0 and
// counts in no bin.
//
// Counts: an LDS histogram per workgroup holds the bins of ONE image; a sweep (256 or 64 consecutive pixels) walks the images it
// touches in index order and flushes the histogram to counts[image] (integer atomics: order independent) whenever it moves on.
#include "cls_common.h"
#include "ce_common.h"

#define CV_BINS (CLS_MAX_OUT * CLS_MAX_OUT)
#define CV_STATE 76                      /* doubles of the running state (rcv.h RCV_OP_VALID_FOLD) */

// hist -> counts[cur] (the non-zero bins), hist cleared; every thread of the workgroup calls this
__device__ __forceinline__ void cv_flush(int* __restrict__ hist, long long cur, int* __restrict__ counts, int C) {
  __syncthreads();                                   // every add to the image that ends here has landed
  if (cur >= 0 && (int)threadIdx.x < C * C) {
    const int v = hist[threadIdx.x];
    if (v) { atomicAdd(&counts[(size_t)cur * C * C + threadIdx.x], v); hist[threadIdx.x] = 0; }
  }
  __syncthreads();
}

// One sweep's counts: pixels [p0, min(p0 + span, total)) -- p0, span uniform over the workgroup -- belong to images p0 / HW ..; `mine`:
// this lane owns pixel p of the sweep, am / t = its class and label.  cur: the image the histogram holds (-1: none), uniform.
__device__ __forceinline__ void cv_count(int* __restrict__ hist, long long& cur, int* __restrict__ counts, int C, size_t p0, int span, size_t total,
                                         size_t HW, size_t p, bool mine, int am, int64_t t) {
  const size_t end = p0 + span < total ? p0 + span : total;
  const size_t n0 = p0 / HW, n1 = (end - 1) / HW;
  const bool in = mine && am < C && t >= 0 && t < (int64_t)C;
  const int bin = in ? am * C + (int)t : 0;
  for (size_t n = n0; n <= n1; ++n) {
    if ((long long)n != cur) { cv_flush(hist, cur, counts, C); cur = (long long)n; }
    const size_t lo = n * HW;
    if (in && p >= lo && p - lo < HW) atomicAdd(&hist[bin], 1);
  }
}

// one pixel's loss terms from its logits (the body of cls_fwd_kernel<.., CE>); returns the class
__device__ __forceinline__ int cv_pixel_loss(const float (&lg)[CLS_MAX_OUT], int COUT, int64_t t, const float* __restrict__ cw, double& a_nll,
                                             double& a_w, double& a_ok) {
  int am;
  const float mx = ce_first_max(lg, COUT, am);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < COUT) se += expf(lg[c] - mx);
  const int tg = (t >= 0 && t < (int64_t)COUT) ? (int)t : -1;          // the int64 decides: 2^32 + c is no class
  ce_pixel_sums(mx, ce_target_logit(lg, COUT, tg), se, am, tg, COUT, cw, a_nll, a_w, a_ok);
  return am;
}

struct CvArgs {
  const int64_t* target;     // int64[N][H][W]
  const float* cw;           // class weights or NULL
  float* part;               // float[gridDim.x][3]
  int* counts;               // int32[N][C][C], accumulated
  uint8_t* lab;              // uint8[N][H][W] or NULL
  size_t total, HW;
  int COUT;
};

// ---- form 0, 8 input channels: a lane per pixel (cls_fwd_kernel<8, FUSED, true> without its stores)
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_valid8_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ tc, const float* __restrict__ r, const float* __restrict__ rc,
                                                         int mode2, int rch, CvArgs a) {
  constexpr int CIN = 8;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ int hist[CV_BINS];
  const int COUT = a.COUT;
  for (int e = threadIdx.x; e < COUT * CIN; e += blockDim.x) ws[e] = w[e];
  for (int e = threadIdx.x; e < COUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = bias ? bias[e] : 0.f;
  if (threadIdx.x < CV_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  double a_nll = 0.0, a_w = 0.0, a_ok = 0.0;
  long long cur = -1;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < a.total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < a.total;
    float v[CIN];
    cls_load_up<CIN, FUSED>(v, x, tc, r, rc, mode2, valid ? p : a.total - 1, rch);
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
    int am = 0;
    int64_t t = -1;
    if (valid) {
      t = a.target[p];
      am = cv_pixel_loss(lg, COUT, t, a.cw, a_nll, a_w, a_ok);
      if (a.lab) __builtin_nontemporal_store((uint8_t)am, a.lab + p);
    }
    cv_count(hist, cur, a.counts, COUT, p0, 256, a.total, a.HW, p, valid, am, t);
  }
  cv_flush(hist, cur, a.counts, COUT);
  ce_store_row(a_nll, a_w, a_ok, a.part + (size_t)blockIdx.x * 3);
}

// ---- form 0, 16 input channels (LabelProp): four lanes per pixel (cls_fwd16_kernel's loads and butterfly); lane 0 of the four owns the pixel
template <bool FUSED>
__global__ __launch_bounds__(256) void cls_valid16_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ tc, const float* __restrict__ r, const float* __restrict__ rc,
                                                          int mode2, int rch, CvArgs a) {
  constexpr int CIN = 16;
  __shared__ float ws[CLS_MAX_OUT * CIN + CLS_MAX_OUT];
  __shared__ int hist[CV_BINS];
  const int COUT = a.COUT;
  for (int e = threadIdx.x; e < CLS_MAX_OUT * CIN; e += blockDim.x) ws[e] = e < COUT * CIN ? w[e] : 0.f;
  for (int e = threadIdx.x; e < CLS_MAX_OUT; e += blockDim.x) ws[CLS_MAX_OUT * CIN + e] = (bias && e < COUT) ? bias[e] : 0.f;
  if (threadIdx.x < CV_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int q = threadIdx.x & 3;
  float4 s = make_float4(1.f, 1.f, 1.f, 1.f), h = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s, h2 = h;
  if (FUSED) {
    s = sld4(tc + 4 * q); h = sld4(tc + CIN + 4 * q);
    if (4 * q < rch && mode2 != RCV_LOAD_PLAIN) { s2 = sld4(rc + 4 * q); h2 = sld4(rc + rch + 4 * q); }
  }
  const bool has_skip = FUSED && 4 * q < rch;
  double a_nll = 0.0, a_w = 0.0, a_ok = 0.0;
  long long cur = -1;
  const size_t stride = (size_t)gridDim.x * 64;
  for (size_t p0 = (size_t)blockIdx.x * 64; p0 < a.total; p0 += stride) {
    const size_t p = p0 + (threadIdx.x >> 2);
    const bool valid = p < a.total;
    const size_t pl = valid ? p : a.total - 1;
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
    const bool mine = valid && q == 0;
    int am = 0;
    int64_t t = -1;
    if (mine) {
      t = a.target[p];
      am = cv_pixel_loss(lg, COUT, t, a.cw, a_nll, a_w, a_ok);
      if (a.lab) __builtin_nontemporal_store((uint8_t)am, a.lab + p);
    }
    cv_count(hist, cur, a.counts, COUT, p0, 64, a.total, a.HW, p, mine, am, t);
  }
  cv_flush(hist, cur, a.counts, COUT);
  ce_store_row(a_nll, a_w, a_ok, a.part + (size_t)blockIdx.x * 3);
}

// ---- form 1: NHWC logits, CP floats per pixel (the 3x3 / 5x5 classifier's padded output); logit c = x[p][c] + bias[c], as nhwc_to_nchw_kernel
__global__ __launch_bounds__(256) void logit_valid_kernel(const float* __restrict__ x, const float* __restrict__ bias, int CP, CvArgs a) {
  __shared__ int hist[CV_BINS];
  const int COUT = a.COUT;
  if (threadIdx.x < CV_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  double a_nll = 0.0, a_w = 0.0, a_ok = 0.0;
  long long cur = -1;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < a.total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < a.total;
    const float* px = x + (valid ? p : a.total - 1) * CP;
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
    int am = 0;
    int64_t t = -1;
    if (valid) {
      t = a.target[p];
      am = cv_pixel_loss(lg, COUT, t, a.cw, a_nll, a_w, a_ok);
      if (a.lab) __builtin_nontemporal_store((uint8_t)am, a.lab + p);
    }
    cv_count(hist, cur, a.counts, COUT, p0, 256, a.total, a.HW, p, valid, am, t);
  }
  cv_flush(hist, cur, a.counts, COUT);
  ce_store_row(a_nll, a_w, a_ok, a.part + (size_t)blockIdx.x * 3);
}

// ---- form 2: a uint8 class map -> counts only (the Dice route: the criterion has formed the loss and the map already)
__global__ __launch_bounds__(256) void map_valid_kernel(const uint8_t* __restrict__ cm, CvArgs a) {
  __shared__ int hist[CV_BINS];
  if (threadIdx.x < CV_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  long long cur = -1;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p0 = (size_t)blockIdx.x * 256; p0 < a.total; p0 += stride) {
    const size_t p = p0 + threadIdx.x;
    const bool valid = p < a.total;
    int am = 0;
    int64_t t = -1;
    if (valid) {
      am = cm[p];
      t = a.target[p];
    }
    cv_count(hist, cur, a.counts, a.COUT, p0, 256, a.total, a.HW, p, valid, am, t);
  }
  cv_flush(hist, cur, a.counts, a.COUT);
}

// ---- RCV_OP_VALID_FOLD: one workgroup of 256 threads folds a batch into the state and clears the counts it read
__global__ __launch_bounds__(256) void valid_fold_kernel(int* __restrict__ counts, const float* __restrict__ part, int n_part,
                                                         const float* __restrict__ loss_scalar, int N, double pixels, int C,
                                                         double* __restrict__ state) {
  __shared__ float s_loss[4];
  __shared__ double s_term[256];
  __shared__ long long s_conf[4][CV_BINS];
  const int tid = threadIdx.x;
  const int CC = C * C;
  // the fp32 batch loss: the rows in ce_finalize_kernel's order, or the criterion's own scalar
  if (n_part > 0) {
    ce_finalize_body(part, n_part, s_loss);
    __syncthreads();
  }
  if (tid == 0) {
    state[0] += (double)(n_part > 0 ? s_loss[0] : loss_scalar[0]);
    state[1] += 1.0;
    state[2] += (double)N;
    state[3] += pixels;
  }
  // iou_sum[c]: the terms of `per` images at a time, a thread per (image, class); then a thread per class adds them in image order
  const int per = 256 / C;
  double acc = tid < C ? state[4 + tid] : 0.0;
  for (int nb = 0; nb < N; nb += per) {
    const int n = nb + tid / C, c = tid % C;
    if (tid < per * C && n < N) {
      const int* cn = counts + (size_t)n * CC;
      long long row = 0, col = 0;
      for (int l = 0; l < C; ++l) { row += cn[c * C + l]; col += cn[l * C + c]; }
      const long long inter = cn[c * C + c], uni = row + col - inter;
      s_term[tid] = uni == 0 ? 1.0 : (double)inter / (double)uni;          // train.py:148-153
    }
    __syncthreads();
    if (tid < C) {
      const int m = N - nb < per ? N - nb : per;
      for (int j = 0; j < m; ++j) acc += s_term[j * C + tid];
    }
    __syncthreads();
  }
  if (tid < C) state[4 + tid] = acc;
  // conf[pred][label] += sum over the images (integers: exact in any order); state rows of 8
  {
    const int e = tid & (CV_BINS - 1), lane4 = tid >> 6;
    long long sum = 0;
    if (e < CC) for (int n = lane4; n < N; n += 4) sum += counts[(size_t)n * CC + e];
    s_conf[lane4][e] = sum;
    __syncthreads();
    if (tid < CC) {
      const long long tot = s_conf[0][tid] + s_conf[1][tid] + s_conf[2][tid] + s_conf[3][tid];
      state[12 + (tid / C) * 8 + (tid % C)] += (double)tot;
    }
    __syncthreads();           // every read of the counts is done
  }
  for (size_t i = tid; i < (size_t)N * CC; i += 256) counts[i] = 0;
}

// Every refusal that depends on the shape of the record sits in front of the `query` return; pointers are checked at launch.
int rcv_launch_cls_valid(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int form = op->i[RCV_I_INMODE];
  const bool fused = (op->flags & RCV_F_FUSED_UP) != 0;
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "cls_valid"); }
  RCV_CHECK_ARG(form >= 0 && form <= 2, "validation tail: source form %d unknown (0 = features, 1 = logits, 2 = class map)", form);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W < 2147483648.0,
                "validation tail: %d x %d x %d pixels: every size must be >= 1 and N*H*W < 2^31", N, H, W);
  RCV_CHECK_ARG(Cout >= 1 && Cout <= CLS_MAX_OUT, "validation tail: %d classes unsupported (1..%d)", Cout, CLS_MAX_OUT);
  const int mode2 = op->i[RCV_I_AUX0];
  int rch = Cin;
  if (form == 0) {
    RCV_CHECK_ARG(Cin == 8 || Cin == 16, "validation tail from features: %d input channels unsupported (8 or 16)", Cin);
    if (fused) {
      if (op->i[RCV_I_AUX1] != 0) rch = op->i[RCV_I_AUX1];
      RCV_CHECK_ARG(rch % 4 == 0 && rch >= 4 && rch <= Cin, "validation tail from features (fused decoder output): %d skip channels for %d inputs", rch, Cin);
      RCV_CHECK_ARG(mode2 == RCV_LOAD_PLAIN || mode2 == RCV_LOAD_AFFINE || mode2 == RCV_LOAD_AFFINE_RELU, "validation tail from features: skip load mode %d", mode2);
    }
  } else {
    RCV_CHECK_ARG(!fused, "validation tail: RCV_F_FUSED_UP belongs to source form 0 (features)");
    if (form == 1)
      RCV_CHECK_ARG(Cin >= Cout && Cin % 4 == 0, "validation tail from logits: %d floats per pixel for %d classes (a multiple of 4, >= the classes)", Cin, Cout);
    else
      RCV_CHECK_ARG(!op->p[RCV_P_PART] && op->i[RCV_I_NPART] == 0,
                    "validation tail from a class map: no loss is formed, so no partial rows (p[PART] NULL, i[NPART] 0)");
  }
  const size_t total = (size_t)N * H * W;
  const int per_wg = (form == 0 && Cin == 16) ? 64 : 256;          // pixels per workgroup and sweep
  const int g = reduce_grid(h, total, per_wg);                     // (256: the grid of RCV_OP_CE_FWD, one partial row per workgroup)
  if (query) {
    if (form != 2) { query->n_part = g; query->part_bytes = (size_t)g * 3 * sizeof(float); }
    return RCV_OK;
  }

  const float* x = (const float*)op->p[RCV_P_IN]; const float* w = (const float*)op->p[RCV_P_W]; const float* bias = (const float*)op->p[RCV_P_BIAS];
  const float* tc = (const float*)op->p[RCV_P_IN_C]; const float* r = (const float*)op->p[RCV_P_X3]; const float* rc = (const float*)op->p[RCV_P_X4];
  CvArgs a;
  a.target = (const int64_t*)op->p[RCV_P_IN2]; a.cw = (const float*)op->p[RCV_P_X0]; a.part = (float*)op->p[RCV_P_PART];
  a.counts = (int*)op->p[RCV_P_X2]; a.lab = (uint8_t*)op->p[RCV_P_OUT]; a.total = total; a.HW = (size_t)H * W; a.COUT = Cout;
  RCV_CHECK_ARG(x && a.target && a.counts, "validation tail: null input, targets (int64[N][H][W]) or counts (int32[N][C][C])");
  if (form != 2) {
    RCV_CHECK_ARG(a.part, "validation tail: null partial rows (rcv_op_workspace)");
    RCV_CHECK_ARG(op->i[RCV_I_NPART] == g, "validation tail: workspace rows %d != %d", op->i[RCV_I_NPART], g);
  }
  if (form == 0) RCV_CHECK_ARG(w, "validation tail from features: null classifier weight");
  if (fused) RCV_CHECK_ARG(tc && r && (mode2 == RCV_LOAD_PLAIN || rc), "validation tail from features (fused decoder output): operands missing");
  const dim3 grid((unsigned)g), block(256);
  if (form == 2) hipLaunchKernelGGL(map_valid_kernel, grid, block, 0, s, (const uint8_t*)op->p[RCV_P_IN], a);
  else if (form == 1) hipLaunchKernelGGL(logit_valid_kernel, grid, block, 0, s, x, bias, Cin, a);
  else if (Cin == 16 && fused) hipLaunchKernelGGL((cls_valid16_kernel<true>), grid, block, 0, s, x, w, bias, tc, r, rc, mode2, rch, a);
  else if (Cin == 16) hipLaunchKernelGGL((cls_valid16_kernel<false>), grid, block, 0, s, x, w, bias, tc, r, rc, mode2, rch, a);
  else if (fused) hipLaunchKernelGGL((cls_valid8_kernel<true>), grid, block, 0, s, x, w, bias, tc, r, rc, mode2, rch, a);
  else hipLaunchKernelGGL((cls_valid8_kernel<false>), grid, block, 0, s, x, w, bias, tc, r, rc, mode2, rch, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

// The loss source is part of the record's shape: rows (p[IN2], i[NPART] > 0) or a scalar (p[X0], i[NPART] = 0), never both or neither.
int rcv_launch_valid_fold(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_COUT], n_part = op->i[RCV_I_NPART];
  if (query) { query->n_part = n_part; query->n_split = 0; query->part_bytes = 0; snprintf(query->label, sizeof(query->label), "valid_fold"); }
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W < 2147483648.0,
                "validation fold: %d x %d x %d pixels: every size must be >= 1 and N*H*W < 2^31", N, H, W);
  RCV_CHECK_ARG(C >= 1 && C <= CLS_MAX_OUT, "validation fold: %d classes unsupported (1..%d)", C, CLS_MAX_OUT);
  RCV_CHECK_ARG(n_part >= 0, "validation fold: %d partial rows", n_part);
  const bool rows = op->p[RCV_P_IN2] != nullptr, scalar = op->p[RCV_P_X0] != nullptr;
  RCV_CHECK_ARG(rows != scalar, "validation fold: exactly one loss source -- partial rows in p[IN2] or a device float in p[X0] (%s given)",
                rows ? "both" : "neither");
  RCV_CHECK_ARG(rows == (n_part > 0), "validation fold: %d partial rows with %s", n_part, rows ? "p[IN2] set" : "a scalar loss in p[X0]");
  if (query) return RCV_OK;
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_OUT], "validation fold: null counts (int32[N][C][C]) or state (double[%d])", CV_STATE);
  hipLaunchKernelGGL(valid_fold_kernel, dim3(1), dim3(256), 0, s, (int*)op->p[RCV_P_IN], (const float*)op->p[RCV_P_IN2], n_part,
                     (const float*)op->p[RCV_P_X0], N, (double)N * H * W, C, (double*)op->p[RCV_P_OUT]);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
