// Pooled patch-classification head of PB_FCN / PB_FCN_2 (model.py:255-266, 403-414; classTrainer.py:83,118-140):
//   pooled = pool(load(r))            max over k x k windows, stride k, floor (nn.MaxPool2d(k)), or the plane mean (AdaptiveAvgPool2d(1))
//   logits = W (pooled * drop) + b    optional Dropout2d keep-scale on the [N,C,1,1] vector, then the 1x1 classifier, NCHW out
// and its backward: dW / db, and d loss / d (loaded source value) scattered back over the plane (first arg-max of a max window, the
// plane for the mean), with the skip-gradient add and the BatchNorm-backward partial rows of the producer.
//
// Launches: forward ONE (a workgroup per pooled pixel pools the window, drops, classifies); backward TWO -- pool_cls_bwd_head_kernel
// (a workgroup per pooled pixel forms d loss / d pooled into the workspace, one more workgroup reduces dW / db over the pooled pixels
// in index order) and pool_cls_scatter_kernel (a grid-stride stream over the source plane, one work item per (pixel, channel quad):
// one 16-byte store of the gradient; r read where the arg-max or the statistics need it).  Fixed summation orders, no float atomics.
#include "rcv_internal.h"
#include "bn_sums.h"

#define POOL_CLS_MAX_OUT 8
#define POOL_CLS_MAX_C 512

__device__ __forceinline__ float4 pc_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void pc_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

template <int MODE>
__device__ __forceinline__ float4 pc_load(const float* p, float4 s, float4 h) {
  float4 v = pc_ld4(p);
  if (MODE != RCV_LOAD_PLAIN) {
    v.x = fmaf(v.x, s.x, h.x); v.y = fmaf(v.y, s.y, h.y); v.z = fmaf(v.z, s.z, h.z); v.w = fmaf(v.w, s.w, h.w);
    if (MODE == RCV_LOAD_AFFINE_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  }
  return v;
}

// k == 0: the whole plane (mean); k > 0: the k x k window of pooled pixel (py, px) (max)
// blockDim.x = G * C4 (G groups of threads, thread t owns quad t % C4 of window positions t / C4, t / C4 + G, ...): 256 threads for a
// max window, 1024 for the plane mean (one workgroup per image streams the whole plane: more loads in flight per workgroup)
template <int MODE>
__global__ __launch_bounds__(1024) void pool_cls_fwd_kernel(const float* __restrict__ r, const float* __restrict__ cst,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ drop, float* __restrict__ pooled,
                                                          float* __restrict__ logits, int H, int W, int C, int nC, int k, int Hp, int Wp) {
  __shared__ float4 red[1024];
  __shared__ float dots[POOL_CLS_MAX_OUT][POOL_CLS_MAX_C / 4];
  const int m = blockIdx.x;
  const int px = m % Wp, py = (m / Wp) % Hp, n = m / (Wp * Hp);
  const int C4 = C / 4, G = blockDim.x / C4;
  const int t = threadIdx.x, q = t % C4, gi = t / C4;
  const bool avg = k == 0;
  const int kh = avg ? H : k, kw = avg ? W : k, P = kh * kw;
  const int y0 = py * kh, x0 = px * kw;
  float4 s = make_float4(1.f, 1.f, 1.f, 1.f), h = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MODE != RCV_LOAD_PLAIN) { s = pc_ld4(cst + 4 * q); h = pc_ld4(cst + C + 4 * q); }
  // (fmaxf drops a NaN where aten's max_pool2d propagates it: the two differ on non-finite inputs only; the backward's arg-max rule matches)
  float4 acc = avg ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll 4
  for (int j = gi; j < P; j += G) {
    const int dy = j / kw, dx = j - dy * kw;
    const float4 v = pc_load<MODE>(r + (((size_t)n * H + y0 + dy) * W + x0 + dx) * C + 4 * q, s, h);
    if (avg) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
    else { acc.x = fmaxf(acc.x, v.x); acc.y = fmaxf(acc.y, v.y); acc.z = fmaxf(acc.z, v.z); acc.w = fmaxf(acc.w, v.w); }
  }
  red[t] = acc;
  __syncthreads();
  if (t < C4) {
    float4 a = red[t];
    for (int g = 1; g < G; ++g) {
      const float4 b = red[g * C4 + t];
      if (avg) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
      else { a.x = fmaxf(a.x, b.x); a.y = fmaxf(a.y, b.y); a.z = fmaxf(a.z, b.z); a.w = fmaxf(a.w, b.w); }
    }
    if (avg) { const float fp = (float)P; a.x /= fp; a.y /= fp; a.z /= fp; a.w /= fp; }
    pc_st4(pooled + (size_t)m * C + 4 * t, a);
    if (drop) {
      const float4 d = pc_ld4(drop + (size_t)n * C + 4 * t);
      a.x *= d.x; a.y *= d.y; a.z *= d.z; a.w *= d.w;
    }
    for (int o = 0; o < nC; ++o) {
      const float4 wv = pc_ld4(w + (size_t)o * C + 4 * t);
      dots[o][t] = fmaf(wv.w, a.w, fmaf(wv.z, a.z, fmaf(wv.y, a.y, wv.x * a.x)));
    }
  }
  __syncthreads();
  if (t < nC) {
    float z = 0.f;
    for (int qq = 0; qq < C4; ++qq) z += dots[t][qq];
    logits[((size_t)n * nC + t) * Hp * Wp + (size_t)py * Wp + px] = z + (bias ? bias[t] : 0.f);
  }
}

// blocks [0, M): dpool[m][c] = drop[n][c] * sum_o W[o][c] * dl[n][o][py][px]  (M = N * Hp * Wp pooled pixels)
// block M:       dW[o][c] = sum_m dl[m,o] * pooled[m][c] * drop[n(m)][c],  db[o] = sum_m dl[m,o]   (m ascending)
__global__ __launch_bounds__(256) void pool_cls_bwd_head_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                                               const float* __restrict__ drop, const float* __restrict__ pooled,
                                                               float* __restrict__ dpool, float* __restrict__ dw, float* __restrict__ db,
                                                               int M, int HWp, int C, int nC) {
  const int C4 = C / 4, t = threadIdx.x;
  if ((int)blockIdx.x < M) {
    const int m = blockIdx.x, n = m / HWp, pp = m - n * HWp;
    for (int qq = t; qq < C4; qq += blockDim.x) {
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int o = 0; o < nC; ++o) {
        const float d = dl[((size_t)n * nC + o) * HWp + pp];
        const float4 wv = pc_ld4(w + (size_t)o * C + 4 * qq);
        g.x = fmaf(wv.x, d, g.x); g.y = fmaf(wv.y, d, g.y); g.z = fmaf(wv.z, d, g.z); g.w = fmaf(wv.w, d, g.w);
      }
      if (drop) {
        const float4 dd = pc_ld4(drop + (size_t)n * C + 4 * qq);
        g.x *= dd.x; g.y *= dd.y; g.z *= dd.z; g.w *= dd.w;
      }
      pc_st4(dpool + (size_t)m * C + 4 * qq, g);
    }
    return;
  }
  for (int e = t; e < nC * C4; e += blockDim.x) {
    const int o = e / C4, qq = e - o * C4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int m = 0; m < M; ++m) {      // (unrolled: the loads of eight pooled pixels in flight; the sum stays in m order)
      const int n = m / HWp, pp = m - n * HWp;
      const float d = dl[((size_t)n * nC + o) * HWp + pp];
      float4 v = pc_ld4(pooled + (size_t)m * C + 4 * qq);
      if (drop) {
        const float4 dd = pc_ld4(drop + (size_t)n * C + 4 * qq);
        v.x *= dd.x; v.y *= dd.y; v.z *= dd.z; v.w *= dd.w;
      }
      a.x = fmaf(d, v.x, a.x); a.y = fmaf(d, v.y, a.y); a.z = fmaf(d, v.z, a.z); a.w = fmaf(d, v.w, a.w);
    }
    pc_st4(dw + (size_t)o * C + 4 * qq, a);
  }
  if (db && t < nC) {
    float a = 0.f;
#pragma unroll 8
    for (int m = 0; m < M; ++m) {
      const int n = m / HWp, pp = m - n * HWp;
      a += dl[((size_t)n * nC + t) * HWp + pp];
    }
    db[t] = a;
  }
}

// dy[n][y][x][c] = (pixel's share of dpool) (+ resid); the BatchNorm-backward partial rows of the producer as pool_bwd_kernel /
// bwd_stats_kernel write them: row 0 = sum v, row 1 = sum v * (e - mu) with v = dy (ENC) or dy * (e*c0 + c1 > 0) (DEC), e = the
// stored tensor (p[EPI_AUX]), c0 / c1 / mu = rows 0 / 1 / 2 of p[EPI_C].  Max: the gradient goes to the FIRST maximum of the window in
// row-major order (aten::max_pool2d_with_indices, pool_bwd_kernel; a strict '>' from -inf: a NaN is not propagated, see the forward),
// recomputed from r and the load constants (no stored indices); pixels outside every window get 0.  Every pixel of a window re-derives
// the window's arg-max: k*k loads per pixel, of which all but its own hit L1 / L2 (the window's other pixels are loaded by lanes of the
// same wave or workgroup at the same time).  Measured against one work item per (window, quad), which reads each value once: at the
// reference's size (bs 32, a 4x4x64 plane, k = 4) 9.2 us per pixel item vs 16.4 us per window item (rocprofv3 kernel averages; 16x
// fewer, 16x longer items leave most of the chip idle) -- the per-pixel form is kept.
// Mean: every pixel gets dpool / (H * W).  blockDim.x is a multiple of C4 (a thread keeps its channel quad).
template <int MODE>
__global__ __launch_bounds__(256) void pool_cls_scatter_kernel(const float* __restrict__ dpool, const float* __restrict__ r,
                                                              const float* __restrict__ cst, const float* __restrict__ resid,
                                                              const float* __restrict__ ec, float* __restrict__ dy, float* __restrict__ part,
                                                              int N, int H, int W, int C, int k, int Hp, int Wp, int stats) {
  __shared__ float4 sh4[2 * 256];
  const int C4 = C / 4;
  const int q = threadIdx.x % C4;
  const bool avg = k == 0;
  float4 s = make_float4(1.f, 1.f, 1.f, 1.f), h = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MODE != RCV_LOAD_PLAIN && !avg) { s = pc_ld4(cst + 4 * q); h = pc_ld4(cst + C + 4 * q); }
  float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0, mu = c0;
  if (stats == RCV_STATS_BWD_DEC) { c0 = pc_ld4(ec + 4 * q); c1 = pc_ld4(ec + C + 4 * q); }
  if (stats != RCV_STATS_NONE) mu = pc_ld4(ec + 2 * C + 4 * q);
  const float fp = (float)H * (float)W;
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  const size_t HW = (size_t)H * W, total = (size_t)N * HW * C4;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / C4;
    const int n = (int)(p / HW);
    const int yx = (int)(p - (size_t)n * HW);
    const int y = yx / W, x = yx - y * W;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (avg) {
      const float4 g = pc_ld4(dpool + (size_t)n * C + 4 * q);
      v = make_float4(g.x / fp, g.y / fp, g.z / fp, g.w / fp);
    } else {
      const int py = y / k, px = x / k;
      if (py < Hp && px < Wp) {
        const float4 g = pc_ld4(dpool + (((size_t)n * Hp + py) * Wp + px) * C + 4 * q);
        float bx = -INFINITY, by = -INFINITY, bz = -INFINITY, bw = -INFINITY;
        int ix = 0, iy = 0, iz = 0, iw = 0;
        const float* win = r + (((size_t)n * H + py * k) * W + px * k) * C + 4 * q;
        for (int j = 0; j < k * k; ++j) {
          const int dj = j / k;
          const float4 u = pc_load<MODE>(win + ((size_t)dj * W + (j - dj * k)) * C, s, h);
          if (u.x > bx) { bx = u.x; ix = j; }
          if (u.y > by) { by = u.y; iy = j; }
          if (u.z > bz) { bz = u.z; iz = j; }
          if (u.w > bw) { bw = u.w; iw = j; }
        }
        const int mine = (y - py * k) * k + (x - px * k);
        v = make_float4(ix == mine ? g.x : 0.f, iy == mine ? g.y : 0.f, iz == mine ? g.z : 0.f, iw == mine ? g.w : 0.f);
      }
    }
    if (resid) { const float4 rr = pc_ld4(resid + e * 4); v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w; }
    pc_st4(dy + e * 4, v);
    if (stats != RCV_STATS_NONE) {
      const float4 xr = pc_ld4(r + e * 4);
      if (stats == RCV_STATS_BWD_DEC) v = bn_relu_mask(v, xr, c0, c1);
      bn_sums_bwd_enc(a1, a2, v, xr, mu);
    }
  }
  if (stats != RCV_STATS_NONE) {
    sh4[threadIdx.x] = a1;
    sh4[blockDim.x + threadIdx.x] = a2;
    __syncthreads();
    if ((int)threadIdx.x < 2 * C4) {
      const int which = threadIdx.x / C4, qq = threadIdx.x % C4;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e = qq; e < (int)blockDim.x; e += C4) { const float4 v = sh4[which * blockDim.x + e]; u.x += v.x; u.y += v.y; u.z += v.z; u.w += v.w; }
      pc_st4(part + ((size_t)blockIdx.x * 2 + which) * C + 4 * qq, u);
    }
  }
}

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_POOL_CLS_FWD / RCV_OP_POOL_CLS_BWD).  Record:
//   i: N, H, W = source plane; CIN = C; COUT = nC; HO, WO = pooled plane (H / k, W / k; 1, 1 for the mean); AUX0 = k (2 or 4: max)
//      or 0 (mean); INMODE = load mode of r; STATS (backward) = RCV_STATS_NONE / BWD_ENC / BWD_DEC; NPART (filled by the query)
//   p: forward  -- IN = r, IN_C = its load constants, W = weight [nC][C][1][1], BIAS = bias [nC] or NULL, X0 = dropout keep-scale
//                  float[N][C] or NULL, X1 = pooled features [N][HO][WO][C] (out, before the dropout), OUT = logits [N][nC][HO][WO]
//      backward -- IN = d loss / d logits [N][nC][HO][WO], EPI_AUX = r (stored tensor: arg-max recompute, statistics), IN_C, W, X0,
//                  X1 as the forward, X2 = dW [nC][C] (out), X3 = db [nC] or NULL (out), OUT = d loss / d load(r) NHWC, RESID
//                  (RCV_F_RESID), EPI_C = producer constants (statistics), PART = workspace: NPART partial rows [2][C], then
//                  d loss / d pooled [N*HO*WO][C]
// Every refusal that depends on the shape of the record sits in front of the query return.
// --------------------------------------------------------------------------------------------
static inline int pool_cls_block(int C4, int threads = 256) { return (threads / C4) * C4; }
static inline int pool_cls_grid(const rcv_handle* h, size_t items, int block) {
  size_t g = (items + block - 1) / block;
  const size_t cap = (size_t)h->num_cus * 4;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

int rcv_launch_pool_cls(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const bool fwd = op->kind == RCV_OP_POOL_CLS_FWD;
  const char* what = fwd ? "pool_cls forward" : "pool_cls backward";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_CIN], nC = op->i[RCV_I_COUT];
  const int k = op->i[RCV_I_AUX0], mode = op->i[RCV_I_INMODE], stats = fwd ? RCV_STATS_NONE : op->i[RCV_I_STATS];
  RCV_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= POOL_CLS_MAX_C, "%s: %d channels unsupported (a multiple of 4, at most %d)", what, C, POOL_CLS_MAX_C);
  RCV_CHECK_ARG(nC >= 1 && nC <= POOL_CLS_MAX_OUT, "%s: %d classes unsupported (1..%d)", what, nC, POOL_CLS_MAX_OUT);
  RCV_CHECK_ARG(k == 0 || k == 2 || k == 4, "%s: pool kind %d unsupported (0 = plane mean, 2 / 4 = k x k max)", what, k);
  RCV_CHECK_ARG(mode == RCV_LOAD_PLAIN || mode == RCV_LOAD_AFFINE || mode == RCV_LOAD_AFFINE_RELU, "%s: load mode %d unsupported", what, mode);
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || stats == RCV_STATS_BWD_ENC || stats == RCV_STATS_BWD_DEC, "%s: statistics kind %d unsupported", what, stats);
  const uint32_t allowed = RCV_F_SIDE_STREAM | (fwd ? 0u : RCV_F_RESID);
  RCV_CHECK_ARG((op->flags & ~allowed) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~allowed);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W * C < 2147483647.0, "%s: plane %dx%dx%d (batch %d) out of range", what, H, W, C, N);
  const int Hp = k ? H / k : 1, Wp = k ? W / k : 1;
  RCV_CHECK_ARG(Hp >= 1 && Wp >= 1, "%s: a %dx%d plane holds no whole %dx%d window", what, H, W, k, k);
  RCV_CHECK_ARG(op->i[RCV_I_HO] == Hp && op->i[RCV_I_WO] == Wp, "%s: pooled plane %dx%d given, %dx%d expected", what, op->i[RCV_I_HO],
                op->i[RCV_I_WO], Hp, Wp);
  const int C4 = C / 4, block = pool_cls_block(C4), M = N * Hp * Wp;
  const int g = pool_cls_grid(h, (size_t)N * H * W * C4, block);
  const int n_part = stats != RCV_STATS_NONE ? g : 0;
  if (query) {
    const char* pk = k == 0 ? "avg" : (k == 2 ? "max2" : "max4");
    const char* md = mode == RCV_LOAD_PLAIN ? "plain" : (mode == RCV_LOAD_AFFINE ? "affine" : "affine_relu");
    if (fwd) snprintf(query->label, sizeof(query->label), "pool_cls_fwd<%s,%s>", pk, md);
    else {
      const char* st = stats == RCV_STATS_NONE ? "none" : (stats == RCV_STATS_BWD_ENC ? "enc" : "dec");
      snprintf(query->label, sizeof(query->label), "pool_cls_bwd<%s,%s,%s>", pk, md, st);
      query->n_part = n_part;
      query->part_bytes = ((size_t)n_part * 2 * C + (size_t)M * C) * sizeof(float);
    }
    return RCV_OK;
  }
  const float* cst = (const float*)op->p[RCV_P_IN_C];
  RCV_CHECK_ARG(mode == RCV_LOAD_PLAIN || cst, "%s: load constants missing", what);
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_W] && op->p[RCV_P_X1] && op->p[RCV_P_OUT], "%s: null operand", what);
  RCV_CHECK_ARG(((uintptr_t)op->p[RCV_P_W] & 15) == 0 && ((uintptr_t)op->p[RCV_P_X0] & 15) == 0, "%s: weight / dropout scale not 16-byte aligned", what);
  if (fwd) {
    auto kern = mode == RCV_LOAD_PLAIN ? pool_cls_fwd_kernel<RCV_LOAD_PLAIN>
                : (mode == RCV_LOAD_AFFINE ? pool_cls_fwd_kernel<RCV_LOAD_AFFINE> : pool_cls_fwd_kernel<RCV_LOAD_AFFINE_RELU>);
    hipLaunchKernelGGL(kern, dim3(M), dim3(k ? block : pool_cls_block(C4, 1024)), 0, s, (const float*)op->p[RCV_P_IN], cst, (const float*)op->p[RCV_P_W],
                       (const float*)op->p[RCV_P_BIAS], (const float*)op->p[RCV_P_X0], (float*)op->p[RCV_P_X1], (float*)op->p[RCV_P_OUT],
                       H, W, C, nC, k, Hp, Wp);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  const bool need_r = k != 0 || stats != RCV_STATS_NONE;
  RCV_CHECK_ARG(op->p[RCV_P_X2] && ((uintptr_t)op->p[RCV_P_X2] & 15) == 0, "%s: dW missing or not 16-byte aligned", what);
  RCV_CHECK_ARG(!need_r || op->p[RCV_P_EPI_AUX], "%s: source tensor (p[EPI_AUX]) missing", what);
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || op->p[RCV_P_EPI_C], "%s: producer constants (p[EPI_C]) missing", what);
  RCV_CHECK_ARG(op->p[RCV_P_PART] && op->i[RCV_I_NPART] == n_part, "%s: workspace missing or rows mismatch (%d given, %d expected)", what,
                op->i[RCV_I_NPART], n_part);
  const float* resid = (op->flags & RCV_F_RESID) ? (const float*)op->p[RCV_P_RESID] : nullptr;
  RCV_CHECK_ARG(!(op->flags & RCV_F_RESID) || resid, "%s: RCV_F_RESID without p[RESID]", what);
  float* part = (float*)op->p[RCV_P_PART];
  float* dpool = part + (size_t)n_part * 2 * C;
  hipLaunchKernelGGL(pool_cls_bwd_head_kernel, dim3(M + 1), dim3(256), 0, s, (const float*)op->p[RCV_P_IN], (const float*)op->p[RCV_P_W],
                     (const float*)op->p[RCV_P_X0], (const float*)op->p[RCV_P_X1], dpool, (float*)op->p[RCV_P_X2], (float*)op->p[RCV_P_X3],
                     M, Hp * Wp, C, nC);
  RCV_HIP(hipGetLastError());
  auto kern = mode == RCV_LOAD_PLAIN ? pool_cls_scatter_kernel<RCV_LOAD_PLAIN>
              : (mode == RCV_LOAD_AFFINE ? pool_cls_scatter_kernel<RCV_LOAD_AFFINE> : pool_cls_scatter_kernel<RCV_LOAD_AFFINE_RELU>);
  hipLaunchKernelGGL(kern, dim3(g), dim3(block), 0, s, (const float*)dpool, (const float*)op->p[RCV_P_EPI_AUX], cst, resid,
                     (const float*)op->p[RCV_P_EPI_C], (float*)op->p[RCV_P_OUT], part, N, H, W, C, k, Hp, Wp, stats);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
