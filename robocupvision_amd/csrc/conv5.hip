// 5x5, stride-1, pad-2 convolution family of the classifier junction (model.py:256-267 Classifier(kernelSize=5), model.py:403-414
// UltClassifier(size=5)): forward, data gradient, filter + bias gradient, the 25-tap filter packer and the fixed-order reduction.
// fp32 on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain per output).  DESIGN.md 4.15.
//
//   RCV_OP_CONV5   D[co][pixel] += W[co][k] * X[k][pixel], k = (tap, ci): the mapping of conv_mfma.hip, so that every lane ends with four
//                  consecutive output channels of one pixel and the shared epilogue (conv_epilogue.h) applies unchanged.
//                  A = packed filter [25][CIN][16] in LDS (a wave reads 64 consecutive floats: no bank conflict),
//                  B = halo tile [(R+4)*(Wt+4)][CIN+2] in LDS (conv_xpitch: the 16 pixels x 2 k-lanes of a half-wave on 32 banks).
//                  One workgroup = 4 waves x 4 pixel blocks of 16 = one R x Wt = 256-pixel tile at a time; a workgroup walks the tiles
//                  blockIdx.x, + gridDim.x, ... with the filter staged once.
//   RCV_OP_WGRAD5  per tap D[co][ci] += G[co][pixel] * X[pixel + tap][ci]: K = pixels, four per MFMA; 25 accumulators and a
//                  pairwise sum of G per lane (the bias gradient).  The four waves of a workgroup are added in wave order
//                  through LDS; workgroup s writes partial row s.
#include "conv_common.h"
#include "conv_epilogue.h"

namespace {

constexpr int C5_TAPS = 25;
constexpr int C5_COLS = 16;                                 // columns of a packed filter (output channels of the record, zero padded)
constexpr int C5_CB = 8;                                    // pointwise (class) channels of the filter gradient = CLS3_PAD of the engine
constexpr int C5_ROW = C5_TAPS * C5_CB * C5_COLS + C5_CB;   // floats of one partial row: [25][8][16] then the bias gradient [8]
constexpr int C5_NT = 256;
constexpr int C5_XL = 12 * 36 * 18;                         // floats of the largest halo tile (8x32 tile, 16 channels; the 16x16 tile: 20 * 20 * 18)
static_assert(C5_XL >= 20 * 20 * 18 && C5_XL >= C5_TAPS * 256 + 4 * C5_CB, "the filter gradient's cross-wave sum [25][4][64] + bias rows [4][8] reuse the tile");

struct Tile5 {
  int R, Wt, tiles_x, tiles_y, IH, IW, ntiles;
};

Tile5 conv5_tiling(int N, int H, int W) {
  Tile5 t;
  t.Wt = W <= 16 ? 16 : 32;          // 16 | Wt: an MFMA pixel block never wraps a tile row
  t.R = 256 / t.Wt;
  t.tiles_x = ceil_div(W, t.Wt); t.tiles_y = ceil_div(H, t.R);
  t.IH = t.R + 4; t.IW = t.Wt + 4;
  t.ntiles = N * t.tiles_x * t.tiles_y;
  return t;
}

struct Wgrad5Args {
  const float* x;      // gathered operand NHWC [N][H][W][CA]
  const float* x_c;    // its load constants [5][CA]
  const float* g;      // pointwise operand NHWC [N][H][W][8]
  float* part;         // [nsplit][C5_ROW]
  int N, H, W, mode, flags;
  int R, Wt, tiles_x, tiles_y, IH, IW, ntiles;
  FastDiv fdWt, fdIW;
};

struct Reduce5Args {
  const float* part;
  float* dw;           // [COUT][CIN][5][5]
  float* db;           // [COUT] or NULL
  int nsplit, Cin, Cout;
};

struct Pack5Args {
  const float* src;    // [COUT][CIN][5][5]
  float* dst;          // [25][rows][16]
  int Cin, Cout, rows, flip;
};

// The (R+4) x (Wt+4) halo tile of all C channels -> xl[pixel][C + 2], through the load transform; taps outside the plane are zero
// AFTER the transform (stage_input of conv_mfma.hip, all channels in one pass)
template <int MODE, int C>
__device__ __forceinline__ void conv5_stage(const float* __restrict__ in, const float* cl, float* xl, int n, int oy0, int ox0, int H, int W,
                                            int IW, int npix, FastDiv fdIW, int tid) {
  constexpr int S = C + 2, Q = C / 4, STEP = C5_NT / Q, UNR = 4;
  const int q = tid % Q;
  float4 k[5];
  if (MODE != RCV_LOAD_PLAIN) {
#pragma unroll
    for (int j = 0; j < 5; ++j) k[j] = *reinterpret_cast<const float4*>(cl + j * C + 4 * q);
  }
  for (int pix0 = tid / Q; pix0 < npix; pix0 += UNR * STEP) {
    float4 x[UNR];
    bool ok[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int pix = pix0 + u * STEP;
      const int iy = fd_div(pix, fdIW), ix = pix - iy * IW;
      const int gy = oy0 + iy, gx = ox0 + ix;
      ok[u] = pix < npix && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok[u]) x[u] = ld4(in + ((size_t)(n * H + gy) * W + gx) * C + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int pix = pix0 + u * STEP;
      if (pix < npix) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) v = xform4<MODE>(x[u], v, k);
        float* d = xl + pix * S + 4 * q;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
  }
}

template <int CIN>
__global__ __launch_bounds__(C5_NT) void conv5_kernel(const ConvArgs a) {
  constexpr int S = CIN + 2, WN = 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wl = smem;                          // [25 * CIN][16]
  float* xl = wl + a.wl_floats;              // [IH * IW][S]
  float* cl = xl + a.xl_floats;              // [5][CIN]
  float* red = cl + 5 * CIN;                 // [4][2][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;

  if (a.in_mode != RCV_LOAD_PLAIN)
    for (int e = tid; e < 5 * CIN; e += C5_NT) cl[e] = a.in_c[e];
  for (int e = tid; e < C5_TAPS * CIN * (C5_COLS / 4); e += C5_NT)
    *reinterpret_cast<float4*>(wl + 4 * e) = ld4(a.w + 4 * e);

  int pixoff[WN];
#pragma unroll
  for (int b = 0; b < WN; ++b) {
    const int p = (wave * WN + b) * 16 + l15;
    const int ty = fd_div(p, a.fdWt), tx = p - ty * a.Wt;      // (R * Wt == 256: every p is a tile pixel)
    pixoff[b] = (ty * a.IW + tx) * S + l4;
  }
  const int aoff = l4 * C5_COLS + l15;
  const int npix = a.IH * a.IW;

  for (int t = blockIdx.x; t < a.total_tiles; t += gridDim.x) {
    TileInfo ti;
    int pt = t;
    ti.pt = t;
    const int tx_i = pt % a.tiles_x;
    pt /= a.tiles_x;
    const int ty_i = pt % a.tiles_y;
    ti.n = pt / a.tiles_y;
    ti.y0 = ty_i * a.R; ti.x0 = tx_i * a.Wt; ti.co0 = 0; ti.py = 0; ti.px = 0;
    ti.oy0 = ti.y0 - 2; ti.ox0 = ti.x0 - 2;
    __syncthreads();      // the previous tile's reads of xl / red; the first tile: cl is written
    with_load_mode<false>(a.in_mode, [&](auto mode) {
      conv5_stage<decltype(mode)::value, CIN>(a.in, cl, xl, ti.n, ti.oy0, ti.ox0, a.H, a.W, a.IW, npix, a.fdIW, tid);
    });
    __syncthreads();
    f32x4 acc[1][WN];
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[0][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const float* wj = wl + (dy * 5 + dx) * CIN * C5_COLS + aoff;
        const float* xj = xl + (dy * a.IW + dx) * S;
#pragma unroll
        for (int kk = 0; kk < CIN / 4; ++kk) {
          const float av = wj[kk * 4 * C5_COLS];
          float bv[WN];
#pragma unroll
          for (int b = 0; b < WN; ++b) bv[b] = xj[pixoff[b] + kk * 4];
#pragma unroll
          for (int b = 0; b < WN; ++b) acc[0][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[b], acc[0][b], 0, 0, 0);
        }
      }
    }
    conv_epilogue<1, WN, 1, 4, KIND_GATHER>(a, ti, acc, red, tid);
  }
}

template <int CA>
__global__ __launch_bounds__(C5_NT) void wgrad5_kernel(const Wgrad5Args a) {
  constexpr int S = CA + 2, KS = 16;       // k-steps (of four pixels) per wave and tile: 4 waves x 16 x 4 = 256 pixels
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xl = smem;                        // [IH * IW][S]; afterwards the cross-wave sum [25][4][64] and the bias rows [4][8]
  float* cl = smem + C5_XL;                // [5][CA]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;

  if (a.mode != RCV_LOAD_PLAIN)
    for (int e = tid; e < 5 * CA; e += C5_NT) cl[e] = a.x_c[e];

  int ty[KS], tx[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int p = (wave * KS + q) * 4 + l4;          // 4 | Wt: the four pixels of a k-step share a tile row
    ty[q] = fd_div(p, a.fdWt); tx[q] = p - ty[q] * a.Wt;
  }
  const int ci = l15 & (CA - 1);           // CA = 8: columns 8..15 repeat 0..7 and are not stored by the reduction
  const int npix = a.IH * a.IW;

  f32x4 acc[C5_TAPS];
#pragma unroll
  for (int j = 0; j < C5_TAPS; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;                        // the lane's share of the bias gradient: class l15 over the pixels of its k-lane

  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    int pt = t;
    const int tx_i = pt % a.tiles_x;
    pt /= a.tiles_x;
    const int ty_i = pt % a.tiles_y;
    const int n = pt / a.tiles_y;
    const int y0 = ty_i * a.R, x0 = tx_i * a.Wt;
    // the A operand of the tile's k-steps: G[co = l15][pixel = l4], zero outside the plane and for the 8 unused rows
    float av[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int gy = y0 + ty[q], gx = x0 + tx[q];
      av[q] = 0.f;
      if (l15 < C5_CB && gy < a.H && gx < a.W) av[q] = a.g[((size_t)(n * a.H + gy) * a.W + gx) * C5_CB + l15];
    }
    {
      // pairwise over the tile's 16 values (a chain of single adds through all pixels loses the bias-gradient bar: its result is
      // a sum of signed terms that cancels to a few per cent of their magnitude)
      float b8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) b8[q] = av[2 * q] + av[2 * q + 1];
      bsum += ((b8[0] + b8[1]) + (b8[2] + b8[3])) + ((b8[4] + b8[5]) + (b8[6] + b8[7]));
    }
    __syncthreads();
    with_load_mode<false>(a.mode, [&](auto mode) {
      conv5_stage<decltype(mode)::value, CA>(a.x, cl, xl, n, y0 - 2, x0 - 2, a.H, a.W, a.IW, npix, a.fdIW, tid);
    });
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const float* xq = xl + (ty[q] * a.IW + tx[q]) * S + ci;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx)
          acc[dy * 5 + dx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], xq[(dy * a.IW + dx) * S], acc[dy * 5 + dx], 0, 0, 0);
    }
  }

  // ((wave 0 + wave 1) + wave 2) + wave 3, element by element
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < C5_TAPS; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* d = xl + (j * 4 + r) * 64 + lane;
          *d = w == 0 ? acc[j][r] : *d + acc[j][r];
        }
    }
  }
  // bias gradient: the four k-lanes of a wave ((0 + 1) + (2 + 3): every lane gets the same sum), then the four waves, pairwise
  bsum += __shfl_xor(bsum, 16);
  bsum += __shfl_xor(bsum, 32);
  float* bl = xl + C5_TAPS * 256;          // [4 waves][8]
  if (lane < C5_CB) bl[wave * C5_CB + lane] = bsum;
  __syncthreads();
  // D[row = 4 * (lane >> 4) + r][col = lane & 15] -> part[s][tap][co][ci], then db
  float* row = a.part + (size_t)blockIdx.x * C5_ROW;
  for (int e = tid; e < C5_TAPS * C5_CB * C5_COLS; e += C5_NT) {
    const int j = e / (C5_CB * C5_COLS), co = (e / C5_COLS) % C5_CB, c = e % C5_COLS;
    row[e] = xl[(j * 4 + (co & 3)) * 64 + (co >> 2) * 16 + c];
  }
  if (tid < C5_CB)
    row[C5_TAPS * C5_CB * C5_COLS + tid] = (a.flags & RCV_F_BIAS) ? (bl[tid] + bl[C5_CB + tid]) + (bl[2 * C5_CB + tid] + bl[3 * C5_CB + tid]) : 0.f;
}

__global__ __launch_bounds__(256) void wgrad5_reduce_kernel(const Reduce5Args a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int nw = a.Cout * a.Cin * C5_TAPS;
  if (e < nw) {
    const int co = e / (a.Cin * C5_TAPS), c = (e / C5_TAPS) % a.Cin, j = e % C5_TAPS;
    const float* p = a.part + (j * C5_CB + co) * C5_COLS + c;
    double u = 0.0;      // split 0, 1, ...: a fixed order; the sum is rounded to fp32 once
    for (int s = 0; s < a.nsplit; ++s) u += (double)p[(size_t)s * C5_ROW];
    a.dw[e] = (float)u;
  } else if (e < nw + a.Cout && a.db) {
    const float* p = a.part + C5_TAPS * C5_CB * C5_COLS + (e - nw);
    double u = 0.0;
    for (int s = 0; s < a.nsplit; ++s) u += (double)p[(size_t)s * C5_ROW];
    a.db[e - nw] = (float)u;
  }
}

__global__ __launch_bounds__(256) void pack5_kernel(const Pack5Args a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= C5_TAPS * a.rows * C5_COLS) return;
  const int j = e / (a.rows * C5_COLS), r = (e / C5_COLS) % a.rows, c = e % C5_COLS;
  const int co = a.flip ? r : c, ci = a.flip ? c : r;      // data gradient: rows = class, columns = input channel, taps reversed
  float v = 0.f;
  if (co < a.Cout && ci < a.Cin) v = a.src[(co * a.Cin + ci) * C5_TAPS + (a.flip ? C5_TAPS - 1 - j : j)];
  a.dst[e] = v;
}

int conv5_common_checks(const rcv_op* op, const char* who) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W];
  RCV_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: empty shape N=%d H=%d W=%d", who, N, H, W);
  RCV_CHECK_ARG(op->i[RCV_I_STRIDE] == 1 && op->i[RCV_I_DIL] == 1, "%s: the 5x5 kernels are built for stride 1 / dilation 1 (got %d / %d)", who,
                op->i[RCV_I_STRIDE], op->i[RCV_I_DIL]);
  RCV_CHECK_ARG(op->i[RCV_I_HO] == H && op->i[RCV_I_WO] == W, "%s: output plane %dx%d must equal the input plane %dx%d (pad 2)", who,
                op->i[RCV_I_HO], op->i[RCV_I_WO], H, W);
  RCV_CHECK_ARG((size_t)N * ceil_div(H, 8) * ceil_div(W, 16) < (1ull << 30), "%s: too many tiles", who);
  const int m = op->i[RCV_I_INMODE];
  RCV_CHECK_ARG(m == RCV_LOAD_PLAIN || m == RCV_LOAD_AFFINE || m == RCV_LOAD_AFFINE_RELU,
                "%s: load mode %d of the gathered operand is not built (PLAIN, AFFINE, AFFINE_RELU)", who, m);
  return RCV_OK;
}

int conv5_launch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = conv5_common_checks(op, "conv5")) return rc;
  const int Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT], stats = op->i[RCV_I_STATS];
  RCV_CHECK_ARG(((Cin == 8 || Cin == 16) && Cout == 8) || (Cin == 8 && Cout == 16),
                "conv5: channels %d -> %d are not built (forward 8 / 16 -> 8 padded class channels, i.e. at most 8 classes; data gradient 8 -> 8 / 16)", Cin, Cout);
  RCV_CHECK_ARG(stats >= RCV_STATS_NONE && stats <= RCV_STATS_BWD_DEC, "conv5: statistics kind %d unknown", stats);
  const Tile5 tl = conv5_tiling(op->i[RCV_I_N], op->i[RCV_I_H], op->i[RCV_I_W]);
  if (query) {
    snprintf(query->label, sizeof(query->label), "conv5_mfma<%d,%dx%d>", Cin, tl.R, tl.Wt);
    query->n_part = stats != RCV_STATS_NONE ? tl.ntiles : 0;
    query->part_bytes = (size_t)query->n_part * 2 * Cout * sizeof(float);
    return RCV_OK;
  }
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.in = (const float*)op->p[RCV_P_IN]; a.in_c = (const float*)op->p[RCV_P_IN_C];
  a.w = (const float*)op->p[RCV_P_W]; a.bias = (const float*)op->p[RCV_P_BIAS]; a.out = (float*)op->p[RCV_P_OUT];
  a.resid = (const float*)op->p[RCV_P_RESID]; a.epi_aux = (const float*)op->p[RCV_P_EPI_AUX]; a.epi_c = (const float*)op->p[RCV_P_EPI_C];
  a.part = (float*)op->p[RCV_P_PART];
  a.N = op->i[RCV_I_N]; a.H = a.Ho = op->i[RCV_I_H]; a.W = a.Wo = op->i[RCV_I_W];
  a.Cin = a.CinP = Cin; a.Cout = a.CoutV = Cout; a.CoutP = C5_COLS; a.stride = 1; a.dil = 1;
  a.R = tl.R; a.Wt = tl.Wt; a.tiles_x = tl.tiles_x; a.tiles_y = tl.tiles_y; a.IH = tl.IH; a.IW = tl.IW;
  a.n_pix_tiles = a.total_tiles = tl.ntiles; a.n_co_tiles = 1; a.n_sub = 1; a.nchunks = 1;
  a.in_mode = op->i[RCV_I_INMODE]; a.stats = stats; a.flags = op->flags;
  a.xpitch = Cin + 2;
  a.wl_floats = C5_TAPS * Cin * C5_COLS; a.xl_floats = tl.IH * tl.IW * a.xpitch;
  a.fdWt = make_fastdiv(tl.Wt); a.fdIW = make_fastdiv(tl.IW);
  RCV_CHECK_ARG(a.in && a.w && a.out, "conv5: null operand");
  RCV_CHECK_ARG(a.in_mode == RCV_LOAD_PLAIN || a.in_c, "conv5: load mode %d needs constants", a.in_mode);
  RCV_CHECK_ARG(!(a.flags & RCV_F_BIAS) || a.bias, "conv5: bias flag without bias");
  RCV_CHECK_ARG(!(a.flags & RCV_F_RESID) || a.resid, "conv5: resid flag without tensor");
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || a.part, "conv5: statistics requested without workspace");
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || op->i[RCV_I_NPART] == tl.ntiles, "conv5: workspace rows %d != %d", op->i[RCV_I_NPART], tl.ntiles);
  RCV_CHECK_ARG(!(stats == RCV_STATS_BWD_ENC || stats == RCV_STATS_BWD_DEC) || (a.epi_aux && a.epi_c), "conv5: backward statistics need epi_aux and epi_c");
  const size_t lds = (size_t)(a.wl_floats + a.xl_floats + 5 * Cin + 4 * 2 * 16) * sizeof(float);      // <= 57.6 KB
  const int grid = tl.ntiles < 2 * h->num_cus ? tl.ntiles : 2 * h->num_cus;
  if (Cin == 8) hipLaunchKernelGGL(conv5_kernel<8>, dim3(grid), dim3(C5_NT), lds, s, a);
  else hipLaunchKernelGGL(conv5_kernel<16>, dim3(grid), dim3(C5_NT), lds, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int wgrad5_launch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = conv5_common_checks(op, "wgrad5")) return rc;
  const int CA = op->i[RCV_I_CIN], CB = op->i[RCV_I_COUT];
  RCV_CHECK_ARG((CA == 8 || CA == 16) && CB == C5_CB,
                "wgrad5: channels %d (gathered) x %d (pointwise) are not built (8 / 16 x the 8 padded class channels, i.e. at most 8 classes)", CA, CB);
  RCV_CHECK_ARG(op->i[RCV_I_INMODE2] == RCV_LOAD_PLAIN, "wgrad5: the pointwise operand is read as it is (load mode %d)", op->i[RCV_I_INMODE2]);
  const Tile5 tl = conv5_tiling(op->i[RCV_I_N], op->i[RCV_I_H], op->i[RCV_I_W]);
  const int nsplit = tl.ntiles < h->num_cus ? tl.ntiles : h->num_cus;
  if (query) {
    snprintf(query->label, sizeof(query->label), "wgrad5_mfma<%d,%dx%d>", CA, tl.R, tl.Wt);
    query->n_split = nsplit;
    query->part_bytes = (size_t)nsplit * C5_ROW * sizeof(float);
    return RCV_OK;
  }
  Wgrad5Args a;
  memset(&a, 0, sizeof(a));
  a.x = (const float*)op->p[RCV_P_IN]; a.x_c = (const float*)op->p[RCV_P_IN_C]; a.g = (const float*)op->p[RCV_P_IN2];
  a.part = (float*)op->p[RCV_P_PART];
  a.N = op->i[RCV_I_N]; a.H = op->i[RCV_I_H]; a.W = op->i[RCV_I_W]; a.mode = op->i[RCV_I_INMODE]; a.flags = (int)op->flags;
  a.R = tl.R; a.Wt = tl.Wt; a.tiles_x = tl.tiles_x; a.tiles_y = tl.tiles_y; a.IH = tl.IH; a.IW = tl.IW; a.ntiles = tl.ntiles;
  a.fdWt = make_fastdiv(tl.Wt); a.fdIW = make_fastdiv(tl.IW);
  RCV_CHECK_ARG(a.x && a.g && a.part, "wgrad5: null operand");
  RCV_CHECK_ARG(op->i[RCV_I_NSPLIT] == nsplit, "wgrad5: workspace splits %d != %d", op->i[RCV_I_NSPLIT], nsplit);
  RCV_CHECK_ARG(a.mode == RCV_LOAD_PLAIN || a.x_c, "wgrad5: load mode %d needs constants", a.mode);
  const size_t lds = (size_t)(C5_XL + 5 * CA) * sizeof(float);
  if (CA == 8) hipLaunchKernelGGL(wgrad5_kernel<8>, dim3(nsplit), dim3(C5_NT), lds, s, a);
  else hipLaunchKernelGGL(wgrad5_kernel<16>, dim3(nsplit), dim3(C5_NT), lds, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int filter5_checks(const rcv_op* op, const char* who) {
  const int Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  RCV_CHECK_ARG(Cin == 8 || Cin == 16, "%s: %d input channels are not built (8 or 16)", who, Cin);
  RCV_CHECK_ARG(Cout >= 1 && Cout <= C5_CB, "%s: %d classes are not built (1..%d)", who, Cout, C5_CB);
  return RCV_OK;
}

int reduce5_launch(const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = filter5_checks(op, "wgrad5_reduce")) return rc;
  RCV_CHECK_ARG(op->i[RCV_I_NSPLIT] > 0, "wgrad5_reduce: %d partial rows", op->i[RCV_I_NSPLIT]);
  if (query) { snprintf(query->label, sizeof(query->label), "wgrad5_reduce"); return RCV_OK; }
  Reduce5Args a;
  a.part = (const float*)op->p[RCV_P_PART]; a.dw = (float*)op->p[RCV_P_OUT]; a.db = (float*)op->p[RCV_P_BIAS];
  a.nsplit = op->i[RCV_I_NSPLIT]; a.Cin = op->i[RCV_I_CIN]; a.Cout = op->i[RCV_I_COUT];
  RCV_CHECK_ARG(a.part && a.dw, "wgrad5_reduce: null operand");
  hipLaunchKernelGGL(wgrad5_reduce_kernel, dim3(ceil_div(a.Cout * a.Cin * C5_TAPS + a.Cout, 256)), dim3(256), 0, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int pack5_launch(const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = filter5_checks(op, "pack5")) return rc;
  if (query) { snprintf(query->label, sizeof(query->label), (op->flags & RCV_F_FLIP) ? "pack5<dgrad>" : "pack5<fwd>"); return RCV_OK; }
  Pack5Args a;
  a.src = (const float*)op->p[RCV_P_IN]; a.dst = (float*)op->p[RCV_P_OUT];
  a.Cin = op->i[RCV_I_CIN]; a.Cout = op->i[RCV_I_COUT]; a.flip = (op->flags & RCV_F_FLIP) ? 1 : 0;
  a.rows = a.flip ? C5_CB : a.Cin;
  RCV_CHECK_ARG(a.src && a.dst, "pack5: null operand");
  hipLaunchKernelGGL(pack5_kernel, dim3(ceil_div(C5_TAPS * a.rows * C5_COLS, 256)), dim3(256), 0, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

}  // namespace

int rcv_launch_conv5(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  switch (op->kind) {
    case RCV_OP_CONV5: return conv5_launch(h, op, s, query);
    case RCV_OP_WGRAD5: return wgrad5_launch(h, op, s, query);
    case RCV_OP_WGRAD5_REDUCE: return reduce5_launch(op, s, query);
    default: return pack5_launch(op, s, query);
  }
}
