// Pointwise (1x1) convolution family between feature maps (model.py:333-377: ConvSep.conv_1x1, trConvSep.conv): forward and data
// gradient in one kernel, the filter gradient with its fixed-order reduction, and the cross-shaped 3x3 filters the 1-D conv pairs
// of those blocks are lowered to.  fp32 on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain per output).  DESIGN.md 4.18.
//
//   RCV_OP_PW        D[co][pixel] += W[co][k] * X[k][pixel] over the flat pixel list P = N*H*W, the mapping of conv5.hip: every lane ends
//                    with four consecutive output channels of one pixel and the shared epilogue (conv_epilogue.h) applies unchanged,
//                    the tensor seen as ONE row of P pixels cut into tiles of 64 * WN.  Neither operand is packed or staged pixel by
//                    pixel: the contraction index of an MFMA step is free as long as A and B agree on it, so a lane loads the float4
//                    X[pixel = l15][16 j + 4 l4 ..] (through the load transform) and feeds its four components to four consecutive
//                    steps; the filter is read from the PARAMETER ([COUT][CIN], or [CIN][COUT] with RCV_F_TRANSPOSED_SRC: the data
//                    gradient) into LDS once per workgroup, rows in that step order, optionally scaled per output channel (the
//                    inference BatchNorm fold).  A workgroup walks the tiles blockIdx.x, + gridDim.x, ...; partial row = tile.
//   RCV_OP_PW_WGRAD  D[co][ci] += G[pixel][co] * X[pixel][ci]: K = pixels, four per MFMA step.  A workgroup stages a chunk of 64
//                    pixels of both operands (through their load transforms) in LDS -- all input channels, and the range of output
//                    channels blockIdx.y names, so that its four waves share at most 16 blocks of 16 x 16 of the filter -- and walks
//                    the chunks blockIdx.x, + gridDim.x, ...; the workgroups (s, *) write partial row s between them.  No atomics.
//   RCV_OP_PW_WGRAD_REDUCE  rows 0, 1, ... summed in float64 in that order, rounded once.
//   RCV_OP_CROSS_PACK / RCV_OP_CROSS_GRAD  two 1-D filters <-> one dense 3x3 parameter-layout filter with a cross of non-zero taps.
#include "conv_common.h"
#include "conv_epilogue.h"

namespace {

constexpr int PW_NT = 256;
constexpr int PW_WGRAD_CAP = 4;    // filter blocks per wave of the filter gradient where the record does not say (i[AUX0])
constexpr int PW_CHUNK = 64;       // pixels per staged chunk of the filter gradient (a multiple of 16)

// row pitch of an LDS image whose 16-float column blocks are read by the four k-lanes of a wave at rows l4, l4 + ..: pitch % 32 == 16
// puts the four rows on four different groups of 16 banks
inline int pw_pitch(int cols) { return cols % 32 == 16 ? cols : cols + 16; }

struct PwArgs {
  ConvArgs c;            // the epilogue's view: Ho = 1, Wo = P, R = 1, Wt = tile
  const float* scale;    // per output channel, or NULL
  int P;                 // pixels
  int J;                 // ceil(Cin / 16)
  int WP;                // floats per filter row in LDS
  int transposed;        // filter parameter is [Cin][Cout]
  int ntiles;
};

struct PwWgradArgs {
  const float* x;        // [P][CA]
  const float* x_c;
  const float* g;        // [P][CB]
  const float* g_aux;
  const float* g_c;
  float* part;           // [nsplit][CB][CA]
  int P, CA, CB, CAP, CBP, XP, GP, x_mode, g_mode, nchunks;
  int chunk;             // pixels per staged chunk
  int CBW;               // output channels of one workgroup (blockIdx.y takes the range CBW * blockIdx.y ..), a multiple of 16
};

struct PwReduceArgs {
  const float* part;
  float* dw;
  int nsplit, n;
};

struct CrossArgs {
  const float* a;        // form 0: [D0/2][D1][3][1]   form 1: [D0][D1][1][3]
  const float* b;        // form 0: [D0/2][D1][1][3]   form 1: [D0][D1][3][1]
  float* dense;          // [D0][D1][3][3]
  float* ga;
  float* gb;
  int D0, D1, form;
};

template <int WM, int WN, int MODE>
__device__ __forceinline__ void pw_tile(const PwArgs& pa, const float* wl, const float* cl, int x0, f32x4 (&acc)[WM][WN], int tid) {
  const ConvArgs& a = pa.c;
  const int lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int CinP = pa.J * 16;
  constexpr bool TWO = MODE == RCV_LOAD_GRAD_ENC || MODE == RCV_LOAD_GRAD_DEC;
  size_t off[WN];
  bool okp[WN];
#pragma unroll
  for (int b = 0; b < WN; ++b) {
    const int p = x0 + (wave * WN + b) * 16 + l15;
    okp[b] = p < pa.P;
    off[b] = (size_t)(okp[b] ? p : 0) * a.Cin;
  }
  for (int j = 0; j < pa.J; ++j) {
    const int ch = 16 * j + 4 * l4;
    const bool ch_ok = ch < a.Cin;          // Cin % 4 == 0: the whole quad is inside or outside
    float4 k[5];
    if (MODE != RCV_LOAD_PLAIN) {
#pragma unroll
      for (int r = 0; r < 5; ++r) k[r] = *reinterpret_cast<const float4*>(cl + r * CinP + ch);
    }
    float xs[WN][4];
#pragma unroll
    for (int b = 0; b < WN; ++b) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (okp[b] && ch_ok) {
        const float4 x = ld4(a.in + off[b] + ch);
        float4 ax = v;
        if (TWO) ax = ld4(a.in_aux + off[b] + ch);
        v = xform4<MODE>(x, ax, k);
      }
      xs[b][0] = v.x; xs[b][1] = v.y; xs[b][2] = v.z; xs[b][3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* wr = wl + (j * 16 + c * 4 + l4) * pa.WP + l15;
      float av[WM];
#pragma unroll
      for (int m = 0; m < WM; ++m) av[m] = wr[m * 16];
#pragma unroll
      for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int b = 0; b < WN; ++b) acc[m][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], xs[b][c], acc[m][b], 0, 0, 0);
    }
  }
}

template <int WM, int WN>
__global__ __launch_bounds__(PW_NT) void pw_kernel(const PwArgs pa) {
  const ConvArgs& a = pa.c;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int CinP = pa.J * 16;
  constexpr int CoP = WM * 16;
  float* wl = smem;                       // [CinP][WP]: row 16 j + 4 c + l4 holds input channel 16 j + 4 l4 + c
  float* cl = wl + CinP * pa.WP;          // [5][CinP]
  float* red = cl + 5 * CinP;             // [4][2][CoP]
  const int tid = threadIdx.x;

  if (a.in_mode != RCV_LOAD_PLAIN)
    for (int e = tid; e < 5 * CinP; e += PW_NT) {
      const int r = e / CinP, ch = e - r * CinP;
      cl[e] = ch < a.Cin ? a.in_c[r * a.Cin + ch] : 0.f;
    }
  for (int e = tid; e < CinP * CoP; e += PW_NT) {
    int co, ci;
    if (pa.transposed) { ci = e / CoP; co = e - ci * CoP; }       // the parameter's rows are contiguous along what it calls Cout
    else { co = e / CinP; ci = e - co * CinP; }
    float v = 0.f;
    if (co < a.Cout && ci < a.Cin) {
      v = pa.transposed ? a.w[(size_t)ci * a.Cout + co] : a.w[(size_t)co * a.Cin + ci];
      if (pa.scale) v *= pa.scale[co];
    }
    wl[((ci >> 4) * 16 + (ci & 3) * 4 + ((ci >> 2) & 3)) * pa.WP + co] = v;
  }

  for (int t = blockIdx.x; t < pa.ntiles; t += gridDim.x) {
    TileInfo ti;
    ti.n = 0; ti.y0 = 0; ti.x0 = t * (64 * WN); ti.co0 = 0; ti.py = 0; ti.px = 0; ti.oy0 = 0; ti.ox0 = ti.x0; ti.pt = t;
    __syncthreads();      // the previous tile's reads of red; the first tile: wl and cl are written
    f32x4 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int b = 0; b < WN; ++b) acc[m][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.in_mode == RCV_LOAD_GRAD_ENC || a.in_mode == RCV_LOAD_GRAD_DEC)
      with_load_mode<true>(a.in_mode, [&](auto mode) { pw_tile<WM, WN, decltype(mode)::value>(pa, wl, cl, ti.x0, acc, tid); });
    else
      with_load_mode<false>(a.in_mode, [&](auto mode) { pw_tile<WM, WN, decltype(mode)::value>(pa, wl, cl, ti.x0, acc, tid); });
    conv_epilogue<WM, WN, 1, 4, KIND_GATHER>(a, ti, acc, red, tid);
  }
}

// `chunk` pixels of the channels c0 .. c0 + CW of one operand -> dst[pixel][pitch], through its load transform (cl: its constants
// [5][CP] from channel 0); zero past the tensor and past its channels
__device__ __forceinline__ void pw_stage(const float* __restrict__ src, const float* __restrict__ aux, const float* cl, float* dst, int mode, int C,
                                         int CP, int c0, int CW, int pitch, int chunk, int p0, int P, int tid) {
  const int Q = CW / 4;
  const bool two = mode == RCV_LOAD_GRAD_ENC || mode == RCV_LOAD_GRAD_DEC;
  for (int e = tid; e < chunk * Q; e += PW_NT) {
    const int pix = e / Q, cw = 4 * (e - pix * Q), ch = c0 + cw;
    const int p = p0 + pix;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < P && ch < C) {
      const size_t off = (size_t)p * C + ch;
      const float4 x = ld4(src + off);
      float4 ax = v;
      if (two) ax = ld4(aux + off);
      float4 k[5];
      if (mode != RCV_LOAD_PLAIN) {
#pragma unroll
        for (int r = 0; r < 5; ++r) k[r] = *reinterpret_cast<const float4*>(cl + r * CP + ch);
      }
      v = xform_rt(mode, x, ax, k);
    }
    *reinterpret_cast<float4*>(dst + pix * pitch + cw) = v;
  }
}

template <int NB>
__global__ __launch_bounds__(PW_NT) void pw_wgrad_kernel(const PwWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xl = smem;                           // [chunk][XP]
  float* gl = xl + a.chunk * a.XP;            // [chunk][GP]: the workgroup's CBW output channels
  float* clx = gl + a.chunk * a.GP;           // [5][CAP]
  float* clg = clx + 5 * a.CAP;               // [5][CBP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int cb0 = blockIdx.y * a.CBW;         // first output channel of this workgroup

  if (a.x_mode != RCV_LOAD_PLAIN)
    for (int e = tid; e < 5 * a.CAP; e += PW_NT) { const int r = e / a.CAP, ch = e - r * a.CAP; clx[e] = ch < a.CA ? a.x_c[r * a.CA + ch] : 0.f; }
  if (a.g_mode != RCV_LOAD_PLAIN)
    for (int e = tid; e < 5 * a.CBP; e += PW_NT) { const int r = e / a.CBP, ch = e - r * a.CBP; clg[e] = ch < a.CB ? a.g_c[r * a.CB + ch] : 0.f; }

  // the wave's blocks of the filter: block q = wave + 4 i covers output channels cb0 + 16 (q / nbx) .., input channels 16 (q % nbx) ..
  const int nbx = a.CAP / 16, nblocks = nbx * (a.CBW / 16);
  int goff[NB], xoff[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int q = wave + 4 * i;
    const int qq = q < nblocks ? q : 0;
    goff[i] = l4 * a.GP + (qq / nbx) * 16 + l15;
    xoff[i] = l4 * a.XP + (qq % nbx) * 16 + l15;
  }
  f32x4 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ksteps = a.chunk / 4;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    __syncthreads();      // the previous chunk's reads; the first chunk: the constants are written
    pw_stage(a.x, nullptr, clx, xl, a.x_mode, a.CA, a.CAP, 0, a.CAP, a.XP, a.chunk, c * a.chunk, a.P, tid);
    pw_stage(a.g, a.g_aux, clg, gl, a.g_mode, a.CB, a.CBP, cb0, a.CBW, a.GP, a.chunk, c * a.chunk, a.P, tid);
    __syncthreads();
    for (int s0 = 0; s0 < ksteps; s0 += 4) {      // (chunk % 16 == 0)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + u;
#pragma unroll
        for (int i = 0; i < NB; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(gl[4 * s * a.GP + goff[i]], xl[4 * s * a.XP + xoff[i]], acc[i], 0, 0, 0);
      }
    }
  }
  // D[row = 4 * l4 + r][col = l15] -> part[s][co][ci]; every element of the row is written by exactly one lane of one workgroup
  float* row = a.part + (size_t)blockIdx.x * a.CB * a.CA;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int q = wave + 4 * i;
    if (q >= nblocks) continue;
    const int ci = (q % nbx) * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cb0 + (q / nbx) * 16 + 4 * l4 + r;
      if (co < a.CB && ci < a.CA) row[co * a.CA + ci] = acc[i][r];
    }
  }
}

// 16 consecutive elements x 16 row lanes per workgroup: lane l sums the rows l, l + 16, ... in that order in float64, then the 16
// lane sums are added in lane order and rounded to fp32 once.  A fixed order whatever the grid (one thread per element over up to
// 1024 rows was a serial chain of dependent loads: 0.43 ms for an 8 x 8 filter).
__global__ __launch_bounds__(256) void pw_reduce_kernel(const PwReduceArgs a) {
  __shared__ double sums[16][17];
  const int el = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;          // (n % 16 == 0: channels are multiples of 8 on both sides, and n = Cin * Cout >= 64)
  double u = 0.0;
  if (e < a.n) {
    int s = rl;
    for (; s + 48 < a.nsplit; s += 64) {        // four loads in flight; added in the order of the plain loop
      const float v0 = a.part[(size_t)s * a.n + e], v1 = a.part[(size_t)(s + 16) * a.n + e];
      const float v2 = a.part[(size_t)(s + 32) * a.n + e], v3 = a.part[(size_t)(s + 48) * a.n + e];
      u += (double)v0; u += (double)v1; u += (double)v2; u += (double)v3;
    }
    for (; s < a.nsplit; s += 16) u += (double)a.part[(size_t)s * a.n + e];
  }
  sums[rl][el] = u;
  __syncthreads();
  if (rl == 0 && e < a.n) {
    double t = sums[0][el];
#pragma unroll
    for (int r = 1; r < 16; ++r) t += sums[r][el];
    a.dw[e] = (float)t;
  }
}

// form 0 (cat(conv_nx1, conv_1xn), model.py:342-349): dense [D0 = planes][D1 = inplanes][3][3]; rows < D0 / 2 carry a in the centre
// column, the others b in the centre row.  form 1 (trconv1x3 + trconv3x1, model.py:367-376): dense [D0][D1][3][3] in the transposed
// conv's own [in][out] layout; a in the centre row, b in the centre column, the centre tap their sum.
__global__ __launch_bounds__(256) void cross_pack_kernel(const CrossArgs c) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= c.D0 * c.D1 * 9) return;
  const int t = e % 9, ky = t / 3, kx = t - 3 * ky, rc = e / 9;      // rc = d0 * D1 + d1
  float v = 0.f;
  if (c.form == 0) {
    const int half = (c.D0 / 2) * c.D1;
    if (rc < half) { if (kx == 1) v = c.a[rc * 3 + ky]; }
    else if (ky == 1) v = c.b[(rc - half) * 3 + kx];
  } else {
    if (ky == 1) v = c.a[rc * 3 + kx];
    if (kx == 1) v += c.b[rc * 3 + ky];
  }
  c.dense[e] = v;
}

// the gather that undoes cross_pack_kernel on a gradient: one thread per element of the two 1-D filters; the centre gradient of
// form 1 goes to both
__global__ __launch_bounds__(256) void cross_grad_kernel(const CrossArgs c) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int na = (c.form == 0 ? c.D0 / 2 : c.D0) * c.D1 * 3;
  if (e >= 2 * na) return;
  const bool second = e >= na;
  const int i = second ? e - na : e, rc = i / 3, k = i - 3 * rc;
  if (c.form == 0) {
    if (!second) c.ga[i] = c.dense[rc * 9 + k * 3 + 1];
    else c.gb[i] = c.dense[(rc + (c.D0 / 2) * c.D1) * 9 + 3 + k];
  } else {
    if (!second) c.ga[i] = c.dense[rc * 9 + 3 + k];
    else c.gb[i] = c.dense[rc * 9 + k * 3 + 1];
  }
}

int pw_shape_checks(const rcv_op* op, const char* who) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  RCV_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: empty shape N=%d H=%d W=%d", who, N, H, W);
  RCV_CHECK_ARG(Cin >= 8 && Cin <= 128 && Cin % 8 == 0 && Cout >= 8 && Cout <= 128 && Cout % 8 == 0,
                "%s: channels %d -> %d are not built (multiples of 8 in 8..128 on both sides)", who, Cin, Cout);
  const double P = (double)N * H * W;
  RCV_CHECK_ARG(P * (Cin > Cout ? Cin : Cout) < 2147483648.0, "%s: operand exceeds 2^31 elements", who);
  return RCV_OK;
}

template <int WM, int WN>
int pw_launch_t(const rcv_handle* h, const PwArgs& pa, int grid, size_t lds, hipStream_t s) {
  static size_t configured[RCV_MAX_DEVICES];
  RCV_ENSURE_LDS((pw_kernel<WM, WN>), lds, h->device, configured);
  hipLaunchKernelGGL((pw_kernel<WM, WN>), dim3(grid), dim3(PW_NT), lds, s, pa);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int pw_launch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = pw_shape_checks(op, "pw")) return rc;
  const int Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT], stats = op->i[RCV_I_STATS], mode = op->i[RCV_I_INMODE];
  RCV_CHECK_ARG(mode == RCV_LOAD_PLAIN || mode == RCV_LOAD_AFFINE || mode == RCV_LOAD_AFFINE_RELU || mode == RCV_LOAD_GRAD_ENC || mode == RCV_LOAD_GRAD_DEC,
                "pw: load mode %d is not built (PLAIN, AFFINE, AFFINE_RELU, GRAD_ENC, GRAD_DEC)", mode);
  RCV_CHECK_ARG(stats >= RCV_STATS_NONE && stats <= RCV_STATS_BWD_DEC, "pw: statistics kind %d unknown", stats);
  const int P = op->i[RCV_I_N] * op->i[RCV_I_H] * op->i[RCV_I_W];
  const int cob = ceil_div(Cout, 16);
  const int WM = cob <= 1 ? 1 : (cob <= 2 ? 2 : (cob <= 4 ? 4 : 8));
  const int WN = WM == 8 ? 2 : 4;      // 64 accumulator registers at most
  const int tile = 64 * WN, ntiles = ceil_div(P, tile);
  if (query) {
    snprintf(query->label, sizeof(query->label), "pw_mfma<%d,%d%s>", WM, WN, (op->flags & RCV_F_TRANSPOSED_SRC) ? ",t" : "");
    query->n_part = stats != RCV_STATS_NONE ? ntiles : 0;
    query->part_bytes = (size_t)query->n_part * 2 * Cout * sizeof(float);
    return RCV_OK;
  }
  PwArgs pa;
  memset(&pa, 0, sizeof(pa));
  ConvArgs& a = pa.c;
  a.in = (const float*)op->p[RCV_P_IN]; a.in_aux = (const float*)op->p[RCV_P_IN_AUX]; a.in_c = (const float*)op->p[RCV_P_IN_C];
  a.w = (const float*)op->p[RCV_P_W]; a.bias = (const float*)op->p[RCV_P_BIAS]; a.out = (float*)op->p[RCV_P_OUT];
  a.resid = (const float*)op->p[RCV_P_RESID]; a.epi_aux = (const float*)op->p[RCV_P_EPI_AUX]; a.epi_c = (const float*)op->p[RCV_P_EPI_C];
  a.part = (float*)op->p[RCV_P_PART];
  a.N = 1; a.H = a.Ho = 1; a.W = a.Wo = P;
  a.Cin = a.CinP = Cin; a.Cout = a.CoutV = Cout; a.CoutP = WM * 16; a.stride = 1; a.dil = 1;
  a.R = 1; a.Wt = tile; a.tiles_x = ntiles; a.tiles_y = 1; a.IH = 1; a.IW = tile;
  a.n_pix_tiles = a.total_tiles = ntiles; a.n_co_tiles = 1; a.n_sub = 1; a.nchunks = 1;
  a.in_mode = mode; a.stats = stats; a.flags = op->flags;
  a.fdWt = make_fastdiv(tile); a.fdIW = make_fastdiv(tile);
  pa.scale = (const float*)op->p[RCV_P_X0];
  pa.P = P; pa.J = ceil_div(Cin, 16); pa.WP = pw_pitch(WM * 16); pa.transposed = (op->flags & RCV_F_TRANSPOSED_SRC) ? 1 : 0; pa.ntiles = ntiles;
  const bool two = mode == RCV_LOAD_GRAD_ENC || mode == RCV_LOAD_GRAD_DEC;
  RCV_CHECK_ARG(a.in && a.w && a.out, "pw: null operand");
  RCV_CHECK_ARG(mode == RCV_LOAD_PLAIN || a.in_c, "pw: load mode %d needs constants", mode);
  RCV_CHECK_ARG(!two || a.in_aux, "pw: gradient load needs aux tensor");
  RCV_CHECK_ARG(!(a.flags & RCV_F_BIAS) || a.bias, "pw: bias flag without bias");
  RCV_CHECK_ARG(!(a.flags & RCV_F_RESID) || a.resid, "pw: resid flag without tensor");
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || a.part, "pw: statistics requested without workspace");
  RCV_CHECK_ARG(stats == RCV_STATS_NONE || op->i[RCV_I_NPART] == ntiles, "pw: workspace rows %d != %d", op->i[RCV_I_NPART], ntiles);
  RCV_CHECK_ARG(!(stats == RCV_STATS_BWD_ENC || stats == RCV_STATS_BWD_DEC) || (a.epi_aux && a.epi_c), "pw: backward statistics need epi_aux and epi_c");
  const int CinP = pa.J * 16;
  const size_t lds = (size_t)(CinP * pa.WP + 5 * CinP + 4 * 2 * WM * 16) * sizeof(float);      // <= 80.4 KB
  const int grid = ntiles < 2 * h->num_cus ? ntiles : 2 * h->num_cus;
  switch (WM) {
    case 1: return pw_launch_t<1, 4>(h, pa, grid, lds, s);
    case 2: return pw_launch_t<2, 4>(h, pa, grid, lds, s);
    case 4: return pw_launch_t<4, 4>(h, pa, grid, lds, s);
    default: return pw_launch_t<8, 2>(h, pa, grid, lds, s);
  }
}

template <int NB>
int pw_wgrad_launch_t(const rcv_handle* h, const PwWgradArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  static size_t configured[RCV_MAX_DEVICES];
  RCV_ENSURE_LDS(pw_wgrad_kernel<NB>, lds, h->device, configured);
  hipLaunchKernelGGL(pw_wgrad_kernel<NB>, grid, dim3(PW_NT), lds, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int pw_wgrad_launch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (const int rc = pw_shape_checks(op, "pw_wgrad")) return rc;
  const int CA = op->i[RCV_I_CIN], CB = op->i[RCV_I_COUT], xm = op->i[RCV_I_INMODE], gm = op->i[RCV_I_INMODE2];
  RCV_CHECK_ARG(xm == RCV_LOAD_PLAIN || xm == RCV_LOAD_AFFINE || xm == RCV_LOAD_AFFINE_RELU,
                "pw_wgrad: load mode %d of the layer input is not built (PLAIN, AFFINE, AFFINE_RELU)", xm);
  RCV_CHECK_ARG(gm == RCV_LOAD_PLAIN || gm == RCV_LOAD_GRAD_ENC || gm == RCV_LOAD_GRAD_DEC,
                "pw_wgrad: load mode %d of the output gradient is not built (PLAIN, GRAD_ENC, GRAD_DEC)", gm);
  const int P = op->i[RCV_I_N] * op->i[RCV_I_H] * op->i[RCV_I_W];
  const int CAP = round_up(CA, 16), CBP = round_up(CB, 16);
  // a workgroup takes all input channels and as many blocks of 16 output channels as leave each wave at most `cap` blocks of the
  // filter; the ranges go to blockIdx.y.  cap = i[AUX0] (4 or 8; 0 = the library's choice): 4 keeps four waves per SIMD resident, which
  // cover each other's staging; 8 halves the number of ranges and with it the re-reads of x
  const int cap = op->i[RCV_I_AUX0] ? op->i[RCV_I_AUX0] : PW_WGRAD_CAP;
  RCV_CHECK_ARG(cap == 4 || cap == 8, "pw_wgrad: %d filter blocks per wave are not built (i[AUX0] = 0, 4 or 8)", cap);
  const int nbx = CAP / 16, nbg = CBP / 16;
  int nbw = 4 * cap / nbx < 1 ? 1 : 4 * cap / nbx;
  if (nbw > nbg) nbw = nbg;
  const int cosplit = ceil_div(nbg, nbw), CBW = nbw * 16;
  const int per_wave = ceil_div(nbx * nbw, 4);
  const int NB = per_wave <= 1 ? 1 : (per_wave <= 2 ? 2 : (per_wave <= 4 ? 4 : 8));
  // 64 pixels per chunk: an accumulator's fp32 chain is 64 products per chunk of its workgroup, and with one row per chunk (below) a
  // plane of a few hundred pixels is summed across chunks in float64 by the reduction.  (256-pixel chunks on the narrow layers put 234
  // pixels in one chain: 7.2e-7 of the largest entry against the bar of 5e-7.)
  const int XP = pw_pitch(CAP), GP = pw_pitch(CBW);
  const int chunk = PW_CHUNK;
  const int nchunks = ceil_div(P, chunk);
  // rows: one per workgroup along x; up to four per compute unit while all rows together stay below 8 MiB
  int per_cu = (int)((8u << 20) / ((size_t)h->num_cus * CA * CB * sizeof(float)));
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  const int nsplit = nchunks < per_cu * h->num_cus ? nchunks : per_cu * h->num_cus;
  if (query) {
    snprintf(query->label, sizeof(query->label), "pw_wgrad_mfma<%d,%d,%d>", NB, chunk, cosplit);
    query->n_split = nsplit;
    query->part_bytes = (size_t)nsplit * CA * CB * sizeof(float);
    return RCV_OK;
  }
  PwWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const float*)op->p[RCV_P_IN]; a.x_c = (const float*)op->p[RCV_P_IN_C];
  a.g = (const float*)op->p[RCV_P_IN2]; a.g_aux = (const float*)op->p[RCV_P_IN2_AUX]; a.g_c = (const float*)op->p[RCV_P_IN2_C];
  a.part = (float*)op->p[RCV_P_PART];
  a.P = P; a.CA = CA; a.CB = CB; a.CAP = CAP; a.CBP = CBP; a.XP = XP; a.GP = GP;
  a.x_mode = xm; a.g_mode = gm; a.nchunks = nchunks; a.chunk = chunk; a.CBW = CBW;
  RCV_CHECK_ARG(a.x && a.g && a.part, "pw_wgrad: null operand");
  RCV_CHECK_ARG(op->i[RCV_I_NSPLIT] == nsplit, "pw_wgrad: workspace splits %d != %d", op->i[RCV_I_NSPLIT], nsplit);
  RCV_CHECK_ARG(xm == RCV_LOAD_PLAIN || a.x_c, "pw_wgrad: load mode %d needs constants", xm);
  RCV_CHECK_ARG(gm == RCV_LOAD_PLAIN || (a.g_c && a.g_aux), "pw_wgrad: gradient load mode %d needs constants and the aux tensor", gm);
  const size_t lds = (size_t)(chunk * (XP + GP) + 5 * (CAP + CBP)) * sizeof(float);      // <= 62.5 KB
  const dim3 grid(nsplit, cosplit);
  switch (NB) {
    case 1: return pw_wgrad_launch_t<1>(h, a, grid, lds, s);
    case 2: return pw_wgrad_launch_t<2>(h, a, grid, lds, s);
    case 4: return pw_wgrad_launch_t<4>(h, a, grid, lds, s);
    default: return pw_wgrad_launch_t<8>(h, a, grid, lds, s);
  }
}

int pw_reduce_launch(const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  RCV_CHECK_ARG(Cin >= 8 && Cin <= 128 && Cin % 8 == 0 && Cout >= 8 && Cout <= 128 && Cout % 8 == 0,
                "pw_wgrad_reduce: channels %d -> %d are not built (multiples of 8 in 8..128 on both sides)", Cin, Cout);
  RCV_CHECK_ARG(op->i[RCV_I_NSPLIT] > 0, "pw_wgrad_reduce: %d partial rows", op->i[RCV_I_NSPLIT]);
  if (query) { snprintf(query->label, sizeof(query->label), "pw_wgrad_reduce"); return RCV_OK; }
  PwReduceArgs a;
  a.part = (const float*)op->p[RCV_P_PART]; a.dw = (float*)op->p[RCV_P_OUT]; a.nsplit = op->i[RCV_I_NSPLIT]; a.n = Cin * Cout;
  RCV_CHECK_ARG(a.part && a.dw, "pw_wgrad_reduce: null operand");
  hipLaunchKernelGGL(pw_reduce_kernel, dim3(ceil_div(a.n, 16)), dim3(256), 0, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int cross_launch(const rcv_op* op, hipStream_t s, OpQuery* query) {
  const bool grad = op->kind == RCV_OP_CROSS_GRAD;
  const char* who = grad ? "cross_grad" : "cross_pack";
  CrossArgs c;
  memset(&c, 0, sizeof(c));
  c.D0 = op->i[RCV_I_COUT]; c.D1 = op->i[RCV_I_CIN]; c.form = op->i[RCV_I_AUX0];
  RCV_CHECK_ARG(c.form == 0 || c.form == 1, "%s: form %d unknown (0 = concatenated conv pair, 1 = summed transposed pair)", who, c.form);
  RCV_CHECK_ARG(c.D0 > 0 && c.D1 > 0 && c.D0 <= 1024 && c.D1 <= 1024 && (c.form == 1 || c.D0 % 2 == 0),
                "%s: filter dimensions %d x %d (the concatenated pair needs an even first dimension)", who, c.D0, c.D1);
  if (query) { snprintf(query->label, sizeof(query->label), "%s<%d>", who, c.form); return RCV_OK; }
  if (grad) {
    c.dense = (float*)op->p[RCV_P_IN]; c.ga = (float*)op->p[RCV_P_OUT]; c.gb = (float*)op->p[RCV_P_X0];
    RCV_CHECK_ARG(c.dense && c.ga && c.gb, "cross_grad: null operand");
    const int n = 2 * (c.form == 0 ? c.D0 / 2 : c.D0) * c.D1 * 3;
    hipLaunchKernelGGL(cross_grad_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, c);
  } else {
    c.a = (const float*)op->p[RCV_P_IN]; c.b = (const float*)op->p[RCV_P_IN2]; c.dense = (float*)op->p[RCV_P_OUT];
    RCV_CHECK_ARG(c.a && c.b && c.dense, "cross_pack: null operand");
    hipLaunchKernelGGL(cross_pack_kernel, dim3(ceil_div(c.D0 * c.D1 * 9, 256)), dim3(256), 0, s, c);
  }
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

}  // namespace

int rcv_launch_pw(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  switch (op->kind) {
    case RCV_OP_PW: return pw_launch(h, op, s, query);
    case RCV_OP_PW_WGRAD: return pw_wgrad_launch(h, op, s, query);
    case RCV_OP_PW_WGRAD_REDUCE: return pw_reduce_launch(op, s, query);
    default: return cross_launch(op, s, query);
  }
}
