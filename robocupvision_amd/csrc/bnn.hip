// The BNN-L / BNN-M-C patch classifiers of the reference (model.py:569-619; trained by objDetEval.py:89-119, run by classVal.py):
//   stage:  x = relu(pool(dropout2d(conv(x))))     K x K conv, stride 1, pad P; MaxPool2d(k, 2) with overlapping windows (k = 4) or
//                                                  MaxPool2d(2, 2); BNN-M-C's classifier is a stage without pool, dropout and ReLU
//   head:   classifier(relu(dropout(fc(x))))       BNN-L: 16 -> 512 -> 4 pointwise, element-wise dropout in the middle
// The step is bound by its chain of dependent launches (3.7 M MAC per 32x32 patch), so a whole stage is ONE launch per direction:
//   bnn_stage_fwd_kernel  a workgroup owns 4x4 outputs of one image: stages the input region planar in LDS, forms the conv tile
//                         (<= 10x10 pixels, all output channels) into LDS, pools it, stores the output and the arg-max bytes
//   bnn_stage_bwd_kernel  a workgroup owns a T x T tile (T = 8; about 16, dividing the plane evenly, for the 3-channel first stage) of the input AND of the conv plane:
//                         gathers d loss / d conv over the <= 4 windows of every pixel of the tile + halo into LDS (no atomics), then
//                         the data gradient of its input pixels and its partial filter / bias gradient (one workspace row)
//   bnn_rows_reduce_kernel  fixed-order sum of the partial rows -> gradients in parameter layout
//   bnn_head_fwd_kernel / bnn_head_bwd_kernel  a workgroup per pixel of the head plane (a thread owns two of the 512 hidden units)
// Arithmetic: fp32 on the vector pipe.  Contractions are 27..1024 long per output with a few thousand outputs per image; the filter
// value of a multiply-add is wave-uniform (a scalar load), the activation one LDS read.  No float atomics, fixed summation orders.
#include "rcv_internal.h"

#define BNN_TP 4          // outputs per tile side of the forward
#define BNN_MAX_C 16
#define BNN_MAX_K 8
#define BNN_FWD_TC 10     // conv pixels per tile side: (BNN_TP - 1) * 2 + 4
#define BNN_HID 512
#define BNN_MAX_OUT 8

struct BnnStage {
  const float* x; const float* w; const float* bias; const float* keep;
  const float* dout; const float* out_c; const uint8_t* arg_c;      // backward
  float* out; uint8_t* arg; uint8_t* label; float* dx; float* part;
  int N, H, W, Cin, Cout, P, k, Hc, Wc, Ho, Wo, T, tiles_y, tiles_x, nchw_in, relu, nchw_out, row_width;
};

__device__ __forceinline__ size_t bnn_out_index(const BnnStage& a, int n, int oy, int ox, int co) {
  return a.nchw_out ? (((size_t)n * a.Cout + co) * a.Ho + oy) * a.Wo + ox : (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Cout + co;
}

// stages rows [gy0, gy0 + rh) x columns [gx0, gx0 + rw) of image n planar into dst[ci][rh][rw]; zero outside the plane
__device__ __forceinline__ void bnn_stage_input(const BnnStage& a, int n, int gy0, int gx0, int rh, int rw, float* dst) {
  const int total = a.Cin * rh * rw;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    int ci, r;
    if (a.nchw_in) { ci = e / (rh * rw); r = e - ci * rh * rw; }
    else { ci = e % a.Cin; r = e / a.Cin; }
    const int y = r / rw, x = r - y * rw, gy = gy0 + y, gx = gx0 + x;
    float v = 0.f;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
      v = a.nchw_in ? a.x[(((size_t)n * a.Cin + ci) * a.H + gy) * a.W + gx] : a.x[(((size_t)n * a.H + gy) * a.W + gx) * a.Cin + ci];
    dst[(ci * rh + y) * rw + x] = v;
  }
}

// out[n,py,px,c] = relu(max over the k x k window at stride 2 of ((conv(x) + bias)[n,y,x,c] * keep[n,c])); arg = window offset of the
// FIRST maximum in row-major order (aten::max_pool2d_with_indices).  k == 0: no pool.
template <int K>
__global__ __launch_bounds__(256) void bnn_stage_fwd_kernel(BnnStage a) {
  __shared__ float s_in[BNN_MAX_C * (BNN_FWD_TC + K - 1) * (BNN_FWD_TC + K - 1)];
  __shared__ float s_cv[BNN_MAX_C * BNN_FWD_TC * BNN_FWD_TC];
  const int b = blockIdx.x;
  const int tx = b % a.tiles_x, ty = (b / a.tiles_x) % a.tiles_y, n = b / (a.tiles_x * a.tiles_y);
  const int stride = a.k ? 2 : 1, win = a.k ? a.k : 1;
  const int oy0 = ty * BNN_TP, ox0 = tx * BNN_TP;
  const int toh = min(BNN_TP, a.Ho - oy0), tow = min(BNN_TP, a.Wo - ox0);
  const int cy0 = oy0 * stride, cx0 = ox0 * stride;
  const int tch = (toh - 1) * stride + win, tcw = (tow - 1) * stride + win;      // <= BNN_FWD_TC; inside the conv plane (floor pooling)
  const int ih = tch + K - 1, iw = tcw + K - 1;
  bnn_stage_input(a, n, cy0 - a.P, cx0 - a.P, ih, iw, s_in);
  __syncthreads();
  const int npx = tch * tcw, pxpad = (npx + 63) & ~63;      // a wave's 64 items share their output channel
  const int items = a.Cout * pxpad;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int co = __builtin_amdgcn_readfirstlane(it / pxpad);
    const int p = it - co * pxpad;
    if (p < npx) {
      const int cy = p / tcw, cx = p - cy * tcw;
      const float* wp = a.w + (size_t)co * a.Cin * K * K;
      float acc = 0.f;
      for (int ci = 0; ci < a.Cin; ++ci) {
        const float* ip = s_in + (ci * ih + cy) * iw + cx;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
          for (int kx = 0; kx < K; ++kx) acc = fmaf(ip[ky * iw + kx], wp[(ci * K + ky) * K + kx], acc);
      }
      acc += a.bias[co];
      if (a.keep) acc *= a.keep[(size_t)n * a.Cout + co];
      s_cv[(co * tch + cy) * tcw + cx] = acc;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < toh * tow * a.Cout; e += 256) {
    const int co = e % a.Cout, q = e / a.Cout, py = q / tow, px = q - py * tow;
    float best;
    int bi = 0;
    if (a.k) {
      best = -INFINITY;
      for (int j = 0; j < a.k * a.k; ++j) {
        const int dy = j / a.k, dx = j - dy * a.k;
        const float v = s_cv[(co * tch + py * 2 + dy) * tcw + px * 2 + dx];
        if (v > best || v != v) { best = v; bi = j; }
      }
    } else {
      best = s_cv[(co * tch + py) * tcw + px];
    }
    if (a.relu) best = best > 0.f ? best : 0.f;
    if (a.out) a.out[bnn_out_index(a, n, oy0 + py, ox0 + px, co)] = best;
    if (a.arg) a.arg[(((size_t)n * a.Ho + oy0 + py) * a.Wo + ox0 + px) * a.Cout + co] = (uint8_t)bi;
    if (a.label) s_in[e] = best;      // (the input region is dead behind the barrier above; e = q * Cout + co < 256)
  }
  if (a.label) {      // the FIRST maximum over the output channels of the values this launch would store; a NaN never wins
    __syncthreads();
    for (int q = threadIdx.x; q < toh * tow; q += 256) {
      float best = -INFINITY;
      int bi = 0;
      for (int co = 0; co < a.Cout; ++co)
        if (s_in[q * a.Cout + co] > best) { best = s_in[q * a.Cout + co]; bi = co; }
      const int py = q / tow, px = q - py * tow;
      a.label[((size_t)n * a.Ho + oy0 + py) * a.Wo + ox0 + px] = (uint8_t)bi;
    }
  }
}

// dconv[n,y,x,c] = keep[n,c] * sum over the <= 4 windows containing (y,x) of [arg(window,c) is this pixel] * [out > 0] * dout (window
// order: py, then px ascending); then dx = conv^T(dconv) for the tile's input pixels, and the tile's share of dW / db as one partial row
// [Cout*Cin*K*K + Cout] of the workspace.  Dynamic LDS: dconv region [Cout][R][R] then input region [Cin][R][R], R = T + K - 1.
template <int K>
__global__ __launch_bounds__(256) void bnn_stage_bwd_kernel(BnnStage a) {
  extern __shared__ __align__(16) float s_dyn[];
  const int T = a.T, R = T + K - 1;
  float* s_d = s_dyn;
  float* s_x = s_dyn + a.Cout * R * R;
  const int b = blockIdx.x;
  const int tx = b % a.tiles_x, ty = (b / a.tiles_x) % a.tiles_y, n = b / (a.tiles_x * a.tiles_y);
  const int y0 = ty * T, x0 = tx * T;
  const int k = a.k;
  for (int e = threadIdx.x; e < a.Cout * R * R; e += 256) {
    const int co = e % a.Cout, r = e / a.Cout, ry = r / R, rx = r - ry * R;
    const int cy = y0 + a.P - (K - 1) + ry, cx = x0 + a.P - (K - 1) + rx;
    float v = 0.f;
    if (cy >= 0 && cy < a.Hc && cx >= 0 && cx < a.Wc) {
      if (k == 0) {
        const size_t o = bnn_out_index(a, n, cy, cx, co);
        v = a.dout[o];
        if (a.relu && !(a.out_c[o] > 0.f)) v = 0.f;
      } else {
        const int py_lo = max(0, (cy - k + 2) >> 1), py_hi = min(a.Ho - 1, cy >> 1);
        const int px_lo = max(0, (cx - k + 2) >> 1), px_hi = min(a.Wo - 1, cx >> 1);
        for (int py = py_lo; py <= py_hi; ++py)
          for (int px = px_lo; px <= px_hi; ++px) {
            const size_t o = bnn_out_index(a, n, py, px, co);
            const int mine = (cy - 2 * py) * k + (cx - 2 * px);
            const bool hit = (int)a.arg_c[(((size_t)n * a.Ho + py) * a.Wo + px) * a.Cout + co] == mine && (!a.relu || a.out_c[o] > 0.f);
            if (hit) v += a.dout[o];
          }
      }
      if (a.keep) v *= a.keep[(size_t)n * a.Cout + co];
    }
    s_d[(co * R + ry) * R + rx] = v;
  }
  bnn_stage_input(a, n, y0 - a.P, x0 - a.P, R, R, s_x);
  __syncthreads();
  if (a.dx) {
    const int thi = min(T, a.H - y0), twi = min(T, a.W - x0);
    const int TT = T * T;      // a multiple of 64: a wave's items share their input channel
    for (int it = threadIdx.x; it < a.Cin * TT; it += 256) {
      const int ci = __builtin_amdgcn_readfirstlane(it / TT);
      const int p = it - ci * TT, iy = p / T, ix = p - iy * T;
      if (iy < thi && ix < twi) {
        float acc = 0.f;
        for (int co = 0; co < a.Cout; ++co) {
          const float* wp = a.w + ((size_t)co * a.Cin + ci) * K * K;
          const float* dp = s_d + (co * R + iy + K - 1) * R + ix + K - 1;
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc = fmaf(dp[-ky * R - kx], wp[ky * K + kx], acc);
        }
        a.dx[(((size_t)n * a.H + y0 + iy) * a.W + x0 + ix) * a.Cin + ci] = acc;
      }
    }
  }
  const int thc = max(0, min(T, a.Hc - y0)), twc = max(0, min(T, a.Wc - x0));
  const int nW = a.Cout * a.Cin * K * K;
  float* row = a.part + (size_t)b * a.row_width;
  const int off = K - 1 - a.P;
  for (int e = threadIdx.x; e < nW; e += 256) {
    const int kx = e % K, ky = (e / K) % K, ci = (e / (K * K)) % a.Cin, co = e / (K * K * a.Cin);
    const float* dp = s_d + (co * R + off) * R + off;
    const float* xp = s_x + (ci * R + ky) * R + kx;
    float acc = 0.f;
    for (int y = 0; y < thc; ++y)
      for (int x = 0; x < twc; ++x) acc = fmaf(dp[y * R + x], xp[y * R + x], acc);
    row[e] = acc;
  }
  if ((int)threadIdx.x < a.Cout) {
    const float* dp = s_d + (threadIdx.x * R + off) * R + off;
    float acc = 0.f;
    for (int y = 0; y < thc; ++y)
      for (int x = 0; x < twc; ++x) acc += dp[y * R + x];
    row[nW + threadIdx.x] = acc;
  }
}

// out[e] = sum over rows of part[row][e]: four interleaved row groups summed in row order each, combined as (g0 + g1) + (g2 + g3);
// element e belongs to the first segment whose running length exceeds it
struct BnnReduce {
  const float* part;
  int rows, width;
  float* out[4];
  int len[4];
};
__global__ __launch_bounds__(256) void bnn_rows_reduce_kernel(BnnReduce a) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  float acc = 0.f;
  if (e < a.width)
    for (int r = g; r < a.rows; r += 4) acc += a.part[(size_t)r * a.width + e];
  sh[g][lane] = acc;
  __syncthreads();
  if (g == 0 && e < a.width) {
    const float s = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
    int o = e;
    for (int q = 0; q < 4; ++q) {
      if (o < a.len[q]) { if (a.out[q]) a.out[q][o] = s; break; }
      o -= a.len[q];
    }
  }
}

// BNN-L's head, model.py:593: logits = Wc relu((Wfc x + bfc) * keep) + bc per pixel of the head plane; keep = NULL in eval mode
struct BnnHead {
  const float* x; const float* wfc; const float* bfc; const float* keep; const float* wc; const float* bc;
  const float* dl;
  float* logits; uint8_t* argmax; float* dx; float* part;
  int M, HW, nC, MB, row_width;
};

__device__ __forceinline__ float bnn_hidden(const BnnHead& a, const float* x, int m, int j) {
  const float4* wr = reinterpret_cast<const float4*>(a.wfc + (size_t)j * 16);
  float z = a.bfc[j];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 wv = wr[q];
    z = fmaf(x[4 * q], wv.x, z); z = fmaf(x[4 * q + 1], wv.y, z); z = fmaf(x[4 * q + 2], wv.z, z); z = fmaf(x[4 * q + 3], wv.w, z);
  }
  if (a.keep) z *= a.keep[(size_t)m * BNN_HID + j];
  return z;
}

__global__ __launch_bounds__(256) void bnn_head_fwd_kernel(BnnHead a) {
  __shared__ float sh[BNN_MAX_OUT][256];
  __shared__ float sh2[BNN_MAX_OUT][16];
  __shared__ float s_l[BNN_MAX_OUT];
  const int m = blockIdx.x, t = threadIdx.x;
  float x[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(a.x + (size_t)m * 16 + 4 * q);
    x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
  }
  const float z0 = bnn_hidden(a, x, m, t), z1 = bnn_hidden(a, x, m, t + 256);
  const float h0 = z0 > 0.f ? z0 : 0.f, h1 = z1 > 0.f ? z1 : 0.f;
  for (int o = 0; o < a.nC; ++o) sh[o][t] = fmaf(h1, a.wc[(size_t)o * BNN_HID + t + 256], h0 * a.wc[(size_t)o * BNN_HID + t]);
  __syncthreads();
  if (t < a.nC * 16) {
    const int o = t >> 4, seg = t & 15;
    float s = 0.f;
    for (int q = 0; q < 16; ++q) s += sh[o][seg * 16 + q];
    sh2[o][seg] = s;
  }
  __syncthreads();
  if (t < a.nC) {
    float s = 0.f;
    for (int q = 0; q < 16; ++q) s += sh2[t][q];
    s += a.bc[t];
    s_l[t] = s;
    if (a.logits) {
      const int n = m / a.HW, pp = m - n * a.HW;
      a.logits[((size_t)n * a.nC + t) * a.HW + pp] = s;
    }
  }
  __syncthreads();
  if (t == 0 && a.argmax) {      // the first maximum in class order; a NaN never wins (the rule of RCV_OP_CLS_LABEL)
    float best = -INFINITY;
    int bi = 0;
    for (int o = 0; o < a.nC; ++o)
      if (s_l[o] > best) { best = s_l[o]; bi = o; }
    a.argmax[m] = (uint8_t)bi;
  }
}

// a workgroup walks pixels [b*MB, (b+1)*MB) in order; partial row = [dWfc 512*16][dbfc 512][dWc nC*512][dbc nC]
__global__ __launch_bounds__(256) void bnn_head_bwd_kernel(BnnHead a) {
  __shared__ float sh[16][257];
  __shared__ float sh2[16][16];
  const int t = threadIdx.x, b = blockIdx.x;
  float dwfc[2][16], dbfc[2] = {0.f, 0.f}, dwc[2][BNN_MAX_OUT], dbc = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) { dwfc[0][i] = 0.f; dwfc[1][i] = 0.f; }
#pragma unroll
  for (int o = 0; o < BNN_MAX_OUT; ++o) { dwc[0][o] = 0.f; dwc[1][o] = 0.f; }
  const int m_end = min(a.M, (b + 1) * a.MB);
  for (int m = b * a.MB; m < m_end; ++m) {
    const int n = m / a.HW, pp = m - n * a.HW;
    float x[16], dl[BNN_MAX_OUT], pi[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(a.x + (size_t)m * 16 + 4 * q);
      x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int o = 0; o < BNN_MAX_OUT; ++o) dl[o] = o < a.nC ? a.dl[((size_t)n * a.nC + o) * a.HW + pp] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) pi[i] = 0.f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = t + 256 * jj;
      const float z = bnn_hidden(a, x, m, j);
      const float h = z > 0.f ? z : 0.f;
      float dh = 0.f;
#pragma unroll
      for (int o = 0; o < BNN_MAX_OUT; ++o)
        if (o < a.nC) { dh = fmaf(dl[o], a.wc[(size_t)o * BNN_HID + j], dh); dwc[jj][o] = fmaf(dl[o], h, dwc[jj][o]); }
      float dz = z > 0.f ? dh : 0.f;
      if (a.keep) dz *= a.keep[(size_t)m * BNN_HID + j];
      dbfc[jj] += dz;
      const float4* wr = reinterpret_cast<const float4*>(a.wfc + (size_t)j * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 wv = wr[q];
        pi[4 * q] = fmaf(dz, wv.x, pi[4 * q]); pi[4 * q + 1] = fmaf(dz, wv.y, pi[4 * q + 1]);
        pi[4 * q + 2] = fmaf(dz, wv.z, pi[4 * q + 2]); pi[4 * q + 3] = fmaf(dz, wv.w, pi[4 * q + 3]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) dwfc[jj][i] = fmaf(dz, x[i], dwfc[jj][i]);
    }
    if (t < a.nC) dbc += a.dl[((size_t)n * a.nC + t) * a.HW + pp];
    __syncthreads();                 // the previous pixel's readers are done
#pragma unroll
    for (int i = 0; i < 16; ++i) sh[i][t] = pi[i];
    __syncthreads();
    {
      const int i = t >> 4, seg = t & 15;
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += sh[i][seg * 16 + q];
      sh2[i][seg] = s;
    }
    __syncthreads();
    if (t < 16) {
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += sh2[t][q];
      a.dx[(size_t)m * 16 + t] = s;
    }
  }
  float* row = a.part + (size_t)b * a.row_width;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int j = t + 256 * jj;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(row + (size_t)j * 16 + 4 * q) = make_float4(dwfc[jj][4 * q], dwfc[jj][4 * q + 1], dwfc[jj][4 * q + 2], dwfc[jj][4 * q + 3]);
    row[BNN_HID * 16 + j] = dbfc[jj];
#pragma unroll
    for (int o = 0; o < BNN_MAX_OUT; ++o)
      if (o < a.nC) row[BNN_HID * 17 + o * BNN_HID + j] = dwc[jj][o];
  }
  if (t < a.nC) row[BNN_HID * 17 + a.nC * BNN_HID + t] = dbc;
}

// --------------------------------------------------------------------------------------------
// launcher.  Stage records (RCV_OP_BNN_STAGE_FWD / _BWD):
//   i: N, H, W = input plane; CIN, COUT; AUX0 = K (3 / 5 / 8); COUNT = padding P (0 / 1 / 3 / 4); AUX1 = pool k (0 / 2 / 4; stride 2);
//      HO, WO = output plane; INMODE = RCV_LOAD_NCHW (the network input, 3 channels: no data gradient) or RCV_LOAD_PLAIN (NHWC);
//      flags: RCV_F_RELU, RCV_F_OUT_NCHW (output / its gradient NCHW: the logits of BNN-M-C's classifier)
//   p: forward  -- IN = x, W = filter [COUT][CIN][K][K] (parameter layout), BIAS, X0 = keep-scale float[N][COUT] or NULL, OUT,
//                  X1 = arg-max bytes uint8[N][HO][WO][COUT] or NULL (pooled stages that will not run backward), X2 = uint8[N][HO][WO]
//                  first maximum over the output channels or NULL (the class map of BNN-M-C's classifier; OUT may then be NULL)
//      backward -- IN = d loss / d out, IN_AUX = out (read with RCV_F_RELU), X1 = arg-max bytes (pooled), X0, W as the forward,
//                  EPI_AUX = x, OUT = dx NHWC (RCV_LOAD_PLAIN only), X2 = dW, X3 = db, PART = NPART rows of COUT*CIN*K*K + COUT floats
// Head records (RCV_OP_BNN_HEAD_FWD / _BWD): i: N, H, W = head plane, CIN = 16, COUT = 1..8 classes, COUNT = 512 hidden units
//   p: forward  -- IN = x NHWC, W = fc weight [512][16], BIAS = fc bias, X0 = keep-scale float[N][H][W][512] or NULL, X1 = classifier
//                  weight [COUT][512], X2 = its bias, OUT = NCHW logits or NULL, X3 = uint8 arg-max [N][H][W] or NULL (one of the two)
//      backward -- IN = NCHW logits gradient, EPI_AUX = x, W, BIAS, X0, X1 as the forward, OUT = dx NHWC, X2 = dWfc, X3 = dbfc,
//                  X4 = dWc, X5 = dbc, PART = NPART rows of 512*17 + COUT*513 floats (rounded up to 4)
// Every refusal that depends on the shape of the record sits in front of the query return.
// --------------------------------------------------------------------------------------------
static int bnn_launch_reduce(const BnnReduce& r, hipStream_t s) {
  hipLaunchKernelGGL(bnn_rows_reduce_kernel, dim3(ceil_div(r.width, 64)), dim3(256), 0, s, r);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

static int bnn_launch_head(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const bool fwd = op->kind == RCV_OP_BNN_HEAD_FWD;
  const char* what = fwd ? "bnn head forward" : "bnn head backward";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_CIN], nC = op->i[RCV_I_COUT];
  RCV_CHECK_ARG(C == 16, "%s: %d input channels unsupported (16)", what, C);
  RCV_CHECK_ARG(op->i[RCV_I_COUNT] == BNN_HID, "%s: %d hidden units unsupported (%d)", what, op->i[RCV_I_COUNT], BNN_HID);
  RCV_CHECK_ARG(nC >= 1 && nC <= BNN_MAX_OUT, "%s: %d classes unsupported (1..%d)", what, nC, BNN_MAX_OUT);
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * H * W * BNN_HID < 2147483647.0, "%s: plane %dx%d (batch %d) out of range", what, H, W, N);
  const int M = N * H * W;
  const int MB = ceil_div(M, 256), rows = ceil_div(M, MB);
  const int width = round_up(BNN_HID * 17 + nC * (BNN_HID + 1), 4);      // rows stay 16-byte aligned
  if (query) {
    snprintf(query->label, sizeof(query->label), fwd ? "bnn_head_fwd<%d>" : "bnn_head_bwd<%d>", nC);
    if (!fwd) { query->n_part = rows; query->part_bytes = (size_t)rows * width * sizeof(float); }
    return RCV_OK;
  }
  BnnHead a;
  memset(&a, 0, sizeof(a));
  a.x = (const float*)op->p[fwd ? RCV_P_IN : RCV_P_EPI_AUX];
  a.wfc = (const float*)op->p[RCV_P_W]; a.bfc = (const float*)op->p[RCV_P_BIAS]; a.keep = (const float*)op->p[RCV_P_X0];
  a.wc = (const float*)op->p[RCV_P_X1];
  a.M = M; a.HW = H * W; a.nC = nC; a.MB = MB; a.row_width = width;
  RCV_CHECK_ARG(a.x && a.wfc && a.bfc && a.wc, "%s: null operand", what);
  RCV_CHECK_ARG((((uintptr_t)a.x | (uintptr_t)a.wfc) & 15) == 0, "%s: input / fc weight not 16-byte aligned", what);
  if (fwd) {
    a.bc = (const float*)op->p[RCV_P_X2]; a.logits = (float*)op->p[RCV_P_OUT]; a.argmax = (uint8_t*)op->p[RCV_P_X3];
    RCV_CHECK_ARG(a.bc && (a.logits || a.argmax), "%s: classifier bias or both outputs missing", what);
    hipLaunchKernelGGL(bnn_head_fwd_kernel, dim3(M), dim3(256), 0, s, a);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  a.dl = (const float*)op->p[RCV_P_IN]; a.dx = (float*)op->p[RCV_P_OUT]; a.part = (float*)op->p[RCV_P_PART];
  RCV_CHECK_ARG(a.dl && a.dx && op->p[RCV_P_X2] && op->p[RCV_P_X3] && op->p[RCV_P_X4] && op->p[RCV_P_X5], "%s: null operand", what);
  RCV_CHECK_ARG(a.part && ((uintptr_t)a.part & 15) == 0 && op->i[RCV_I_NPART] == rows, "%s: workspace missing, unaligned or rows mismatch (%d given, %d expected)",
                what, op->i[RCV_I_NPART], rows);
  hipLaunchKernelGGL(bnn_head_bwd_kernel, dim3(rows), dim3(256), 0, s, a);
  RCV_HIP(hipGetLastError());
  BnnReduce r;
  r.part = a.part; r.rows = rows; r.width = width;
  r.out[0] = (float*)op->p[RCV_P_X2]; r.len[0] = BNN_HID * 16;
  r.out[1] = (float*)op->p[RCV_P_X3]; r.len[1] = BNN_HID;
  r.out[2] = (float*)op->p[RCV_P_X4]; r.len[2] = nC * BNN_HID;
  r.out[3] = (float*)op->p[RCV_P_X5]; r.len[3] = nC;
  return bnn_launch_reduce(r, s);
}

int rcv_launch_bnn(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (op->kind == RCV_OP_BNN_HEAD_FWD || op->kind == RCV_OP_BNN_HEAD_BWD) return bnn_launch_head(h, op, s, query);
  const bool fwd = op->kind == RCV_OP_BNN_STAGE_FWD;
  const char* what = fwd ? "bnn stage forward" : "bnn stage backward";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int K = op->i[RCV_I_AUX0], k = op->i[RCV_I_AUX1], P = op->i[RCV_I_COUNT], mode = op->i[RCV_I_INMODE];
  RCV_CHECK_ARG(K == 3 || K == 5 || K == 8, "%s: filter size %d unsupported (3, 5 or 8)", what, K);
  RCV_CHECK_ARG(k == 0 || k == 2 || k == 4, "%s: pool size %d unsupported (0 = none, 2 or 4 at stride 2)", what, k);
  RCV_CHECK_ARG((P == 0 || P == 1 || P == 3 || P == 4) && P < K, "%s: padding %d unsupported for a %dx%d filter (0, 1, 3 or 4, below the filter size)", what, P, K, K);
  RCV_CHECK_ARG(mode == RCV_LOAD_NCHW || mode == RCV_LOAD_PLAIN, "%s: load mode %d unsupported (RCV_LOAD_NCHW or RCV_LOAD_PLAIN)", what, mode);
  RCV_CHECK_ARG(mode == RCV_LOAD_NCHW ? Cin == 3 : (Cin == 8 || Cin == 16), "%s: %d input channels unsupported (3 for the NCHW network input, 8 or 16 NHWC)",
                what, Cin);
  RCV_CHECK_ARG(Cout == 4 || Cout == 8 || Cout == 16, "%s: %d output channels unsupported (4, 8 or 16)", what, Cout);
  const uint32_t allowed = RCV_F_SIDE_STREAM | RCV_F_RELU | RCV_F_OUT_NCHW;
  RCV_CHECK_ARG((op->flags & ~allowed) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~allowed);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (double)N * (H + 2 * P) * (W + 2 * P) * 16 < 2147483647.0, "%s: plane %dx%d (batch %d) out of range", what, H, W, N);
  const int Hc = H + 2 * P - K + 1, Wc = W + 2 * P - K + 1;
  const int need = k ? k : 1;
  RCV_CHECK_ARG(Hc >= need && Wc >= need, "%s: a %dx%d plane is too small for a %dx%d filter at padding %d and a %dx%d pool window", what, H, W, K, K, P, need, need);
  const int Ho = k ? (Hc - k) / 2 + 1 : Hc, Wo = k ? (Wc - k) / 2 + 1 : Wc;
  RCV_CHECK_ARG(op->i[RCV_I_HO] == Ho && op->i[RCV_I_WO] == Wo, "%s: output plane %dx%d given, %dx%d expected", what, op->i[RCV_I_HO], op->i[RCV_I_WO], Ho, Wo);
  // Backward tile: 8 x 8 where a data gradient is formed (its work items need T * T to be a multiple of 64).  The 3-channel first
  // stage forms none, so its tile may have any size: the plane's longer side E (input or conv plane, whichever is larger) is cut
  // into round(E / 16) equal parts -- a 33 x 33 conv plane gives 2 x 2 tiles of 17 where fixed 16 x 16 tiles gave 3 x 3 with five
  // one-pixel slivers, each a full partial row for the reduction to read; 16 where the LDS tile would pass 64 KB (T <= 23)
  int T = 8;
  if (Cin == 3) {
    const int E = std::max(std::max(H, Hc), std::max(W, Wc));
    T = ceil_div(E, std::max(1, (E + 8) / 16));
    if ((size_t)(Cin + Cout) * (T + K - 1) * (T + K - 1) * sizeof(float) > 64 * 1024) T = 16;
  }
  const int tiles_y = fwd ? ceil_div(Ho, BNN_TP) : ceil_div(H > Hc ? H : Hc, T), tiles_x = fwd ? ceil_div(Wo, BNN_TP) : ceil_div(W > Wc ? W : Wc, T);
  RCV_CHECK_ARG((double)N * tiles_y * tiles_x < 2147483647.0, "%s: too many tiles", what);
  const int rows = N * tiles_y * tiles_x, width = Cout * Cin * K * K + Cout;
  if (query) {
    snprintf(query->label, sizeof(query->label), fwd ? "bnn_stage_fwd<%d,%d,%d>" : "bnn_stage_bwd<%d,%d,%d>", K, k, fwd ? BNN_TP : T);
    if (!fwd) { query->n_part = rows; query->part_bytes = (size_t)rows * width * sizeof(float); }
    return RCV_OK;
  }
  BnnStage a;
  memset(&a, 0, sizeof(a));
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.P = P; a.k = k; a.Hc = Hc; a.Wc = Wc; a.Ho = Ho; a.Wo = Wo; a.T = T;
  a.tiles_y = tiles_y; a.tiles_x = tiles_x; a.nchw_in = mode == RCV_LOAD_NCHW; a.relu = (op->flags & RCV_F_RELU) != 0;
  a.nchw_out = (op->flags & RCV_F_OUT_NCHW) != 0; a.row_width = width;
  a.w = (const float*)op->p[RCV_P_W]; a.keep = (const float*)op->p[RCV_P_X0];
  if (fwd) {
    a.x = (const float*)op->p[RCV_P_IN]; a.bias = (const float*)op->p[RCV_P_BIAS]; a.out = (float*)op->p[RCV_P_OUT]; a.arg = (uint8_t*)op->p[RCV_P_X1];
    a.label = (uint8_t*)op->p[RCV_P_X2];
    RCV_CHECK_ARG(a.x && a.w && a.bias && (a.out || a.label), "%s: null operand", what);
    auto kern = K == 3 ? bnn_stage_fwd_kernel<3> : (K == 5 ? bnn_stage_fwd_kernel<5> : bnn_stage_fwd_kernel<8>);
    hipLaunchKernelGGL(kern, dim3(rows), dim3(256), 0, s, a);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  a.x = (const float*)op->p[RCV_P_EPI_AUX]; a.dout = (const float*)op->p[RCV_P_IN]; a.out_c = (const float*)op->p[RCV_P_IN_AUX];
  a.arg_c = (const uint8_t*)op->p[RCV_P_X1]; a.dx = (float*)op->p[RCV_P_OUT]; a.part = (float*)op->p[RCV_P_PART];
  RCV_CHECK_ARG(a.x && a.w && a.dout && op->p[RCV_P_X2] && op->p[RCV_P_X3], "%s: null operand", what);
  RCV_CHECK_ARG(!a.relu || a.out_c, "%s: RCV_F_RELU without the forward output (p[IN_AUX])", what);
  RCV_CHECK_ARG(k == 0 || a.arg_c, "%s: arg-max bytes (p[X1]) missing", what);
  RCV_CHECK_ARG(a.nchw_in ? a.dx == nullptr : a.dx != nullptr, "%s: the data gradient (p[OUT]) is produced for an NHWC input and only for it", what);
  RCV_CHECK_ARG(a.part && op->i[RCV_I_NPART] == rows, "%s: workspace missing or rows mismatch (%d given, %d expected)", what, op->i[RCV_I_NPART], rows);
  const int R = T + K - 1;
  const size_t lds = (size_t)(Cin + Cout) * R * R * sizeof(float);      // at most 64 KB (checked below)
  RCV_CHECK_ARG(lds <= 64 * 1024, "%s: tile needs %zu bytes of LDS", what, lds);
  auto kern = K == 3 ? bnn_stage_bwd_kernel<3> : (K == 5 ? bnn_stage_bwd_kernel<5> : bnn_stage_bwd_kernel<8>);
  hipLaunchKernelGGL(kern, dim3(rows), dim3(256), lds, s, a);
  RCV_HIP(hipGetLastError());
  BnnReduce r;
  memset(&r, 0, sizeof(r));
  r.part = a.part; r.rows = rows; r.width = width;
  r.out[0] = (float*)op->p[RCV_P_X2]; r.len[0] = width - Cout;
  r.out[1] = (float*)op->p[RCV_P_X3]; r.len[1] = Cout;
  return bnn_launch_reduce(r, s);
}
