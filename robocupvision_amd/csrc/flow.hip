// RCV_OP_FARNEBACK / RCV_OP_REMAP_LABELS: label propagation by dense optical flow (test.py:135-140 --lProp; transform.py:185-187 optFlow =
// cv2.calcOpticalFlowFarneback(pyr_scale .5, levels 2, winsize 15, iterations 2, poly_n 7, poly_sigma 1.5, flags 0); transform.py:189-198
// updateLabels = cv2.remap(INTER_NEAREST, BORDER_CONSTANT 0) through pixel + flow), DESIGN §4.11.  The contract is
// tests/farneback_restatement.py; every kernel below names the function of that file it computes.
//
// Per plane, coarsest first (B pairs, plane h x w; the batch is the grid's outer dimension):
//   image     gray on load (uint8, or RGB -> (4899 R + 9617 G + 1868 B + 8192) >> 14), separable blur with reflect-101 borders and the
//             pixel-centre bilinear resize of both frames, gathered per output pixel (a form of its own for the 3-tap blurs of
//             planes 0 and 1)                                                                                 -> img [2][B][h][w]
//   polyexp   32x16 tile + poly_n halo in LDS, replicated borders; vertical pass (g, j g, j^2 g) into LDS, horizontal pass, the
//             inverse normal matrix                                                                               -> R [2][B][5][h][w]
//   init      flow = 2 x bilinear resize of the coarser plane's flow (0 on the coarsest), M = matrices(flow)      -> flow, M[0]
//   iterate   (x iterations) 32x16 tile + winsize/2 halo of the five planes of M in LDS, replicated borders; vertical sums, horizontal
//             sums, 2x2 solve -> flow; all but the last rebuild M from the new flow at the same pixel              -> flow, M[1 - cur]
// The last iterate of plane 0 writes the caller's flow tensor.  fp32 on the vector ALU throughout; every window is summed directly in tap
// order (top to bottom, then left to right): no running sums, no atomics, so a pixel's value does not depend on the tile it falls in, on its
// position in the batch or on the run.  The filter taps and the inverse normal matrix are formed on the host in double.
#include <math.h>
#include "rcv_internal.h"

namespace {

constexpr int FL_TX = 32, FL_TY = 16, FL_THREADS = 256;
constexpr int FL_MAXR = 7;                                // widest halo: poly_n = 7, winsize = 15
constexpr int FL_LW = FL_TX + 2 * FL_MAXR + 1;            // LDS row pitch (47: odd, rows fall into different banks)
constexpr int FL_MAXPLANES = 5;                           // full resolution + 4 coarser planes (a 512-pixel short side)
constexpr int FL_MAXBLUR = 19;                            // blur radius of a plane image: 1 on planes 0 and 1, then 4, 9, 19 (round(5 sigma) | 1 taps)
constexpr int FL_MIN_SIZE = 32;

struct FlowPoly {
  float g[2 * FL_MAXR + 1], xg[2 * FL_MAXR + 1], xxg[2 * FL_MAXR + 1];
  float ibx, iby, ixy;          // b_x = ibx m_x, b_y = iby m_y, a_xy = ixy m_xy
  float ixx[3], iyy[3];         // a_xx = ixx . (m_1, m_xx, m_yy), a_yy likewise
};

struct FlowBlur {
  float k[2 * FL_MAXBLUR + 1];
  int r;
};

struct FlowPlane {
  int h, w;
  size_t img, R, M, flow;       // float offsets into the workspace; M holds two buffers; flow of plane 0 is the caller's tensor
};

struct FlowPlan {
  int n_planes;
  FlowPlane pl[FL_MAXPLANES];
  size_t floats;
};

static inline size_t fl_align(size_t floats) { return (floats + 63) & ~(size_t)63; }

// Python's round(): half to even
static inline int fl_round_even(double v) { return (int)nearbyint(v); }

static void fl_plan(int B, int H, int W, int levels, FlowPlan* p) {
  int k = 0;
  double s = 1.0;
  while (k < levels) {
    s *= 0.5;
    if (W * s < FL_MIN_SIZE || H * s < FL_MIN_SIZE) break;
    ++k;
  }
  p->n_planes = k + 1;
  size_t off = 0;
  s = 1.0;
  for (int j = 0; j <= k; ++j, s *= 0.5) {
    FlowPlane& q = p->pl[j];
    q.h = fl_round_even(H * s); q.w = fl_round_even(W * s);
    const size_t hw = (size_t)q.h * q.w;
    q.img = off; off += fl_align(2 * (size_t)B * hw);
    q.R = off; off += fl_align(10 * (size_t)B * hw);
    q.M = off; off += 2 * fl_align(5 * (size_t)B * hw);
    q.flow = off; if (j) off += fl_align(2 * (size_t)B * hw);
  }
  p->floats = off;
}

// ---- host constants (double, rounded once) -----------------------------------------------------------------------------------------
static void fl_blur_taps(int j, FlowBlur* b) {
  const double sigma = (1.0 / pow(0.5, j) - 1.0) / 2.0;
  memset(b, 0, sizeof(*b));
  if (sigma <= 0) { b->r = 1; b->k[0] = 0.25f; b->k[1] = 0.5f; b->k[2] = 0.25f; return; }
  int n = fl_round_even(5.0 * sigma) | 1;
  if (n < 3) n = 3;
  double k[2 * FL_MAXBLUR + 1], sum = 0;
  for (int t = 0; t < n; ++t) { const double x = t - (n - 1) / 2.0; k[t] = exp(-x * x / (2.0 * sigma * sigma)); sum += k[t]; }
  b->r = (n - 1) / 2;
  for (int t = 0; t < n; ++t) b->k[t] = (float)(k[t] / sum);
}

static void fl_poly_taps(int n, double sigma, FlowPoly* p) {
  memset(p, 0, sizeof(*p));
  double g[2 * FL_MAXR + 1], sum = 0;
  for (int t = 0; t <= 2 * n; ++t) { const double i = t - n; g[t] = exp(-i * i / (2.0 * sigma * sigma)); sum += g[t]; }
  double s2 = 0, s4 = 0;
  for (int t = 0; t <= 2 * n; ++t) {
    const double i = t - n;
    g[t] /= sum;
    p->g[t] = (float)g[t]; p->xg[t] = (float)(i * g[t]); p->xxg[t] = (float)(i * i * g[t]);
    s2 += g[t] * i * i; s4 += g[t] * i * i * i * i;
  }
  // the normal matrix over (1, i, j, i^2, j^2, ij) with weights g(i) g(j), sum g = 1: i, j and ij decouple (diagonal s2, s2, s2^2); the rest is
  // A = [[1, s2, s2], [s2, s4, s2^2], [s2, s2^2, s4]] over (1, i^2, j^2), inverted here by cofactors
  const double a = 1, b = s2, c = s4, d = s2 * s2;
  const double det = a * (c * c - d * d) - b * (b * c - d * b) + b * (b * d - c * b);
  const double i10 = -(b * c - d * b) / det, i11 = (a * c - b * b) / det, i12 = -(a * d - b * b) / det;
  p->ibx = (float)(1.0 / s2); p->iby = (float)(1.0 / s2); p->ixy = (float)(1.0 / (s2 * s2));
  p->ixx[0] = (float)i10; p->ixx[1] = (float)i11; p->ixx[2] = (float)i12;
  p->iyy[0] = (float)i10; p->iyy[1] = (float)i12; p->iyy[2] = (float)i11;
}

// ---- device helpers ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fl_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
__device__ __forceinline__ int fl_refl101(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

__device__ __forceinline__ float fl_gray(const uint8_t* __restrict__ src, int ch, size_t i) {
  if (ch == 1) return (float)src[i];
  const uint8_t* c = src + 3 * i;
  return (float)((4899 * (int)c[0] + 9617 * (int)c[1] + 1868 * (int)c[2] + 8192) >> 14);
}

// resize(): source coordinate of destination index d; i0 / i1 clamped, f the weight of i1
__device__ __forceinline__ void fl_src(int d, float ratio, int n_src, int* i0, int* i1, float* f) {
  const float s = ((float)d + 0.5f) * ratio - 0.5f;
  const float fl = floorf(s);
  *f = s - fl;
  const int i = (int)fl;
  *i0 = fl_clamp(i, n_src);
  *i1 = fl_clamp(i + 1, n_src);
}

// matrices(): M at pixel (x, y) of pair b from the expansions R0 / R1 (planar [5][h][w]) and the flow (dx, dy)
__device__ __forceinline__ void fl_matrices(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int x, int y, float dx,
                                            float dy, float* __restrict__ M) {
  const size_t hw = (size_t)h * w, at = (size_t)y * w + x;
  const float fx = (float)x + dx, fy = (float)y + dy;
  const float x1f = floorf(fx), y1f = floorf(fy);
  float r0[5], rw[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) r0[c] = R0[c * hw + at];
  if (x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1)) {      // false for NaN
    const float a = fx - x1f, b = fy - y1f;
    const size_t o = (size_t)(int)y1f * w + (int)x1f;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const float* r = R1 + c * hw + o;
      const float top = r[0] * (1.f - a) + r[1] * a;
      const float bot = r[w] * (1.f - a) + r[w + 1] * a;
      rw[c] = top * (1.f - b) + bot * b;
    }
  } else {
    rw[0] = 0.f; rw[1] = 0.f; rw[2] = r0[2]; rw[3] = r0[3]; rw[4] = r0[4];
  }
  float bx = (r0[0] - rw[0]) * 0.5f, by = (r0[1] - rw[1]) * 0.5f;
  float axx = (r0[2] + rw[2]) * 0.5f, ayy = (r0[3] + rw[3]) * 0.5f, axy = (r0[4] + rw[4]) * 0.25f;
  bx += axx * dx + axy * dy;
  by += axy * dx + ayy * dy;
  const int ex = min(x, w - 1 - x), ey = min(y, h - 1 - y);
  if (ex < 5 || ey < 5) {
    // the weight of a pixel d = 0..4 from an edge; 1 beyond.  Both edges of an axis count (planes narrower than 10)
    auto bw = [](int d) { return d >= 5 ? 1.f : (d >= 2 ? 0.4472f : 0.14f); };
    const float s = (bw(x) * bw(w - 1 - x)) * (bw(y) * bw(h - 1 - y));
    bx *= s; by *= s; axx *= s; ayy *= s; axy *= s;
  }
  M[0 * hw + at] = axx * axx + axy * axy;
  M[1 * hw + at] = (axx + ayy) * axy;
  M[2 * hw + at] = ayy * ayy + axy * axy;
  M[3 * hw + at] = axx * bx + axy * by;
  M[4 * hw + at] = axy * bx + ayy * by;
}

// ---- plane_image(): grid (ceil(hw / 256), 2B) --------------------------------------------------------------------------------------
__global__ __launch_bounds__(FL_THREADS) void flow_image_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ next, int ch,
                                                                 int B, int H, int W, int h, int w, float ry, float rx, FlowBlur kb,
                                                                 float* __restrict__ img) {
  const int at = blockIdx.x * FL_THREADS + threadIdx.x;
  if (at >= h * w) return;
  const int z = blockIdx.y, b = z % B;
  const uint8_t* src = (z < B ? prev : next) + (size_t)b * H * W * ch;
  const int y = at / w, x = at - y * w;
  int ys[2], xs[2];
  float fy, fx;
  fl_src(y, ry, H, &ys[0], &ys[1], &fy);
  fl_src(x, rx, W, &xs[0], &xs[1], &fx);
  float v[2][2];
  for (int cy = 0; cy < 2; ++cy)
    for (int cx = 0; cx < 2; ++cx) {
      // rows blurred first (the inner sum), then columns
      float acc = 0.f;
      for (int tj = 0; tj <= 2 * kb.r; ++tj) {
        const size_t row = (size_t)fl_refl101(ys[cy] + tj - kb.r, H) * W;
        float racc = 0.f;
        for (int ti = 0; ti <= 2 * kb.r; ++ti) racc += kb.k[ti] * fl_gray(src, ch, row + fl_refl101(xs[cx] + ti - kb.r, W));
        acc += kb.k[tj] * racc;
      }
      v[cy][cx] = acc;
    }
  const float top = v[0][0] * (1.f - fx) + v[0][1] * fx;
  const float bot = v[1][0] * (1.f - fx) + v[1][1] * fx;
  img[(size_t)z * h * w + at] = top * (1.f - fy) + bot * fy;
}

// plane_image() with a 3-tap blur (planes 0 and 1: every plane of the reference's parameters), same grid.  The four corners' 3x3 windows
// lie in one 4x4 patch of source pixels (3x3 where a clamped end makes two corners coincide): it is loaded once, the taps are in registers
// and every loop unrolls.  Each corner is summed in the order of the general kernel.
__global__ __launch_bounds__(FL_THREADS) void flow_image3_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ next, int ch,
                                                                  int B, int H, int W, int h, int w, float ry, float rx, float k0, float k1,
                                                                  float k2, float* __restrict__ img) {
  const int at = blockIdx.x * FL_THREADS + threadIdx.x;
  if (at >= h * w) return;
  const int z = blockIdx.y, b = z % B;
  const uint8_t* src = (z < B ? prev : next) + (size_t)b * H * W * ch;
  const int y = at / w, x = at - y * w;
  int ys[2], xs[2];
  float fy, fx;
  fl_src(y, ry, H, &ys[0], &ys[1], &fy);
  fl_src(x, rx, W, &xs[0], &xs[1], &fx);
  const bool dy = ys[1] != ys[0], dx = xs[1] != xs[0];      // the second corner is the next pixel, or (clamped) the same one
  const float k[3] = {k0, k1, k2};
  int cols[4];
  // (the clamp only guards the last row / column of the patch, which no corner uses where the end is clamped)
#pragma unroll
  for (int i = 0; i < 4; ++i) cols[i] = fl_clamp(fl_refl101(xs[0] - 1 + i, W), W);
  float hs[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t row = (size_t)fl_clamp(fl_refl101(ys[0] - 1 + j, H), H) * W;
    float g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = fl_gray(src, ch, row + cols[i]);
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      a0 += k[t] * g[t];
      a1 += k[t] * (dx ? g[t + 1] : g[t]);
    }
    hs[j][0] = a0; hs[j][1] = a1;
  }
  float v[2][2];
#pragma unroll
  for (int cx = 0; cx < 2; ++cx) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      a0 += k[t] * hs[t][cx];
      a1 += k[t] * (dy ? hs[t + 1][cx] : hs[t][cx]);
    }
    v[0][cx] = a0; v[1][cx] = a1;
  }
  const float top = v[0][0] * (1.f - fx) + v[0][1] * fx;
  const float bot = v[1][0] * (1.f - fx) + v[1][1] * fx;
  img[(size_t)z * h * w + at] = top * (1.f - fy) + bot * fy;
}

// ---- poly_exp(): grid (tiles_x, tiles_y, 2B) ---------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(FL_THREADS) void flow_polyexp_kernel(const float* __restrict__ img, int h, int w, FlowPoly kp,
                                                                   float* __restrict__ R) {
  constexpr int TW = FL_TX + 2 * N, TH = FL_TY + 2 * N;
  __shared__ float in[TH][FL_LW];
  __shared__ float vs[3][FL_TY][FL_LW];
  const int x0 = blockIdx.x * FL_TX, y0 = blockIdx.y * FL_TY, z = blockIdx.z;
  const size_t hw = (size_t)h * w;
  const float* src = img + (size_t)z * hw;
  for (int i = threadIdx.x; i < TH * TW; i += FL_THREADS) {
    const int ly = i / TW, lx = i - ly * TW;
    in[ly][lx] = src[(size_t)fl_clamp(y0 + ly - N, h) * w + fl_clamp(x0 + lx - N, w)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FL_TY * TW; i += FL_THREADS) {
    const int ly = i / TW, lx = i - ly * TW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * N; ++t) {
      const float v = in[ly + t][lx];
      s0 += kp.g[t] * v; s1 += kp.xg[t] * v; s2 += kp.xxg[t] * v;
    }
    vs[0][ly][lx] = s0; vs[1][ly][lx] = s1; vs[2][ly][lx] = s2;
  }
  __syncthreads();
  const int tx = threadIdx.x % FL_TX;
  for (int ty = threadIdx.x / FL_TX; ty < FL_TY; ty += FL_THREADS / FL_TX) {
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) continue;
    float m1 = 0.f, mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * N; ++t) {
      const float v0 = vs[0][ty][tx + t], v1 = vs[1][ty][tx + t], v2 = vs[2][ty][tx + t];
      m1 += kp.g[t] * v0; mx += kp.xg[t] * v0; mxx += kp.xxg[t] * v0;
      my += kp.g[t] * v1; mxy += kp.xg[t] * v1;
      myy += kp.g[t] * v2;
    }
    float* out = R + (size_t)z * 5 * hw + (size_t)y * w + x;
    out[0] = kp.ibx * mx;
    out[hw] = kp.iby * my;
    out[2 * hw] = kp.ixx[0] * m1 + kp.ixx[1] * mxx + kp.ixx[2] * myy;
    out[3 * hw] = kp.iyy[0] * m1 + kp.iyy[1] * mxx + kp.iyy[2] * myy;
    out[4 * hw] = kp.ixy * mxy;
  }
}

// ---- flow carried to the next plane, first matrices(): grid (ceil(hw / 256), B) --------------------------------------------------------
__global__ __launch_bounds__(FL_THREADS) void flow_init_kernel(const float* __restrict__ coarse, int hc, int wc, float ry, float rx,
                                                                const float* __restrict__ R, int B, int h, int w,
                                                                float* __restrict__ flow, float* __restrict__ M) {
  const int at = blockIdx.x * FL_THREADS + threadIdx.x;
  if (at >= h * w) return;
  const int b = blockIdx.y;
  const int y = at / w, x = at - y * w;
  const size_t hw = (size_t)h * w;
  float d[2] = {0.f, 0.f};
  if (coarse) {
    int ys[2], xs[2];
    float fy, fx;
    fl_src(y, ry, hc, &ys[0], &ys[1], &fy);
    fl_src(x, rx, wc, &xs[0], &xs[1], &fx);
    for (int c = 0; c < 2; ++c) {
      const float* p = coarse + ((size_t)b * 2 + c) * hc * wc;
      const float top = p[(size_t)ys[0] * wc + xs[0]] * (1.f - fx) + p[(size_t)ys[0] * wc + xs[1]] * fx;
      const float bot = p[(size_t)ys[1] * wc + xs[0]] * (1.f - fx) + p[(size_t)ys[1] * wc + xs[1]] * fx;
      d[c] = (top * (1.f - fy) + bot * fy) * 2.f;
    }
  }
  flow[((size_t)b * 2 + 0) * hw + at] = d[0];
  flow[((size_t)b * 2 + 1) * hw + at] = d[1];
  fl_matrices(R + (size_t)b * 5 * hw, R + (size_t)(B + b) * 5 * hw, h, w, x, y, d[0], d[1], M + (size_t)b * 5 * hw);
}

// ---- box_mean(), solve(), matrices(): grid (tiles_x, tiles_y, B) ---------------------------------------------------------------------
__global__ __launch_bounds__(FL_THREADS) void flow_iterate_kernel(const float* __restrict__ Min, const float* __restrict__ R, int B, int h,
                                                                   int w, int r, float inv_area, float* __restrict__ flow,
                                                                   float* __restrict__ Mout /* NULL: the last iteration */) {
  __shared__ float in[5][FL_TY + 2 * FL_MAXR][FL_LW];
  __shared__ float vs[5][FL_TY][FL_LW];
  const int TW = FL_TX + 2 * r, TH = FL_TY + 2 * r;
  const int x0 = blockIdx.x * FL_TX, y0 = blockIdx.y * FL_TY, b = blockIdx.z;
  const size_t hw = (size_t)h * w;
  const float* src = Min + (size_t)b * 5 * hw;
  for (int i = threadIdx.x; i < TH * TW; i += FL_THREADS) {
    const int ly = i / TW, lx = i - ly * TW;
    const size_t o = (size_t)fl_clamp(y0 + ly - r, h) * w + fl_clamp(x0 + lx - r, w);
#pragma unroll
    for (int c = 0; c < 5; ++c) in[c][ly][lx] = src[c * hw + o];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FL_TY * TW; i += FL_THREADS) {
    const int ly = i / TW, lx = i - ly * TW;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t <= 2 * r; ++t) {
#pragma unroll
      for (int c = 0; c < 5; ++c) s[c] += in[c][ly + t][lx];
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) vs[c][ly][lx] = s[c];
  }
  __syncthreads();
  const int tx = threadIdx.x % FL_TX;
  for (int ty = threadIdx.x / FL_TX; ty < FL_TY; ty += FL_THREADS / FL_TX) {
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) continue;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t <= 2 * r; ++t) {
#pragma unroll
      for (int c = 0; c < 5; ++c) s[c] += vs[c][ty][tx + t];
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] *= inv_area;
    const float idet = 1.f / (s[0] * s[2] - s[1] * s[1] + 1e-3f);
    const float dx = (s[2] * s[3] - s[1] * s[4]) * idet;
    const float dy = (s[0] * s[4] - s[1] * s[3]) * idet;
    const size_t at = (size_t)y * w + x;
    flow[((size_t)b * 2 + 0) * hw + at] = dx;
    flow[((size_t)b * 2 + 1) * hw + at] = dy;
    if (Mout) fl_matrices(R + (size_t)b * 5 * hw, R + (size_t)(B + b) * 5 * hw, h, w, x, y, dx, dy, Mout + (size_t)b * 5 * hw);
  }
}

// ---- update_labels(): grid (ceil(HW / 256), N) -------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(FL_THREADS) void flow_remap_kernel(const T* __restrict__ lab, const float* __restrict__ flow, int H, int W,
                                                                 T* __restrict__ out) {
  const int at = blockIdx.x * FL_THREADS + threadIdx.x;
  if (at >= H * W) return;
  const size_t hw = (size_t)H * W, n = blockIdx.y;
  const int y = at / W, x = at - y * W;
  const float sx = rintf((float)x + flow[(n * 2 + 0) * hw + at]);      // rintf: half to even, as the contract's round()
  const float sy = rintf((float)y + flow[(n * 2 + 1) * hw + at]);
  T v = 0;
  if (sx >= 0.f && sx < (float)W && sy >= 0.f && sy < (float)H) v = lab[n * hw + (size_t)(int)sy * W + (int)sx];      // false for NaN
  out[n * hw + at] = v;
}

}  // namespace

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_FARNEBACK).  Record:
//   i: N = B pairs, H, W; CIN = bytes per pixel of the frames (1 = gray, 3 = RGB); COUNT = levels; AUX0 = winsize; AUX1 = iterations;
//      STRIDE = poly_n; DIL = cv2's flags word (0 only); NPART = workspace size in 256-byte units (filled by the query)
//   f: [0] = pyr_scale (0.5 only), [1] = poly_sigma
//   p: IN = prev uint8 [B][H][W](x3), IN2 = next, OUT = flow float [B][2][H][W], PART = workspace
// Every refusal that depends on the record's parameters sits in front of the query return.
// --------------------------------------------------------------------------------------------
static int rcv_launch_farneback(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "farneback";
  const int B = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], ch = op->i[RCV_I_CIN], levels = op->i[RCV_I_COUNT];
  const int winsize = op->i[RCV_I_AUX0], iters = op->i[RCV_I_AUX1], poly_n = op->i[RCV_I_STRIDE], cvflags = op->i[RCV_I_DIL];
  const float pyr_scale = op->f[0], poly_sigma = op->f[1];
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(cvflags == 0, "%s: OpenCV flags %d unsupported (0 only: no initial flow, no Gaussian window)", what, cvflags);
  RCV_CHECK_ARG(pyr_scale == 0.5f, "%s: pyr_scale %g unsupported (0.5 only)", what, (double)pyr_scale);
  RCV_CHECK_ARG(levels >= 0 && levels < FL_MAXPLANES, "%s: levels %d unsupported (0..%d)", what, levels, FL_MAXPLANES - 1);
  RCV_CHECK_ARG(winsize >= 1 && winsize <= 2 * FL_MAXR + 1 && (winsize & 1), "%s: winsize %d unsupported (odd, 1..%d)", what, winsize,
                2 * FL_MAXR + 1);
  RCV_CHECK_ARG(iters >= 1 && iters <= 64, "%s: iterations %d unsupported (1..64)", what, iters);
  RCV_CHECK_ARG(poly_n == 5 || poly_n == 7, "%s: poly_n %d unsupported (5 or 7)", what, poly_n);
  RCV_CHECK_ARG(isfinite(poly_sigma) && poly_sigma >= 0.1f && poly_sigma <= 100.f, "%s: poly_sigma %g unsupported (0.1..100)", what,
                (double)poly_sigma);
  RCV_CHECK_ARG(ch == 1 || ch == 3, "%s: %d bytes per pixel unsupported (1 = gray, 3 = RGB)", what, ch);
  RCV_CHECK_ARG(B >= 1 && B <= 32767 && H >= 2 && W >= 2 && H <= 8192 && W <= 8192, "%s: batch %d of %dx%d planes out of range", what, B, H, W);
  FlowPlan plan;
  fl_plan(B, H, W, levels, &plan);
  const size_t bytes = plan.floats * 4;
  RCV_CHECK_ARG(bytes / 256 < 2147483647ull, "%s: the workspace of batch %d of %dx%d planes does not fit", what, B, H, W);
  if (query) {
    snprintf(query->label, sizeof(query->label), "farneback<%s,n%d,%dpl>", ch == 1 ? "gray" : "rgb", poly_n, plan.n_planes);
    query->n_part = (int)(bytes / 256);
    query->part_bytes = bytes;
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT], "%s: null operand", what);
  RCV_CHECK_ARG(((uintptr_t)op->p[RCV_P_OUT] & 3) == 0, "%s: flow not 4-byte aligned", what);
  RCV_CHECK_ARG(op->p[RCV_P_PART] && ((uintptr_t)op->p[RCV_P_PART] & 255) == 0, "%s: workspace missing or not 256-byte aligned", what);
  RCV_CHECK_ARG(op->i[RCV_I_NPART] == (int)(bytes / 256), "%s: workspace of %d x 256 bytes given, %zu expected (rcv_op_workspace)", what,
                op->i[RCV_I_NPART], bytes / 256);
  float* ws = (float*)op->p[RCV_P_PART];
  FlowPoly kp;
  fl_poly_taps(poly_n, (double)poly_sigma, &kp);
  const float inv_area = (float)(1.0 / ((double)winsize * winsize));
  const float* coarse = nullptr;
  int hc = 0, wc = 0;
  for (int j = plan.n_planes - 1; j >= 0; --j) {
    const FlowPlane& q = plan.pl[j];
    const int hw = q.h * q.w;
    float* flow = j ? ws + q.flow : (float*)op->p[RCV_P_OUT];
    FlowBlur kb;
    fl_blur_taps(j, &kb);
    const dim3 flat(ceil_div(hw, FL_THREADS), 2 * B), tiles(ceil_div(q.w, FL_TX), ceil_div(q.h, FL_TY), 2 * B);
    if (kb.r == 1)
      hipLaunchKernelGGL(flow_image3_kernel, flat, dim3(FL_THREADS), 0, s, (const uint8_t*)op->p[RCV_P_IN], (const uint8_t*)op->p[RCV_P_IN2], ch, B,
                         H, W, q.h, q.w, (float)((double)H / q.h), (float)((double)W / q.w), kb.k[0], kb.k[1], kb.k[2], ws + q.img);
    else
      hipLaunchKernelGGL(flow_image_kernel, flat, dim3(FL_THREADS), 0, s, (const uint8_t*)op->p[RCV_P_IN], (const uint8_t*)op->p[RCV_P_IN2], ch, B,
                         H, W, q.h, q.w, (float)((double)H / q.h), (float)((double)W / q.w), kb, ws + q.img);
    if (poly_n == 5) hipLaunchKernelGGL(flow_polyexp_kernel<5>, tiles, dim3(FL_THREADS), 0, s, ws + q.img, q.h, q.w, kp, ws + q.R);
    else hipLaunchKernelGGL(flow_polyexp_kernel<7>, tiles, dim3(FL_THREADS), 0, s, ws + q.img, q.h, q.w, kp, ws + q.R);
    float* M[2] = {ws + q.M, ws + q.M + fl_align(5 * (size_t)B * hw)};
    hipLaunchKernelGGL(flow_init_kernel, dim3(flat.x, B), dim3(FL_THREADS), 0, s, coarse, hc, wc, coarse ? (float)((double)hc / q.h) : 0.f,
                       coarse ? (float)((double)wc / q.w) : 0.f, ws + q.R, B, q.h, q.w, flow, M[0]);
    for (int it = 0; it < iters; ++it)
      hipLaunchKernelGGL(flow_iterate_kernel, dim3(tiles.x, tiles.y, B), dim3(FL_THREADS), 0, s, M[it & 1], ws + q.R, B, q.h, q.w, winsize / 2,
                         inv_area, flow, it + 1 < iters ? M[(it + 1) & 1] : (float*)nullptr);
    coarse = flow; hc = q.h; wc = q.w;
  }
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_REMAP_LABELS).  Record: i: N, H, W; INMODE = element bytes of the class map (1 = uint8, 8 = int64);
//   p: IN = class map [N][H][W], IN2 = flow float [N][2][H][W], OUT = class map [N][H][W] (must not overlap IN)
// --------------------------------------------------------------------------------------------
static int rcv_launch_remap_labels(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "remap_labels";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], eb = op->i[RCV_I_INMODE];
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(eb == 1 || eb == 8, "%s: class map element size %d unsupported (1 = uint8, 8 = int64)", what, eb);
  RCV_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "%s: batch %d of %dx%d planes out of range", what, N, H, W);
  if (query) {
    snprintf(query->label, sizeof(query->label), "remap_labels<%s>", eb == 1 ? "u8" : "i64");
    query->n_part = 0;
    query->part_bytes = 0;
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT], "%s: null operand", what);
  RCV_CHECK_ARG(op->p[RCV_P_IN] != op->p[RCV_P_OUT], "%s: the remap cannot run in place", what);
  const dim3 grid(ceil_div(H * W, FL_THREADS), N);
  if (eb == 1)
    hipLaunchKernelGGL(flow_remap_kernel<uint8_t>, grid, dim3(FL_THREADS), 0, s, (const uint8_t*)op->p[RCV_P_IN], (const float*)op->p[RCV_P_IN2],
                       H, W, (uint8_t*)op->p[RCV_P_OUT]);
  else
    hipLaunchKernelGGL(flow_remap_kernel<long long>, grid, dim3(FL_THREADS), 0, s, (const long long*)op->p[RCV_P_IN],
                       (const float*)op->p[RCV_P_IN2], H, W, (long long*)op->p[RCV_P_OUT]);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

int rcv_launch_flow(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  return op->kind == RCV_OP_FARNEBACK ? rcv_launch_farneback(h, op, s, query) : rcv_launch_remap_labels(h, op, s, query);
}
