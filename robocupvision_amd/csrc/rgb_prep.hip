// RCV_OP_RGB_PREP (rcv_rgb_prep): the RGB loader of trainer.py:75-123 (SSDataSet with the transforms of trainer.py / pruner.py /
// labelPropTrain.py / tester.py / makeLPImages.py / classTrainer.py / objDetEval.py) for a whole batch:
//   uint8 RGB frames [B][Hs][Ws][3] (+ label planes [B][Hs][Ws], uint8 / int32)  ->  fp32 NCHW YUV [B][3][H][W] (+ int64 targets [B][H][W]).
// Per image, in the reference's order (the contract is restated in tests/rgb_prep_restatement.py and pinned to Pillow there):
//   1. Scale: Pillow's 8-bit BILINEAR resize as two integer passes from host-made tables, exactly as csrc/batch_prep.hip;
//   2. HorizontalFlip, VerticalFlip: mirrored x / y (frame and label alike);
//   3. torchvision's PIL ColorJitter: up to four operations on the uint8 pixel, in the order the parameter row gives --
//        Image.blend(d, x, f) per byte in fp32, multiply and add rounded separately: t = d + f (x - d); 0 if t <= 0, 255 if t >= 255,
//        else t truncated; brightness d = 0, contrast d = m (the rounded mean of L over the whole image as it stands), saturation
//        d = L; L = (19595 R + 38470 G + 7471 B + 32768) >> 16;
//        hue: convert("HSV"), H = (H + shift) & 255, convert("RGB"), with Pillow's roundings --
//          RGB -> HSV: V = maxc; maxc == minc gives H = S = 0; else in fp32 cr = maxc - minc, s = cr / maxc, rc = (maxc - r) / cr (gc, bc
//          likewise); h = bc - gc in fp32 where r == maxc, else (2.0 + rc) - bc resp. (4.0 + gc) - rc in fp64 rounded to fp32;
//          h = fp32(fmod(h / 6.0 + 1.0, 1.0)) in fp64; H = int(h * 255.0), S = int(s * 255.0), products in fp64;
//          HSV -> RGB in fp32: S == 0 gives (V, V, V); else hf = H * 6 / 255, i = floor(hf), f = hf - i, fs = S / 255,
//          p = rnd(V (1 - fs)), q = rnd(V (1 - fs f)), t = rnd(V (1 - fs (1 - f))), rnd = half away from zero; (R, G, B) by i mod 6;
//   4. rgb2yuv + ToTensor + Normalize([.5, 0, 0], [.5, .5, .5]) in fp64: c = byte / 255.0, a matrix row's three products summed left
//      to right, ((y - 0.5) / 0.5, u / 0.5, v / 0.5) rounded once to fp32;
//   5. label: gather through the NEAREST index tables, mirrors, maskLabel, widened to int64.
// Nothing random and no trigonometry here: the parameter row {hflip, vflip, n_ops, op0..op3, f_b, f_c, f_s, hue_shift, 0} comes from the host.
//
// Contrast needs the mean of L over the whole image, so the op is two launches on one stream.  The statistics launch has the grid of
// the main one; a workgroup recomputes its tile's resize and the operations in front of the contrast and writes ONE integer partial sum
// (nothing to zero, no atomics; integer sums have no order to fix).  The main launch sums its image's partials in its prologue, forms
// m = floor((2 sum + n) / (2 n)) and does everything.  Both go through rp_horizontal / rp_vertical / rp_ops.  The statistics launch is
// skipped when the record says that no row holds a contrast (validation mode, rcv.h i[COUNT]).
//
// Tiling as csrc/batch_prep.hip: one workgroup = 8 output rows x 64 output columns of one image, lane = output x; the horizontal pass
// of the source rows under the tile goes to LDS as bytes (from staged source rows where a row shrinks by more than about 3), the
// vertical pass reads it back; the plane stores are contiguous over the
// lanes (reversed under a horizontal flip).  Every table entry is clamped where it is used.
//
// Roundings: this file is compiled with floating-point contraction off (the pragma below): every product that feeds a sum is rounded
// on its own.  __fmul_rn and its kin would not do: the header defines them as the plain operators, which the compiler may fuse.
#include "rcv_internal.h"

#pragma clang fp contract(off)

#define RP_TR 8
#define RP_TC 64
#define RP_MAXK 17                       /* taps of a downscale by 8 */
#define RP_ROWS_MAX 74                   /* source rows under 8 output rows at a downscale by 8 */
#define RP_RC 8                          /* source rows staged at a time */
#define RP_SEG 1600                      /* bytes of one staged row segment: ((63 * 8 + 2 * 8 + 2) * 3 + 15) rounded up to 16 */
#define RP_PREC 22
#define RP_STAGE_MIN_TAPS 9              /* taps per output column from which the source rows are staged in LDS */
#define RP_IDENT_PIX 2048                /* pixels of one image per workgroup where nothing is resized */
#define RP_NPAR 12                       /* floats of a parameter row */

struct RpArgs {
  const uint8_t* frames; const void* labels; float* imgs; int64_t* tgt;
  const int32_t* xtab; const int32_t* ytab; const int32_t* lx; const int32_t* ly; const float* params; uint32_t* part;
  int B, Hs, Ws, H, W, kx, ky, lab_bytes, train, mask, rows_cap, tiles_x, tiles_y, stats, wpi;      // wpi: workgroups per image
};

__device__ __forceinline__ int rp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int rp_clip8(int acc) { return rp_clampi(acc >> RP_PREC, 0, 255); }

// transform.py:26-49 on one value; m bits: 1 = nb, 2 = nr, 4 = ng, 8 = nl
__device__ __forceinline__ int rp_mask(int v, int m) {
  int rN = 2, gN = 3, lN = 4;
  if (m & 1) { if (v == 1) v = 0; if (v > 1) v -= 1; rN = 1; gN = 2; lN = 3; }
  if (m & 2) { if (v == rN) v = 0; if (v > rN) v -= 1; gN = 1; lN = 2; }
  if (m & 4) { if (v == gN) v = 0; if (v > gN) v -= 1; lN = 1; }
  if (m & 8) { if (v == lN) v = 0; }
  return v;
}

// the parameter row of an image; ops = the four op codes, 4 bits each (15 = none; no indexed array: it would live in scratch memory);
// cpos = position of the first contrast among its operations, -1 = none (uniform over a workgroup)
struct RpRow { bool hflip, vflip; int n_ops, cpos, ops, shift; float fb, fc, fs; };

__device__ __forceinline__ RpRow rp_row(const RpArgs& a, int b) {
  RpRow j;
  j.hflip = false; j.vflip = false; j.n_ops = 0; j.cpos = -1; j.ops = 0xffff; j.shift = 0; j.fb = 1.f; j.fc = 1.f; j.fs = 1.f;
  if (a.train) {
    const float* p = a.params + (size_t)b * RP_NPAR;
    j.hflip = p[0] != 0.f; j.vflip = p[1] != 0.f;
    j.n_ops = rp_clampi((int)p[2], 0, 4);
    j.ops = 0;
    for (int k = 0; k < 4; ++k) {
      const int c = (int)p[3 + k];
      j.ops |= (c >= 0 && c <= 3 ? c : 15) << (4 * k);
    }
    j.fb = p[7]; j.fc = p[8]; j.fs = p[9]; j.shift = (int)p[10] & 255;
    for (int k = j.n_ops - 1; k >= 0; --k) if (((j.ops >> (4 * k)) & 15) == 1) j.cpos = k;
  }
  return j;
}

__device__ __forceinline__ int rp_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// Image.blend(d, x, f) on one byte (x - d is exact in fp32)
__device__ __forceinline__ int rp_blend(int d, int x, float f) {
  const float prod = f * (float)(x - d);
  const float t = (float)d + prod;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// rnd(v) of a value that is never negative, clipped to a byte ((double)v + 0.5 is exact)
__device__ __forceinline__ int rp_rnd8(float v) { return rp_clampi((int)((double)v + 0.5), 0, 255); }

// Pillow's convert("HSV"), H = (H + shift) & 255, convert("RGB") on one pixel
__device__ __forceinline__ void rp_hue(int shift, int& r, int& g, int& b) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  const int V = maxc;
  int Hh = 0, S = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) {
      h = bc - gc;
    } else if (g == maxc) {
      const double t2 = 2.0 + (double)rc;
      h = (float)(t2 - (double)bc);
    } else {
      const double t4 = 4.0 + (double)gc;
      h = (float)(t4 - (double)rc);
    }
    const double h6 = (double)h / 6.0;
    double x = h6 + 1.0;                        // in [5/6, 11/6]
    if (x >= 1.0) x = x - 1.0;                  // fmod(x, 1.0), exact
    const float hf = (float)x;
    Hh = rp_clampi((int)((double)hf * 255.0), 0, 255);
    S = rp_clampi((int)((double)s * 255.0), 0, 255);
  }
  Hh = (Hh + shift) & 255;
  if (S == 0) { r = V; g = V; b = V; return; }
  const float h6 = (float)Hh * 6.f;
  const float hf = h6 / 255.f;
  const float fi = floorf(hf);
  const float f = hf - fi;
  const float fs = (float)S / 255.f;
  const float v = (float)V;
  const float one_fs = 1.f - fs;
  const float fsf = fs * f;
  const float one_f = 1.f - f;
  const float fs1f = fs * one_f;
  const float wp = v * one_fs;
  const float wq = v * (1.f - fsf);
  const float wt = v * (1.f - fs1f);
  const int p = rp_rnd8(wp), q = rp_rnd8(wq), t = rp_rnd8(wt);
  switch ((int)fi % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// a resized pixel after the first k operations of its image's row; m = the contrast mean (looked at by a contrast in front of k only)
__device__ __forceinline__ void rp_ops(const RpRow& j, int k, int m, int& r, int& g, int& b) {
  for (int i = 0; i < k; ++i) {
    const int op = (j.ops >> (4 * i)) & 15;
    if (op == 0) {
      r = rp_blend(0, r, j.fb); g = rp_blend(0, g, j.fb); b = rp_blend(0, b, j.fb);
    } else if (op == 1) {
      r = rp_blend(m, r, j.fc); g = rp_blend(m, g, j.fc); b = rp_blend(m, b, j.fc);
    } else if (op == 2) {
      const int l = rp_luma(r, g, b);
      r = rp_blend(l, r, j.fs); g = rp_blend(l, g, j.fs); b = rp_blend(l, b, j.fs);
    } else if (op == 3) {
      rp_hue(j.shift, r, g, b);
    }
  }
}

// sum over the workgroup (256 threads), returned to every thread; s_red: 256 values
__device__ __forceinline__ unsigned long long rp_block_sum(unsigned long long v, unsigned long long* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s_red[tid] += s_red[tid + w];
    __syncthreads();
  }
  return s_red[0];
}

// the contrast mean of image b from the partial sums of the statistics launch: floor((2 sum L + n) / (2 n))
__device__ __forceinline__ int rp_mean(const RpArgs& a, const RpRow& j, int b, unsigned long long* s_red) {
  if (j.cpos < 0 || !a.stats) return 0;          // (uniform over the workgroup)
  unsigned long long v = 0;
  const uint32_t* part = a.part + (size_t)b * a.wpi;
  for (int i = threadIdx.x; i < a.wpi; i += 256) v += part[i];
  const unsigned long long sum = rp_block_sum(v, s_red), n = (unsigned long long)a.H * a.W;
  return (int)((2ull * sum + n) / (2ull * n));
}

// steps 4 and 5 for one output pixel (x, y: coordinates before the mirrors) of image b from its bytes after step 3
__device__ __forceinline__ void rp_finish(const RpArgs& a, const RpRow& j, const double* s_c, int b, int y, int x, int r, int g, int bl) {
  const double cr = s_c[r], cg = s_c[g], cb = s_c[bl];
  const double y0 = cr * 0.299, y1 = cg * 0.587, y2 = cb * 0.114;
  const double u0 = cr * -0.14714119, u1 = cg * -0.28886916, u2 = cb * 0.43601035;
  const double v0 = cr * 0.61497538, v1 = cg * -0.51496512, v2 = cb * -0.10001026;
  const double yy = (y0 + y1) + y2, uu = (u0 + u1) + u2, vv = (v0 + v1) + v2;
  const int xo = j.hflip ? a.W - 1 - x : x, yo = j.vflip ? a.H - 1 - y : y;
  const size_t plane = (size_t)a.H * a.W, o = (size_t)yo * a.W + xo;
  float* img = a.imgs + (size_t)b * 3 * plane + o;
  img[0] = (float)((yy - 0.5) / 0.5); img[plane] = (float)(uu / 0.5); img[2 * plane] = (float)(vv / 0.5);
  if (!a.tgt) return;                      // the patch chain: no label plane (uniform over the launch)
  const int sy = rp_clampi(a.ly[y], 0, a.Hs - 1), sx = rp_clampi(a.lx[x], 0, a.Ws - 1);
  const size_t li = ((size_t)b * a.Hs + sy) * a.Ws + sx;
  const int lv = a.lab_bytes == 1 ? (int)((const uint8_t*)a.labels)[li] : ((const int32_t*)a.labels)[li];
  a.tgt[(size_t)b * plane + o] = (int64_t)rp_mask(lv, a.mask);
}

struct RpTile { int x0, y0, tw, th, ys0, nrows; };

// the tile's tables to LDS and the horizontal pass of the source rows under it: s_h[r][x][c].  STAGE (as csrc/batch_prep.hip, from 9
// taps per column): the source-row segments of the tile are first copied to LDS with 16-byte aligned loads, RP_RC rows at a time, and
// the taps read LDS bytes; otherwise the taps read global bytes through the cache.
template <bool STAGE>
__device__ __forceinline__ RpTile rp_horizontal(const RpArgs& a, int b, int tile, int32_t* s_xc, int32_t* s_yc, uint8_t* s_h, uint8_t* s_src) {
  const int tid = threadIdx.x;
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  RpTile t;
  t.x0 = tx * RP_TC; t.y0 = ty * RP_TR;
  t.tw = min(RP_TC, a.W - t.x0); t.th = min(RP_TR, a.H - t.y0);
  const int sx = 2 + a.kx, sy = 2 + a.ky;
  for (int i = tid; i < t.tw * sx; i += 256) s_xc[i] = a.xtab[(size_t)t.x0 * sx + i];
  for (int i = tid; i < t.th * sy; i += 256) s_yc[i] = a.ytab[(size_t)t.y0 * sy + i];
  __syncthreads();
  t.ys0 = rp_clampi(s_yc[0], 0, a.Hs - 1);
  const int ys1 = rp_clampi(s_yc[(t.th - 1) * sy] + s_yc[(t.th - 1) * sy + 1], t.ys0 + 1, a.Hs);
  t.nrows = min(ys1 - t.ys0, a.rows_cap);
  const uint8_t* fb = a.frames + (size_t)b * a.Hs * a.Ws * 3;
  const int x = tid & (RP_TC - 1);
  const int32_t* xc = s_xc + (x < t.tw ? x : 0) * sx;
  const int xf = rp_clampi(xc[0], 0, a.Ws - 1);
  const int xn = min(rp_clampi(xc[1], 0, a.kx), a.Ws - xf);
  if (!STAGE) {
    if (x < t.tw) {
      for (int r = tid >> 6; r < t.nrows; r += 4) {
        const uint8_t* p = fb + ((size_t)(t.ys0 + r) * a.Ws + xf) * 3;
        int a0 = 1 << (RP_PREC - 1), a1 = a0, a2 = a0;
        for (int k = 0; k < xn; ++k) {
          const int c = xc[2 + k];
          a0 += (int)p[3 * k] * c; a1 += (int)p[3 * k + 1] * c; a2 += (int)p[3 * k + 2] * c;
        }
        uint8_t* q = s_h + (r * RP_TC + x) * 3;
        q[0] = (uint8_t)rp_clip8(a0); q[1] = (uint8_t)rp_clip8(a1); q[2] = (uint8_t)rp_clip8(a2);
      }
    }
  } else {
    // source pixels under this tile's horizontal taps: [xs0, xs0 + segpix)
    const int xs0 = rp_clampi(s_xc[0], 0, a.Ws - 1);
    const int xs1 = rp_clampi(s_xc[(t.tw - 1) * sx] + s_xc[(t.tw - 1) * sx + 1], xs0 + 1, a.Ws);
    const int segpix = min(xs1 - xs0, (RP_SEG - 16) / 3);
    const int seg = segpix * 3;
    const int nvmax = (seg + 15 + 15) / 16;
    const int rel = rp_clampi(xf - xs0, 0, segpix - 1);
    const int xns = min(xn, segpix - rel);
    const uintptr_t lo = (uintptr_t)a.frames, hi = lo + (size_t)a.B * a.Hs * a.Ws * 3;
    for (int r0 = 0; r0 < t.nrows; r0 += RP_RC) {
      const int nr = min(RP_RC, t.nrows - r0);
      for (int i = tid; i < nr * nvmax; i += 256) {
        const int rr = i / nvmax, v = i - rr * nvmax;
        const uintptr_t A = (uintptr_t)(fb + ((size_t)(t.ys0 + r0 + rr) * a.Ws + xs0) * 3);
        const uintptr_t va = (A & ~(uintptr_t)15) + 16u * (uintptr_t)v;
        if (va >= A + seg) continue;
        uint4 w;
        if (va >= lo && va + 16 <= hi) {
          w = *(const uint4*)va;
        } else {                          // the first / last 16 bytes of the whole frame buffer when it is not 16-byte aligned
          uint32_t d[4] = {0u, 0u, 0u, 0u};
          for (int q = 0; q < 16; ++q) {
            const uintptr_t ad = va + q;
            if (ad >= lo && ad < hi) d[q >> 2] |= (uint32_t)(*(const uint8_t*)ad) << (8 * (q & 3));
          }
          w = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *(uint4*)(s_src + rr * RP_SEG + 16 * v) = w;
      }
      __syncthreads();
      if (x < t.tw) {
        for (int rr = tid >> 6; rr < nr; rr += 4) {
          const uintptr_t A = (uintptr_t)(fb + ((size_t)(t.ys0 + r0 + rr) * a.Ws + xs0) * 3);
          const uint8_t* p = s_src + rr * RP_SEG + (int)(A & 15) + rel * 3;
          int a0 = 1 << (RP_PREC - 1), a1 = a0, a2 = a0;
          for (int k = 0; k < xns; ++k) {
            const int c = xc[2 + k];
            a0 += (int)p[3 * k] * c; a1 += (int)p[3 * k + 1] * c; a2 += (int)p[3 * k + 2] * c;
          }
          uint8_t* q = s_h + ((r0 + rr) * RP_TC + x) * 3;
          q[0] = (uint8_t)rp_clip8(a0); q[1] = (uint8_t)rp_clip8(a1); q[2] = (uint8_t)rp_clip8(a2);
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  return t;
}

// the vertical pass for the output pixel (x, yl) of the tile (x < tw, yl < th)
__device__ __forceinline__ void rp_vertical(const RpArgs& a, const RpTile& t, const int32_t* s_yc, const uint8_t* s_h, int yl, int x, int& r, int& g,
                                            int& b) {
  const int32_t* yc = s_yc + yl * (2 + a.ky);
  const int yf = yc[0] - t.ys0, yn = rp_clampi(yc[1], 0, a.ky);
  int a0 = 1 << (RP_PREC - 1), a1 = a0, a2 = a0;
  for (int k = 0; k < yn; ++k) {
    const int c = yc[2 + k];
    const uint8_t* q = s_h + (rp_clampi(yf + k, 0, t.nrows - 1) * RP_TC + x) * 3;
    a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
  }
  r = rp_clip8(a0); g = rp_clip8(a1); b = rp_clip8(a2);
}

// STATS: the statistics launch (one partial sum of L per workgroup); otherwise the main launch.  STAGE: see rp_horizontal.
// Grid: B * tiles_x * tiles_y.
template <bool STATS, bool STAGE>
__global__ __launch_bounds__(256) void rgb_prep_kernel(RpArgs a) {
  __shared__ double s_c[256];
  __shared__ unsigned long long s_red[256];
  __shared__ int32_t s_xc[RP_TC * (2 + RP_MAXK)];
  __shared__ int32_t s_yc[RP_TR * (2 + RP_MAXK)];
  __shared__ uint8_t s_h[RP_ROWS_MAX * RP_TC * 3];
  __shared__ __align__(16) uint8_t s_src[STAGE ? RP_RC * RP_SEG : 16];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.wpi, tile = blockIdx.x % a.wpi;
  const RpRow j = rp_row(a, b);
  if (STATS && j.cpos < 0) {                     // no contrast in this image: nobody reads its partials
    if (tid == 0) a.part[blockIdx.x] = 0u;
    return;
  }
  int m = 0;
  if (!STATS) {
    s_c[tid] = (double)tid / 255.0;
    m = rp_mean(a, j, b, s_red);
  }
  const RpTile t = rp_horizontal<STAGE>(a, b, tile, s_xc, s_yc, s_h, s_src);
  const int x = tid & (RP_TC - 1);
  unsigned long long lsum = 0;
  for (int idx = tid; idx < t.th * RP_TC; idx += 256) {
    const int yl = idx >> 6;
    if (x >= t.tw) continue;
    int r, g, bl;
    rp_vertical(a, t, s_yc, s_h, yl, x, r, g, bl);
    if (STATS) {
      rp_ops(j, j.cpos, 0, r, g, bl);
      lsum += (unsigned long long)rp_luma(r, g, bl);
    } else {
      rp_ops(j, j.n_ops, m, r, g, bl);
      rp_finish(a, j, s_c, b, t.y0 + yl, t.x0 + x, r, g, bl);
    }
  }
  if (STATS) {
    const unsigned long long s = rp_block_sum(lsum, s_red);      // <= 512 * 255
    if (tid == 0) a.part[blockIdx.x] = (uint32_t)s;
  }
}

// H == Hs and W == Ws: no resize (transform.py:15-16); one thread per pixel, RP_IDENT_PIX pixels of one image per workgroup
template <bool STATS>
__global__ __launch_bounds__(256) void rgb_prep_ident_kernel(RpArgs a) {
  __shared__ double s_c[256];
  __shared__ unsigned long long s_red[256];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.wpi, blk = blockIdx.x % a.wpi;
  const RpRow j = rp_row(a, b);
  if (STATS && j.cpos < 0) {
    if (tid == 0) a.part[blockIdx.x] = 0u;
    return;
  }
  int m = 0;
  if (!STATS) {
    s_c[tid] = (double)tid / 255.0;
    m = rp_mean(a, j, b, s_red);
    __syncthreads();
  }
  const int npix = a.H * a.W;
  const uint8_t* fb = a.frames + (size_t)b * npix * 3;
  const int start = blk * RP_IDENT_PIX, end = start + min(RP_IDENT_PIX, npix - start);
  unsigned long long lsum = 0;
  for (int p = start + tid; p < end; p += 256) {
    const uint8_t* q = fb + (size_t)p * 3;
    int r = q[0], g = q[1], bl = q[2];
    if (STATS) {
      rp_ops(j, j.cpos, 0, r, g, bl);
      lsum += (unsigned long long)rp_luma(r, g, bl);
    } else {
      const int y = p / a.W, x = p - y * a.W;
      rp_ops(j, j.n_ops, m, r, g, bl);
      rp_finish(a, j, s_c, b, y, x, r, g, bl);
    }
  }
  if (STATS) {
    const unsigned long long s = rp_block_sum(lsum, s_red);      // <= 2048 * 255
    if (tid == 0) a.part[blockIdx.x] = (uint32_t)s;
  }
}

// Pillow's precompute_coeffs: taps per output index of the BILINEAR filter
static int rp_ksize(int in, int out) {
  double scale = (double)in / out;
  if (scale < 1.0) scale = 1.0;
  int c = (int)scale;
  if ((double)c < scale) ++c;
  return c * 2 + 1;
}

// Every refusal that depends on the shape of the record, and the tables, sits in front of the `query` return (what rcv_batch_prep
// refuses is refused here); the batch operands are checked at launch.
int rcv_launch_rgb_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], Hs = op->i[RCV_I_H], Ws = op->i[RCV_I_W], H = op->i[RCV_I_HO], W = op->i[RCV_I_WO];
  const int kx = op->i[RCV_I_CIN], ky = op->i[RCV_I_COUT], lab_bytes = op->i[RCV_I_INMODE2];
  const int train = op->i[RCV_I_AUX0], mask = op->i[RCV_I_AUX1], stats = op->i[RCV_I_COUNT];
  const bool with_labels = lab_bytes != 0;
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), "rgb_prep");
  }
  RCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "rgb prep: B %d, source %d x %d, output %d x %d: every size must be >= 1", B, Hs, Ws,
                H, W);
  RCV_CHECK_ARG((long long)Hs <= 8LL * H && (long long)Ws <= 8LL * W,
                "rgb prep: %d x %d -> %d x %d shrinks an axis by more than 8 (the kernel is built for at most %d taps)", Hs, Ws, H, W, RP_MAXK);
  RCV_CHECK_ARG(lab_bytes == 0 || lab_bytes == 1 || lab_bytes == 4,
                "rgb prep: label element size %d unsupported (1 = uint8, 4 = int32, 0 = no labels)", lab_bytes);
  RCV_CHECK_ARG(kx == rp_ksize(Ws, W) && ky == rp_ksize(Hs, H), "rgb prep: %d / %d taps per column / row given, %d -> %d and %d -> %d take %d / %d", kx,
                ky, Ws, W, Hs, H, rp_ksize(Ws, W), rp_ksize(Hs, H));
  RCV_CHECK_ARG((train == 0 || train == 1) && mask >= 0 && mask <= 15 && (stats == 0 || stats == 1),
                "rgb prep: train %d / maskLabel flags %d / statistics %d out of range", train, mask, stats);
  const int tiles_x = ceil_div(W, RP_TC), tiles_y = ceil_div(H, RP_TR);
  RCV_CHECK_ARG((double)B * Hs * Ws < 2147483647.0 && (double)B * H * W < 2147483647.0 && (double)B * tiles_x * tiles_y < 2147483647.0,
                "rgb prep: %d images of %d x %d -> %d x %d: more than 2^31 pixels", B, Hs, Ws, H, W);
  if (with_labels)
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2] && op->p[RCV_P_X3] && op->p[RCV_P_X4],
                  "rgb prep: null table (frame taps of x / y, label index of x / y)");
  else
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2], "rgb prep: null table (frame taps of x / y)");
  const bool ident = H == Hs && W == Ws;
  const int wpi = ident ? ceil_div(H * W, RP_IDENT_PIX) : tiles_x * tiles_y;
  RCV_CHECK_ARG((double)B * wpi < 2147483647.0, "rgb prep: grid too large");
  const bool two = train && stats;
  const int n_part = two ? B * wpi : 0;
  if (query) {
    query->n_part = n_part;
    query->part_bytes = (size_t)n_part * sizeof(uint32_t);
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_OUT], "rgb prep: null operand");
  RCV_CHECK_ARG(!with_labels || (op->p[RCV_P_IN2] && op->p[RCV_P_X0]), "rgb prep: null label operand");
  RCV_CHECK_ARG(!train || op->p[RCV_P_IN_C], "rgb prep: training mode needs the parameter rows float[B][%d]", RP_NPAR);
  RCV_CHECK_ARG(!two || (op->p[RCV_P_PART] && ((uintptr_t)op->p[RCV_P_PART] & 3) == 0 && op->i[RCV_I_NPART] == n_part),
                "rgb prep: workspace missing, unaligned or of %d partial sums where %d are needed (rcv_op_workspace)", op->i[RCV_I_NPART], n_part);
  RpArgs a;
  a.frames = (const uint8_t*)op->p[RCV_P_IN]; a.imgs = (float*)op->p[RCV_P_OUT];
  a.labels = with_labels ? op->p[RCV_P_IN2] : nullptr; a.tgt = with_labels ? (int64_t*)op->p[RCV_P_X0] : nullptr;
  a.xtab = (const int32_t*)op->p[RCV_P_X1]; a.ytab = (const int32_t*)op->p[RCV_P_X2];
  a.lx = with_labels ? (const int32_t*)op->p[RCV_P_X3] : nullptr; a.ly = with_labels ? (const int32_t*)op->p[RCV_P_X4] : nullptr;
  a.params = train ? (const float*)op->p[RCV_P_IN_C] : nullptr; a.part = two ? (uint32_t*)op->p[RCV_P_PART] : nullptr;
  a.B = B; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.kx = kx; a.ky = ky; a.lab_bytes = with_labels ? lab_bytes : 1; a.train = train; a.mask = mask;
  a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.stats = two ? 1 : 0; a.wpi = wpi; a.rows_cap = 0;
  const dim3 grid(B * wpi), block(256);
  if (ident) {
    if (two) hipLaunchKernelGGL(rgb_prep_ident_kernel<true>, grid, block, 0, s, a);
    hipLaunchKernelGGL(rgb_prep_ident_kernel<false>, grid, block, 0, s, a);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  const double scale_y = (double)Hs / H, support_y = scale_y < 1.0 ? 1.0 : scale_y;
  const double span = (RP_TR - 1) * scale_y + 2.0 * support_y;
  a.rows_cap = (int)span + ((double)(int)span < span ? 1 : 0) + 2;
  if (a.rows_cap > RP_ROWS_MAX) a.rows_cap = RP_ROWS_MAX;
  const bool stage = kx >= RP_STAGE_MIN_TAPS;
  void (*const stat_kernel)(RpArgs) = stage ? rgb_prep_kernel<true, true> : rgb_prep_kernel<true, false>;
  void (*const main_kernel)(RpArgs) = stage ? rgb_prep_kernel<false, true> : rgb_prep_kernel<false, false>;
  if (two) hipLaunchKernelGGL(stat_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(main_kernel, grid, block, 0, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
