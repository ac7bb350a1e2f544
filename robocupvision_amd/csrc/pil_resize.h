// Pillow's 8-bit BILINEAR resize as one tile pass, and the small pieces the loader kernels share: THE definition for
// csrc/batch_prep.hip, csrc/rgb_prep.hip and (the small pieces and the colour step) csrc/patches.hip.  Every piece is a bit-exactness
// contract against Pillow, pinned by the goldens and the live Pillow comparisons of tests/test_*batch_prep*, *rgb_prep*, *resident*,
// *patches*: a fix to the staging loads, the clamps or a constant is made here, once.
//   resize: two integer passes (horizontal, rounded to uint8, then vertical) from host-made tables -- per output index a first tap, a
//     tap count and 22-bit integer coefficients (robocupvision_amd/data.py); out = clip((sum + 2^21) >> 22).  Integer only.
//   tile: one workgroup (256 threads) = PIL_TR output rows x PIL_TC output columns of one image, lane = output x (one wave = one row).
//     The horizontal pass of the source rows under the tile's vertical taps goes to LDS as bytes (s_h [rows][64][3]); the vertical pass
//     reads it back.  STAGE: the source-row segments of the tile are first copied to LDS with 16-byte aligned loads, PIL_RC rows at a
//     time, and the horizontal taps read LDS bytes; otherwise the taps read global bytes through the cache.
//   Every table entry is clamped where it is used: a wrong table gives wrong pixels, never an access outside the operands.
// The tile functions are templated on the kernel's argument struct (BpArgs, RpArgs: frames, xtab, ytab, Hs, Ws, H, W, kx, ky, rows_cap,
// ... by name), which keeps its own layout.
// pil_yuv_norm is floating point and needs every product rounded on its own: include this header BELOW the file's
// `#pragma clang fp contract(off)` (rgb_prep.hip, patches.hip); the function repeats the pragma for its own body.  batch_prep.hip, which
// is compiled with contraction on and uses explicit fmaf, does not call it.
#pragma once
#include "rcv_internal.h"

#define PIL_TR 8
#define PIL_TC 64
#define PIL_MAXK 17                      /* taps of a downscale by 8: ceil(8) * 2 + 1 */
#define PIL_ROWS_MAX 74                  /* ceil(7 * 8 + 2 * 8) + 2 source rows under 8 output rows */
#define PIL_RC 8                         /* source rows staged at a time */
#define PIL_SEG 1600                     /* bytes of one staged row segment: ((63 * 8 + 2 * 8 + 2) * 3 + 15) rounded up to 16 */
#define PIL_PREC 22                      /* Pillow's 8-bit resampling: 32 - 8 - 2 */
#define PIL_STAGE_MIN_TAPS 9             /* taps per output column from which the source rows are staged in LDS (measured) */
#define PIL_IDENT_PIX 2048               /* pixels of one image per workgroup where nothing is resized */

// ---- device, small
__device__ __forceinline__ int pil_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int pil_clip8(int acc) { return pil_clampi(acc >> PIL_PREC, 0, 255); }

// maskLabel, transform.py:26-49, on one value; m bits: 1 = nb, 2 = nr, 4 = ng, 8 = nl (the branches are uniform over the launch)
__device__ __forceinline__ int pil_mask_label(int v, int m) {
  int rN = 2, gN = 3, lN = 4;
  if (m & 1) { if (v == 1) v = 0; if (v > 1) v -= 1; rN = 1; gN = 2; lN = 3; }
  if (m & 2) { if (v == rN) v = 0; if (v > rN) v -= 1; gN = 1; lN = 2; }
  if (m & 4) { if (v == gN) v = 0; if (v > gN) v -= 1; lN = 1; }
  if (m & 8) { if (v == lN) v = 0; }
  return v;
}

// the indexed forms: the store image of element e of a.index (elements of 4 / 8 bytes), or -1 where it is outside [0, a.nsrc) -- tested
// before it is used for anything
template <typename Args>
__device__ __forceinline__ int pil_source(const Args& a, size_t e) {
  const long long v = a.idx_bytes == 8 ? (long long)((const int64_t*)a.index)[e] : (long long)((const int32_t*)a.index)[e];
  return v >= 0 && v < (long long)a.nsrc ? (int)v : -1;
}

// element li of label planes of 1 (uint8) / 4 (int32) byte elements
__device__ __forceinline__ int pil_label_at(const void* labels, int lab_bytes, size_t li) {
  return lab_bytes == 1 ? (int)((const uint8_t*)labels)[li] : ((const int32_t*)labels)[li];
}

// the label under output pixel (x, y) of source image src, through the NEAREST index tables
template <typename Args>
__device__ __forceinline__ int pil_label(const Args& a, int src, int y, int x) {
  const int sy = pil_clampi(a.ly[y], 0, a.Hs - 1), sx = pil_clampi(a.lx[x], 0, a.Ws - 1);
  return pil_label_at(a.labels, a.lab_bytes, ((size_t)src * a.Hs + sy) * a.Ws + sx);
}

// the 16-byte word at the aligned address va of a buffer [lo, hi); bytes outside it (the first / last word of a buffer that is not
// 16-byte aligned) read as zero and are never looked at.  Keep the d[t >> 2] form: with four named words and a chain of tests the
// staged loop of batch_prep_kernel is scheduled differently and resize_u8 measured 1.1 % slower.
__device__ __forceinline__ uint4 pil_load16(uintptr_t va, uintptr_t lo, uintptr_t hi) {
  if (va >= lo && va + 16 <= hi) return *reinterpret_cast<const uint4*>(va);
  uint32_t d[4] = {0u, 0u, 0u, 0u};
  for (int t = 0; t < 16; ++t) {
    const uintptr_t ad = va + t;
    if (ad >= lo && ad < hi) d[t >> 2] |= (uint32_t)(*(const uint8_t*)ad) << (8 * (t & 3));
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// ---- device, tile
struct PilTile { int x0, y0, tw, th, ys0, nrows; };          // origin and size in output pixels; first source row, source rows held in s_h

// tile (tx, ty) of an image; ys0 / nrows are pil_horizontal's
template <typename Args>
__device__ __forceinline__ PilTile pil_tile(const Args& a, int tx, int ty) {
  PilTile t;
  t.x0 = tx * PIL_TC; t.y0 = ty * PIL_TR;
  t.tw = min(PIL_TC, a.W - t.x0); t.th = min(PIL_TR, a.H - t.y0);
  t.ys0 = 0; t.nrows = 0;
  return t;
}

// an indexed form with a refused index: the tile's pixels of batch row b are zeros, their targets 0.  The test of a.tgt is for
// rgb_prep's records without labels; batch_prep's indexed form always has targets (its own copy wrote them without the test).
template <typename Args>
__device__ __forceinline__ void pil_zero(const Args& a, int b, int y, int x) {
  const size_t plane = (size_t)a.H * a.W, o = (size_t)y * a.W + x;
  float* img = a.imgs + (size_t)b * 3 * plane + o;
  img[0] = 0.f; img[plane] = 0.f; img[2 * plane] = 0.f;
  if (a.tgt) a.tgt[(size_t)b * plane + o] = 0;
}
template <typename Args>
__device__ __forceinline__ void pil_zero_tile(const Args& a, int b, const PilTile& t) {
  for (int idx = threadIdx.x; idx < t.th * PIL_TC; idx += 256)
    if ((idx & (PIL_TC - 1)) < t.tw) pil_zero(a, b, t.y0 + (idx >> 6), t.x0 + (idx & (PIL_TC - 1)));
}

// The tile's tables to LDS (closed by a barrier: what the caller has written to LDS in front of the call is visible after it) and the
// horizontal pass of the source rows of image src under the tile: s_h[r][x][c] for the rows ys0 .. ys0 + nrows.  nimg: the images
// behind a.frames (the aligned staging loads stay inside them).  LDS: s_xc [PIL_TC][2 + PIL_MAXK], s_yc [PIL_TR][2 + PIL_MAXK],
// s_h [PIL_ROWS_MAX][PIL_TC][3], s_src (STAGE only, 16-byte aligned) [PIL_RC][PIL_SEG].
template <bool STAGE, typename Args>
__device__ __forceinline__ void pil_horizontal(const Args& a, int src, int nimg, PilTile& t, int32_t* s_xc, int32_t* s_yc, uint8_t* s_h,
                                               uint8_t* s_src) {
  const int tid = threadIdx.x;
  const int sx = 2 + a.kx, sy = 2 + a.ky;
  for (int i = tid; i < t.tw * sx; i += 256) s_xc[i] = a.xtab[(size_t)t.x0 * sx + i];
  for (int i = tid; i < t.th * sy; i += 256) s_yc[i] = a.ytab[(size_t)t.y0 * sy + i];
  __syncthreads();
  // source rows under this tile's vertical taps
  t.ys0 = pil_clampi(s_yc[0], 0, a.Hs - 1);
  const int ys1 = pil_clampi(s_yc[(t.th - 1) * sy] + s_yc[(t.th - 1) * sy + 1], t.ys0 + 1, a.Hs);
  t.nrows = min(ys1 - t.ys0, a.rows_cap);
  const uint8_t* fb = a.frames + (size_t)src * a.Hs * a.Ws * 3;
  // this thread's column is fixed
  const int x = tid & (PIL_TC - 1);
  const int32_t* xc = s_xc + (x < t.tw ? x : 0) * sx;
  const int xf = pil_clampi(xc[0], 0, a.Ws - 1);
  const int xn = min(pil_clampi(xc[1], 0, a.kx), a.Ws - xf);
  if (!STAGE) {
    if (x < t.tw) {
      for (int r = tid >> 6; r < t.nrows; r += 4) {
        const uint8_t* p = fb + ((size_t)(t.ys0 + r) * a.Ws + xf) * 3;
        int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
        for (int k = 0; k < xn; ++k) {
          const int c = xc[2 + k];
          a0 += (int)p[3 * k] * c; a1 += (int)p[3 * k + 1] * c; a2 += (int)p[3 * k + 2] * c;
        }
        uint8_t* q = s_h + (r * PIL_TC + x) * 3;
        q[0] = (uint8_t)pil_clip8(a0); q[1] = (uint8_t)pil_clip8(a1); q[2] = (uint8_t)pil_clip8(a2);
      }
    }
  } else {
    // source pixels under this tile's horizontal taps: [xs0, xs0 + segpix)
    const int xs0 = pil_clampi(s_xc[0], 0, a.Ws - 1);
    const int xs1 = pil_clampi(s_xc[(t.tw - 1) * sx] + s_xc[(t.tw - 1) * sx + 1], xs0 + 1, a.Ws);
    const int segpix = min(xs1 - xs0, (PIL_SEG - 16) / 3);
    const int seg = segpix * 3;
    const int nvmax = (seg + 15 + 15) / 16;
    const int rel = pil_clampi(xf - xs0, 0, segpix - 1);
    const int xns = min(xn, segpix - rel);
    const uintptr_t lo = (uintptr_t)a.frames, hi = lo + (size_t)nimg * a.Hs * a.Ws * 3;
    for (int r0 = 0; r0 < t.nrows; r0 += PIL_RC) {
      const int nr = min(PIL_RC, t.nrows - r0);
      for (int i = tid; i < nr * nvmax; i += 256) {
        const int rr = i / nvmax, v = i - rr * nvmax;
        const uintptr_t A = (uintptr_t)(fb + ((size_t)(t.ys0 + r0 + rr) * a.Ws + xs0) * 3);
        const uintptr_t va = (A & ~(uintptr_t)15) + 16u * (uintptr_t)v;
        if (va >= A + seg) continue;
        *(uint4*)(s_src + rr * PIL_SEG + 16 * v) = pil_load16(va, lo, hi);
      }
      __syncthreads();
      if (x < t.tw) {
        for (int rr = tid >> 6; rr < nr; rr += 4) {
          const uintptr_t A = (uintptr_t)(fb + ((size_t)(t.ys0 + r0 + rr) * a.Ws + xs0) * 3);
          const uint8_t* p = s_src + rr * PIL_SEG + (int)(A & 15) + rel * 3;
          int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
          for (int k = 0; k < xns; ++k) {
            const int c = xc[2 + k];
            a0 += (int)p[3 * k] * c; a1 += (int)p[3 * k + 1] * c; a2 += (int)p[3 * k + 2] * c;
          }
          uint8_t* q = s_h + ((r0 + rr) * PIL_TC + x) * 3;
          q[0] = (uint8_t)pil_clip8(a0); q[1] = (uint8_t)pil_clip8(a1); q[2] = (uint8_t)pil_clip8(a2);
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
}

// the vertical pass for the output pixel (x, yl) of the tile (x < tw, yl < th): its three resized bytes
template <typename Args>
__device__ __forceinline__ void pil_vertical(const Args& a, const PilTile& t, const int32_t* s_yc, const uint8_t* s_h, int yl, int x, int& c0,
                                             int& c1, int& c2) {
  const int32_t* yc = s_yc + yl * (2 + a.ky);
  const int yf = yc[0] - t.ys0, yn = pil_clampi(yc[1], 0, a.ky);
  int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
  for (int k = 0; k < yn; ++k) {
    const int c = yc[2 + k];
    const uint8_t* q = s_h + (pil_clampi(yf + k, 0, t.nrows - 1) * PIL_TC + x) * 3;
    a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
  }
  c0 = pil_clip8(a0); c1 = pil_clip8(a1); c2 = pil_clip8(a2);
}

// ---- device, colour: rgb2yuv + ToTensor + Normalize([.5, 0, 0], [.5, .5, .5]) in fp64 from c = byte / 255.0 of the three bytes -- a
// matrix row's three products summed left to right, ((y - 0.5) / 0.5, u / 0.5, v / 0.5) rounded once to fp32.  A caller that wants Y
// alone drops u and v (nothing is computed for them).  Contraction off: see the head of the file.
__device__ __forceinline__ void pil_yuv_norm(double cr, double cg, double cb, float& y, float& u, float& v) {
#pragma clang fp contract(off)
  const double y0 = cr * 0.299, y1 = cg * 0.587, y2 = cb * 0.114;
  const double yy = (y0 + y1) + y2;
  const double u0 = cr * -0.14714119, u1 = cg * -0.28886916, u2 = cb * 0.43601035;
  const double v0 = cr * 0.61497538, v1 = cg * -0.51496512, v2 = cb * -0.10001026;
  const double uu = (u0 + u1) + u2, vv = (v0 + v1) + v2;
  y = (float)((yy - 0.5) / 0.5); u = (float)(uu / 0.5); v = (float)(vv / 0.5);
}

// ---- host
// Pillow's precompute_coeffs: taps per output index of the BILINEAR filter, ceil(max(in / out, 1)) * 2 + 1, in 64-bit integers
// (csrc/patches.hip asks before it has bounded the frame: nothing may overflow for any int).  Equal to the fp64 form of data.py's
// bilinear_table wherever a launcher admits the sizes (scripts/ksize_agree.hip).
static inline long long pil_ksize(int in, int out) { return (in > out ? ((long long)in + out - 1) / out : 1LL) * 2 + 1; }

// source rows that the vertical taps of PIL_TR output rows can span
static inline int pil_rows_cap(int Hs, int H) {
  const double scale_y = (double)Hs / H, support_y = scale_y < 1.0 ? 1.0 : scale_y;
  const double span = (PIL_TR - 1) * scale_y + 2.0 * support_y;
  const int cap = (int)span + ((double)(int)span < span ? 1 : 0) + 2;
  return cap > PIL_ROWS_MAX ? PIL_ROWS_MAX : cap;
}

// staging pays where the row shrinks by more than about 3 (measured)
static inline bool pil_stage(int kx) { return kx >= PIL_STAGE_MIN_TAPS; }

// The refusals of a resize record that rcv_launch_batch_prep and rcv_launch_rgb_prep share, `who` in front ("batch prep", "rgb prep"):
// B images of Hs x Ws -> H x W out of the nsrc behind the frame pointer (slot: the name of the record's integer that holds nsrc),
// kx / ky taps as given; an indexed record brings its index (elements of idx_bytes) and its bad-index counter, which live for an epoch,
// as the tables do: a plan without them has nothing to gather by.
static inline int pil_check_record(const char* who, const char* slot, int B, int nsrc, int Hs, int Ws, int H, int W, int kx, int ky, bool indexed,
                                   int idx_bytes, const void* index, const void* bad) {
  RCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "%s: B %d, source %d x %d, output %d x %d: every size must be >= 1", who, B, Hs, Ws,
                H, W);
  RCV_CHECK_ARG(nsrc >= 1, "%s: a store of %d images (i[%s]): there must be at least 1", who, nsrc, slot);
  RCV_CHECK_ARG((long long)Hs <= 8LL * H && (long long)Ws <= 8LL * W,
                "%s: %d x %d -> %d x %d shrinks an axis by more than 8 (the kernel is built for at most %d taps)", who, Hs, Ws, H, W, PIL_MAXK);
  if (indexed)
    RCV_CHECK_ARG(idx_bytes == 4 || idx_bytes == 8, "%s: index element size %d unsupported (4 = int32, 8 = int64)", who, idx_bytes);
  const int wx = (int)pil_ksize(Ws, W), wy = (int)pil_ksize(Hs, H);
  RCV_CHECK_ARG(kx == wx && ky == wy, "%s: %d / %d taps per column / row given, %d -> %d and %d -> %d take %d / %d", who, kx, ky, Ws, W, Hs, H, wx, wy);
  RCV_CHECK_ARG((double)nsrc * Hs * Ws < 2147483647.0 && (double)B * H * W < 2147483647.0 &&
                    (double)B * ceil_div(W, PIL_TC) * ceil_div(H, PIL_TR) < 2147483647.0,
                "%s: %d images of %d x %d -> %d x %d: more than 2^31 pixels", who, nsrc > B ? nsrc : B, Hs, Ws, H, W);
  if (indexed) RCV_CHECK_ARG(index && bad, "%s: null index or null bad-index counter", who);
  return RCV_OK;
}
