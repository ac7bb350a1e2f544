// RCV_OP_OBJECT_PATCHES (rcv_object_patches): the step between RCV_OP_OBJECTS and the patch classifiers -- the box of every found
// object is cut out of the full-resolution frame and brought to the classifiers' input, one launch, one workgroup per slot of `rows`:
//   uint8 RGB frames [N][Hs][Ws][3], rows int32 [N][C-1][M][8], counts int32 [N][C-1][4]  ->  fp32 YUV [P][3][Sh][Sw] (+ uint8 [P][Sh][Sw][3]),
//   P = N (C-1) M.  The contract is restated in tests/patches_restatement.py and pinned to Pillow there:
//   0. slot (n, c, k) is valid iff k < min(counts[n][c][3], M); an invalid slot is zero in every output (written here: nothing is
//      pre-zeroed);
//   1. the box in class-map pixels (map H x W), every value clamped where it is used: x0 = clamp(x - margin, 0, W - 1),
//      x1 = clamp(x + w + margin, x0 + 1, W); y0, y1 likewise with H -- no row content can address outside the frame;
//   2. the box in frame pixels, fp64, one division each: fx0 = (x0 Ws) / W, fx1 = (x1 Ws) / W, fy0 = (y0 Hs) / H, fy1 = (y1 Hs) / H;
//   3. Pillow's resize((Sw, Sh), BILINEAR, box = (fx0, fy0, fx1, fy1)): per axis precompute_coeffs with the box offset, in fp64 --
//      scale = (in1 - in0) / out, support = max(scale, 1), center = in0 + (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
//      xmax = min(int(center + support + 0.5), inSize), triangle weights summed left to right, each divided by the sum, then
//      int(0.5 + w 2^22); the horizontal pass first, the vertical pass second, each from 2^21, int32 sums, >> 22, clipped to a byte;
//   4. step 4 of csrc/rgb_prep.hip (pil_yuv_norm of csrc/pil_resize.h, the one both files call): c = byte / 255.0 in fp64, a matrix
//      row's three products summed left to right, ((y - 0.5) / 0.5, u / 0.5, v / 0.5) rounded once to fp32.
// The clamps, the 22-bit rounding and the tap count are that header's too; the box coefficient builder, the chunked walk and the text
// of the guarded 16-byte load (pt_load16: see there) are this file's own.
//
// The workgroup (256 threads) reads its box, builds the two coefficient tables in LDS as int32 (threads 0..Sw-1 one row of the x
// table each, threads 64..64+Sh-1 one row of the y table: a row is a sequential fp64 sum, the rows are independent), then walks the
// source rows under the box in chunks of PT_CHUNK: the horizontal pass of a chunk goes to LDS as bytes, the vertical pass adds the
// chunk's share to accumulators that stay in registers across chunks.  The horizontal taps read row segments staged in LDS: a batch
// of rows (up to 32 KiB) is loaded with 16-byte aligned loads into registers and stored to LDS, and the loads of the next batch are
// in flight while the taps of this one run -- one workgroup has nobody else on its compute unit to hide a load behind (DESIGN
// §4.12).  A thread owns the output pixels tid + 256 j, j < NPP (a template argument: the accumulator array is indexed by unrolled
// constants only, it never lives in scratch memory); the sums are integers, so the order of the chunks fixes nothing.  The row
// width of the tables follows from the FRAME at enqueue time (Kmax = ceil(in / out) 2 + 1: no box is larger than its frame), so the
// LDS carve is the same for every slot of a launch.
//
// Workgroups of very different cost run side by side (a ball next to a robot that fills the frame); that is accepted.
//
// Roundings: floating-point contraction is off for this file (the pragma below): a fused multiply-add in in0 + (xx + 0.5) scale
// changes bytes.  fp64 division and the conversions are correctly rounded / truncating on this hardware as on the host.
#include "rcv_internal.h"

#pragma clang fp contract(off)

#include "pil_resize.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_CHUNK = 64;             // source rows whose horizontal pass is held in LDS at a time
constexpr int PT_MAXS = 64;              // largest patch side

constexpr int PT_LD = 8;                 // 16-byte words of source rows a thread holds in registers per batch
constexpr int PT_STAGE_WORDS = PT_THREADS * PT_LD;      // words of a batch: 32 KiB of LDS

struct PtArgs {
  const uint8_t* frames; const int32_t* rows; const int32_t* counts; float* images; uint8_t* bytes;
  size_t frames_bytes;                   // N Hs Ws 3: the aligned staging loads stay inside the buffer
  int Hs, Ws, H, W, Sh, Sw, M, margin, kx, ky, slots_per_image;
};

__host__ __device__ inline int pt_round4(int v) { return (v + 3) & ~3; }
__host__ __device__ inline int pt_round16(int v) { return (v + 15) & ~15; }
// dynamic LDS: x table [Sw][2 + kx] | y table [Sh][2 + ky] | horizontal-pass bytes [PT_CHUNK][Sw][3] | staged source rows
// [PT_STAGE_WORDS] x 16 bytes; every carve a multiple of 16 bytes
__host__ __device__ inline size_t pt_table_bytes(int Sh, int Sw, int kx, int ky) {
  return ((size_t)pt_round4(Sw * (2 + kx)) + (size_t)pt_round4(Sh * (2 + ky))) * 4;
}
__host__ __device__ inline size_t pt_lds_bytes(int Sh, int Sw, int kx, int ky) {
  return pt_table_bytes(Sh, Sw, kx, ky) + (size_t)pt_round16(PT_CHUNK * Sw * 3) + (size_t)PT_STAGE_WORDS * 16;
}

__device__ __forceinline__ long long pt_clampl(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one triangle weight of precompute_coeffs
__device__ __forceinline__ double pt_weight(int x, double center, double ss) {
  const double d = ((double)x - center) + 0.5;
  const double t = fabs(d * ss);
  return t < 1.0 ? 1.0 - t : 0.0;
}

// row xx of one axis' table: {first tap, tap count, K coefficients}
__device__ __forceinline__ void pt_coeff_row(int inSize, double in0, double in1, int outSize, int K, int xx, int32_t* row) {
  const double scale = (in1 - in0) / (double)outSize;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double ss = 1.0 / support;
  const double off = ((double)xx + 0.5) * scale;
  const double center = in0 + off;
  const double lo = center - support, hi = center + support;
  const int xmin = pil_clampi((int)(lo + 0.5), 0, inSize - 1);
  const int xmax = min((int)(hi + 0.5), inSize);
  const int n = pil_clampi(xmax - xmin, 0, K);
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += pt_weight(x + xmin, center, ss);
  row[0] = xmin; row[1] = n;
  for (int x = 0; x < n; ++x) {
    double w = pt_weight(x + xmin, center, ss);
    if (ww != 0.0) w = w / ww;
    row[2 + x] = (int)(0.5 + w * 4194304.0);
  }
}

// pil_load16 (csrc/pil_resize.h) with the four words named: the same values, kept here because with the header's array form the
// unrolled register batches below are scheduled differently and the full-frame launch measured 0.9 % slower
__device__ __forceinline__ uint4 pt_load16(uintptr_t va, uintptr_t lo, uintptr_t hi) {
  if (va >= lo && va + 16 <= hi) return *reinterpret_cast<const uint4*>(va);
  uint32_t d0 = 0u, d1 = 0u, d2 = 0u, d3 = 0u;
  for (int q = 0; q < 16; ++q) {
    const uintptr_t ad = va + q;
    const uint32_t bv = (ad >= lo && ad < hi) ? (uint32_t)(*reinterpret_cast<const uint8_t*>(ad)) << (8 * (q & 3)) : 0u;
    if (q < 4) d0 |= bv; else if (q < 8) d1 |= bv; else if (q < 12) d2 |= bv; else d3 |= bv;
  }
  return make_uint4(d0, d1, d2, d3);
}

// a batch of source-row segments into registers: word i = tid + 256 j (i < words) is word i % nv of row i / nv, rows `pitch` bytes
// apart from `first` (the segment's first byte in the first row), each segment segb bytes from the aligned word below its start
__device__ __forceinline__ void pt_batch_load(uint4 (&w)[PT_LD], const uint8_t* first, size_t pitch, int words, int nv, int segb,
                                              uintptr_t lo, uintptr_t hi) {
#pragma unroll
  for (int j = 0; j < PT_LD; ++j) {
    const int i = threadIdx.x + PT_THREADS * j;
    w[j] = make_uint4(0u, 0u, 0u, 0u);
    if (i < words) {
      const int rr = i / nv, v = i - rr * nv;
      const uintptr_t A = (uintptr_t)(first + (size_t)rr * pitch);
      const uintptr_t va = (A & ~(uintptr_t)15) + 16u * (uintptr_t)v;
      if (va < A + segb) w[j] = pt_load16(va, lo, hi);
    }
  }
}

// Grid: P workgroups.  NPP: output pixels per thread, ceil(Sh Sw / 256) <= NPP.
template <int NPP>
__global__ __launch_bounds__(PT_THREADS) void object_patches_kernel(PtArgs a) {
  extern __shared__ __attribute__((aligned(16))) char pt_sh[];
  const int tid = threadIdx.x;
  const size_t slot = blockIdx.x;
  const int npix = a.Sh * a.Sw;
  float* img = a.images + slot * 3 * (size_t)npix;
  uint8_t* byt = a.bytes ? a.bytes + slot * 3 * (size_t)npix : nullptr;
  const size_t oc = slot / a.M;
  const int k = (int)(slot - oc * a.M);
  if (k >= a.counts[oc * 4 + 3]) {              // (k < M always) an invalid slot: zeros, written here
    for (int i = tid; i < 3 * npix; i += PT_THREADS) {
      img[i] = 0.f;
      if (byt) byt[i] = 0;
    }
    return;
  }
  const int sx = 2 + a.kx, sy = 2 + a.ky;
  int32_t* s_xc = reinterpret_cast<int32_t*>(pt_sh);
  int32_t* s_yc = s_xc + pt_round4(a.Sw * sx);
  uint8_t* s_h = reinterpret_cast<uint8_t*>(s_yc + pt_round4(a.Sh * sy));
  uint8_t* s_src = s_h + pt_round16(PT_CHUNK * a.Sw * 3);

  // steps 1 and 2 (W Ws and H Hs fit int32: refused otherwise)
  const int32_t* row = a.rows + slot * 8;
  const long long bx = row[0], by = row[1], bw = row[2], bh = row[3];
  const int x0 = (int)pt_clampl(bx - a.margin, 0, a.W - 1), x1 = (int)pt_clampl(bx + bw + a.margin, x0 + 1, a.W);
  const int y0 = (int)pt_clampl(by - a.margin, 0, a.H - 1), y1 = (int)pt_clampl(by + bh + a.margin, y0 + 1, a.H);
  const double fx0 = (double)(x0 * a.Ws) / (double)a.W, fx1 = (double)(x1 * a.Ws) / (double)a.W;
  const double fy0 = (double)(y0 * a.Hs) / (double)a.H, fy1 = (double)(y1 * a.Hs) / (double)a.H;

  // step 3: the tables (waves 0 and 1 side by side)
  if (tid < a.Sw) pt_coeff_row(a.Ws, fx0, fx1, a.Sw, a.kx, tid, s_xc + tid * sx);
  if (tid >= 64 && tid - 64 < a.Sh) pt_coeff_row(a.Hs, fy0, fy1, a.Sh, a.ky, tid - 64, s_yc + (tid - 64) * sy);
  __syncthreads();

  int acc[NPP][3];
#pragma unroll
  for (int j = 0; j < NPP; ++j) { acc[j][0] = 1 << (PIL_PREC - 1); acc[j][1] = 1 << (PIL_PREC - 1); acc[j][2] = 1 << (PIL_PREC - 1); }

  const int n_img = (int)(slot / a.slots_per_image);
  const uint8_t* fb = a.frames + (size_t)n_img * a.Hs * a.Ws * 3;
  const int ys0 = pil_clampi(s_yc[0], 0, a.Hs - 1);
  const int ys1 = pil_clampi(s_yc[(a.Sh - 1) * sy] + s_yc[(a.Sh - 1) * sy + 1], ys0 + 1, a.Hs);
  // source pixels under the box's horizontal taps: [xs0, xs0 + segpix)
  const int xs0 = pil_clampi(s_xc[0], 0, a.Ws - 1);
  const int xs1 = pil_clampi(s_xc[(a.Sw - 1) * sx] + s_xc[(a.Sw - 1) * sx + 1], xs0 + 1, a.Ws);
  const int segpix = xs1 - xs0, segb = segpix * 3;
  const int nv = (segb + 30) / 16;               // 16-byte words that hold a row's segment starting up to 15 bytes into the first
  const int rb = pil_clampi(PT_STAGE_WORDS / nv, 1, PT_CHUNK);      // source rows per batch (nv <= PT_STAGE_WORDS: refused otherwise)
  const uintptr_t lo = (uintptr_t)a.frames, hi = lo + a.frames_bytes;
  const uint8_t* seg0 = fb + (size_t)xs0 * 3;
  const size_t pitch = (size_t)a.Ws * 3;

  // The source rows [ys0, ys1) go through LDS in batches of at most rb rows that never straddle a chunk: a batch is loaded into
  // registers (16-byte aligned words, PT_LD per thread), stored to s_src as [row][nv words], and while its taps run the loads of
  // the next batch are already in flight.  At the end of a chunk the vertical pass adds the chunk's share.
  int row0 = ys0;
  int nb = min(rb, min(PT_CHUNK, ys1 - ys0));
  uint4 w[PT_LD];
  pt_batch_load(w, seg0 + (size_t)row0 * pitch, pitch, nb * nv, nv, segb, lo, hi);
  while (row0 < ys1) {
#pragma unroll
    for (int j = 0; j < PT_LD; ++j) {
      const int i = tid + PT_THREADS * j;
      if (i < nb * nv) *reinterpret_cast<uint4*>(s_src + 16 * i) = w[j];
    }
    __syncthreads();      // (also: the vertical pass of the chunk before is through with s_h)
    const int c0 = ys0 + (row0 - ys0) / PT_CHUNK * PT_CHUNK, c1 = min(c0 + PT_CHUNK, ys1);      // this batch's chunk
    const int row1 = row0 + nb;
    int nb1 = 0;
    if (row1 < ys1) {
      nb1 = min(rb, (row1 < c1 ? c1 : min(c1 + PT_CHUNK, ys1)) - row1);
      pt_batch_load(w, seg0 + (size_t)row1 * pitch, pitch, nb1 * nv, nv, segb, lo, hi);
    }
    // the horizontal pass of source rows [row0, row1) into s_h[row - c0][x][c]
    for (int i = tid; i < nb * a.Sw; i += PT_THREADS) {
      const int rr = i / a.Sw, x = i - rr * a.Sw;
      const int32_t* xc = s_xc + x * sx;
      const int rel = pil_clampi(xc[0] - xs0, 0, segpix - 1);
      const int xn = min(pil_clampi(xc[1], 0, a.kx), segpix - rel);
      const uintptr_t A = (uintptr_t)(seg0 + (size_t)(row0 + rr) * pitch);
      const uint8_t* p = s_src + 16 * nv * rr + (int)(A & 15) + rel * 3;
      int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
#pragma unroll 4
      for (int t = 0; t < xn; ++t) {
        const int c = xc[2 + t];
        a0 += (int)p[3 * t] * c; a1 += (int)p[3 * t + 1] * c; a2 += (int)p[3 * t + 2] * c;
      }
      uint8_t* q = s_h + ((row0 - c0 + rr) * a.Sw + x) * 3;
      q[0] = (uint8_t)pil_clip8(a0); q[1] = (uint8_t)pil_clip8(a1); q[2] = (uint8_t)pil_clip8(a2);
    }
    __syncthreads();
    if (row1 == c1) {       // (uniform) the chunk [c0, c1) is complete: its share of the vertical pass
#pragma unroll
      for (int j = 0; j < NPP; ++j) {
        const int p = tid + PT_THREADS * j;
        if (p < npix) {
          const int y = p / a.Sw, x = p - y * a.Sw;
          const int32_t* yc = s_yc + y * sy;
          const int yf = pil_clampi(yc[0], 0, a.Hs - 1), yn = pil_clampi(yc[1], 0, a.ky);
          const int r0 = max(yf, c0), r1 = min(yf + yn, c1);
          int a0 = acc[j][0], a1 = acc[j][1], a2 = acc[j][2];
          for (int r = r0; r < r1; ++r) {
            const int c = yc[2 + r - yf];
            const uint8_t* q = s_h + ((r - c0) * a.Sw + x) * 3;
            a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
          }
          acc[j][0] = a0; acc[j][1] = a1; acc[j][2] = a2;
        }
      }
    }
    row0 = row1; nb = nb1;
  }

  // step 4 and the stores: planes contiguous over the lanes
#pragma unroll
  for (int j = 0; j < NPP; ++j) {
    const int p = tid + PT_THREADS * j;
    if (p < npix) {
      const int r = pil_clip8(acc[j][0]), g = pil_clip8(acc[j][1]), b = pil_clip8(acc[j][2]);
      if (byt) { byt[3 * p] = (uint8_t)r; byt[3 * p + 1] = (uint8_t)g; byt[3 * p + 2] = (uint8_t)b; }
      pil_yuv_norm((double)r / 255.0, (double)g / 255.0, (double)b / 255.0, img[p], img[npix + p], img[2 * npix + p]);
    }
  }
}

}  // namespace

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_OBJECT_PATCHES).  Record:
//   i: N, H = Hs, W = Ws (the frames); HO = H, WO = W (the class map the boxes live in); COUT = C - 1; COUNT = M; AUX0 = Sh, AUX1 = Sw;
//      CIN = margin
//   p: IN = frames uint8 [N][Hs][Ws][3], IN2 = rows int32 [N][C-1][M][8], X0 = counts int32 [N][C-1][4], OUT = images float
//      [P][3][Sh][Sw], X1 = bytes uint8 [P][Sh][Sw][3] or NULL
// No workspace.  Every refusal that depends on the shape of the record sits in front of the query return.
// --------------------------------------------------------------------------------------------
int rcv_launch_object_patches(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "object patches";
  const int N = op->i[RCV_I_N], Hs = op->i[RCV_I_H], Ws = op->i[RCV_I_W], H = op->i[RCV_I_HO], W = op->i[RCV_I_WO];
  const int Cm1 = op->i[RCV_I_COUT], M = op->i[RCV_I_COUNT], Sh = op->i[RCV_I_AUX0], Sw = op->i[RCV_I_AUX1], margin = op->i[RCV_I_CIN];
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), "object_patches");
  }
  RCV_CHECK_ARG(N >= 1 && M >= 1 && Cm1 >= 1, "%s: %d frames, %d classes with boxes, %d rows per class: every count must be >= 1", what, N, Cm1, M);
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(Sh >= 1 && Sh <= PT_MAXS && Sw >= 1 && Sw <= PT_MAXS, "%s: patch size %d x %d unsupported (each side 1..%d)", what, Sh, Sw, PT_MAXS);
  RCV_CHECK_ARG(margin >= 0, "%s: margin %d must be >= 0", what, margin);
  RCV_CHECK_ARG(Hs >= 1 && Ws >= 1, "%s: frames of %d x %d: every size must be >= 1", what, Hs, Ws);
  RCV_CHECK_ARG(H >= 1 && H <= Hs && W >= 1 && W <= Ws, "%s: a class map of %d x %d does not fit frames of %d x %d (1..Hs, 1..Ws)", what, H, W, Hs, Ws);
  RCV_CHECK_ARG((long long)W * Ws <= 2147483647LL && (long long)H * Hs <= 2147483647LL,
                "%s: map %d x %d times frame %d x %d: a box corner times the frame size can pass 32 bits", what, H, W, Hs, Ws);
  RCV_CHECK_ARG((double)N * Cm1 * M < 2147483647.0, "%s: %d x %d x %d slots: more than 2^31", what, N, Cm1, M);
  const long long kxl = pil_ksize(Ws, Sw), kyl = pil_ksize(Hs, Sh);      // of a whole axis: no box of the frame takes more taps per output index
  RCV_CHECK_ARG((3LL * Ws + 30) / 16 <= PT_STAGE_WORDS, "%s: a source row of %d pixels does not fit the %d-byte staging buffer in LDS", what, Ws,
                PT_STAGE_WORDS * 16);
  const long long ldsl = ((2 + kxl) * Sw + (2 + kyl) * Sh + 8) * 4 + PT_CHUNK * Sw * 3 + 16 + PT_STAGE_WORDS * 16;      // >= pt_lds_bytes, no overflow
  RCV_CHECK_ARG(ldsl <= (long long)h->max_lds,
                "%s: the coefficient tables of %d x %d -> %d x %d (%lld / %lld taps per column / row) need %lld bytes of LDS with the row buffers, %d available",
                what, Hs, Ws, Sh, Sw, kxl, kyl, ldsl, h->max_lds);
  const int kx = (int)kxl, ky = (int)kyl;
  const size_t lds = pt_lds_bytes(Sh, Sw, kx, ky);
  const int npp = Sh * Sw <= 4 * PT_THREADS ? 4 : 16;
  if (query) {
    snprintf(query->label, sizeof(query->label), "object_patches<%d>", npp);
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_X0] && op->p[RCV_P_OUT], "%s: null operand", what);
  RCV_CHECK_ARG((((uintptr_t)op->p[RCV_P_IN2] | (uintptr_t)op->p[RCV_P_X0] | (uintptr_t)op->p[RCV_P_OUT]) & 3) == 0,
                "%s: rows / counts / images not 4-byte aligned", what);
  PtArgs a;
  a.frames = (const uint8_t*)op->p[RCV_P_IN]; a.rows = (const int32_t*)op->p[RCV_P_IN2]; a.counts = (const int32_t*)op->p[RCV_P_X0];
  a.images = (float*)op->p[RCV_P_OUT]; a.bytes = (uint8_t*)op->p[RCV_P_X1];
  a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.Sh = Sh; a.Sw = Sw; a.M = M; a.margin = margin; a.kx = kx; a.ky = ky; a.slots_per_image = Cm1 * M;
  a.frames_bytes = (size_t)N * Hs * Ws * 3;
  const dim3 grid(N * Cm1 * M), block(PT_THREADS);
  if (npp == 4) {
    static size_t configured[RCV_MAX_DEVICES];
    RCV_ENSURE_LDS(object_patches_kernel<4>, lds, h->device, configured);
    hipLaunchKernelGGL(object_patches_kernel<4>, grid, block, lds, s, a);
  } else {
    static size_t configured[RCV_MAX_DEVICES];
    RCV_ENSURE_LDS(object_patches_kernel<16>, lds, h->device, configured);
    hipLaunchKernelGGL(object_patches_kernel<16>, grid, block, lds, s, a);
  }
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
