// RCV_OP_RGB_PREP (rcv_rgb_prep): the RGB loader of trainer.py:75-123 (SSDataSet with the transforms of trainer.py / pruner.py /
// labelPropTrain.py / tester.py / makeLPImages.py / classTrainer.py / objDetEval.py) for a whole batch:
//   uint8 RGB frames [B][Hs][Ws][3] (+ label planes [B][Hs][Ws], uint8 / int32)  ->  fp32 NCHW YUV [B][3][H][W] (+ int64 targets [B][H][W]).
// Per image, in the reference's order (the contract is restated in tests/rgb_prep_restatement.py and pinned to Pillow there):
//   1. Scale: Pillow's 8-bit BILINEAR resize as two integer passes from host-made tables (csrc/pil_resize.h);
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
// m = floor((2 sum + n) / (2 n)) and does everything.  Both go through pil_horizontal / pil_vertical / rp_ops.  The statistics launch
// is skipped when the record says that no row holds a contrast (validation mode, rcv.h i[COUNT]).
//
// The resize, its tile (one workgroup = 8 output rows x 64 output columns of one image, lane = output x), the label gather, maskLabel,
// the index test and step 4's arithmetic are csrc/pil_resize.h's, shared with csrc/batch_prep.hip (step 4: with csrc/patches.hip);
// this file holds steps 2, 3 and 5 and the launchers.  The plane stores are contiguous over the lanes (reversed under a horizontal flip).
//
// RCV_OP_RGB_PREP_IDX (rcv_rgb_prep_indexed) takes image b from store[index[b]]: the index is read from device memory and tested against
// [0, N) before it forms an address, in both launches (a 0 partial; a zero image with zero targets, counted once).  The kernels are
// instantiated with the index off for RCV_OP_RGB_PREP.
// RCV_OP_LP_PAIR_PREP (rcv_lp_pair_prep) is at the end of the file: both frames of a LabelProp pair through steps 2-5 with ONE row, Y only,
// then the assembly of labelPropTrain.py:162-193, from a store that is already at the network's size.
//
// Roundings: this file is compiled with floating-point contraction off (the pragma below): every product that feeds a sum is rounded
// on its own.  __fmul_rn and its kin would not do: the header defines them as the plain operators, which the compiler may fuse.
#include "rcv_internal.h"

#pragma clang fp contract(off)

#include "pil_resize.h"

#define RP_PAIR_PIX 512                  /* pixels of both frames of a pair per workgroup of lp_pair_prep_kernel */
#define RP_NPAR 12                       /* floats of a parameter row */

struct RpArgs {
  const uint8_t* frames; const void* labels; float* imgs; int64_t* tgt;
  const int32_t* xtab; const int32_t* ytab; const int32_t* lx; const int32_t* ly; const float* params; uint32_t* part;
  int B, Hs, Ws, H, W, kx, ky, lab_bytes, train, mask, rows_cap, tiles_x, tiles_y, stats, wpi;      // wpi: workgroups per image
  // the indexed forms (behind everything the plain kernels read, whose argument offsets stay as they were)
  int nsrc;                                 // images behind `frames` / `labels`: the N of the store
  int idx_bytes; const void* index; int* bad;          // index [B] (pairs [B][2]) of 4 / 8 byte elements, counter of the refused ones
};

enum { RP_PLAIN = 0, RP_IDX = 1, RP_PAIR = 2 };          // the form a kernel is instantiated for

// the parameter row of an image; ops = the four op codes, 4 bits each (15 = none; no indexed array: it would live in scratch memory);
// cpos = position of the first contrast among its operations, -1 = none (uniform over a workgroup)
struct RpRow { bool hflip, vflip; int n_ops, cpos, ops, shift; float fb, fc, fs; };

__device__ __forceinline__ RpRow rp_row(const RpArgs& a, int b) {
  RpRow j;
  j.hflip = false; j.vflip = false; j.n_ops = 0; j.cpos = -1; j.ops = 0xffff; j.shift = 0; j.fb = 1.f; j.fc = 1.f; j.fs = 1.f;
  if (a.train) {
    const float* p = a.params + (size_t)b * RP_NPAR;
    j.hflip = p[0] != 0.f; j.vflip = p[1] != 0.f;
    j.n_ops = pil_clampi((int)p[2], 0, 4);
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
__device__ __forceinline__ int rp_rnd8(float v) { return pil_clampi((int)((double)v + 0.5), 0, 255); }

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
    Hh = pil_clampi((int)((double)hf * 255.0), 0, 255);
    S = pil_clampi((int)((double)s * 255.0), 0, 255);
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

// steps 4 and 5 for one output pixel (x, y: coordinates before the mirrors) of batch row b (image src of `labels`) from its bytes after
// step 3; s_c[v] = v / 255.0
__device__ __forceinline__ void rp_finish(const RpArgs& a, const RpRow& j, const double* s_c, int b, int src, int y, int x, int r, int g, int bl) {
  float yy, uu, vv;
  pil_yuv_norm(s_c[r], s_c[g], s_c[bl], yy, uu, vv);
  const int xo = j.hflip ? a.W - 1 - x : x, yo = j.vflip ? a.H - 1 - y : y;
  const size_t plane = (size_t)a.H * a.W, o = (size_t)yo * a.W + xo;
  float* img = a.imgs + (size_t)b * 3 * plane + o;
  img[0] = yy; img[plane] = uu; img[2 * plane] = vv;
  if (!a.tgt) return;                      // the patch chain: no label plane (uniform over the launch)
  a.tgt[(size_t)b * plane + o] = (int64_t)pil_mask_label(pil_label(a, src, y, x), a.mask);
}

// STATS: the statistics launch (one partial sum of L per workgroup); otherwise the main launch.  STAGE: see pil_horizontal.
// FORM: RP_PLAIN, or RP_IDX (image b is store[index[b]]).  Grid: B * tiles_x * tiles_y.
template <bool STATS, bool STAGE, int FORM>
__global__ __launch_bounds__(256) void rgb_prep_kernel(RpArgs a) {
  __shared__ double s_c[256];
  __shared__ unsigned long long s_red[256];
  __shared__ int32_t s_xc[PIL_TC * (2 + PIL_MAXK)];
  __shared__ int32_t s_yc[PIL_TR * (2 + PIL_MAXK)];
  __shared__ uint8_t s_h[PIL_ROWS_MAX * PIL_TC * 3];
  __shared__ __align__(16) uint8_t s_src[STAGE ? PIL_RC * PIL_SEG : 16];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.wpi, tile = blockIdx.x % a.wpi;
  PilTile t = pil_tile(a, tile % a.tiles_x, tile / a.tiles_x);
  int src = b;
  if (FORM == RP_IDX) {
    src = pil_source(a, (size_t)b);
    if (src < 0) {                               // (the same for the whole workgroup, and in front of every barrier)
      if (STATS) {
        if (tid == 0) a.part[blockIdx.x] = 0u;
        return;
      }
      pil_zero_tile(a, b, t);
      if (tile == 0 && tid == 0) atomicAdd(a.bad, 1);
      return;
    }
  }
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
  pil_horizontal<STAGE>(a, src, FORM == RP_IDX ? a.nsrc : a.B, t, s_xc, s_yc, s_h, s_src);
  const int x = tid & (PIL_TC - 1);
  unsigned long long lsum = 0;
  for (int idx = tid; idx < t.th * PIL_TC; idx += 256) {
    const int yl = idx >> 6;
    if (x >= t.tw) continue;
    int r, g, bl;
    pil_vertical(a, t, s_yc, s_h, yl, x, r, g, bl);
    if (STATS) {
      rp_ops(j, j.cpos, 0, r, g, bl);
      lsum += (unsigned long long)rp_luma(r, g, bl);
    } else {
      rp_ops(j, j.n_ops, m, r, g, bl);
      rp_finish(a, j, s_c, b, src, t.y0 + yl, t.x0 + x, r, g, bl);
    }
  }
  if (STATS) {
    const unsigned long long s = rp_block_sum(lsum, s_red);      // <= 512 * 255
    if (tid == 0) a.part[blockIdx.x] = (uint32_t)s;
  }
}

// H == Hs and W == Ws: no resize (transform.py:15-16); one thread per pixel, PIL_IDENT_PIX pixels of one image per workgroup.
// FORM: RP_PLAIN, RP_IDX, or (STATS only) RP_PAIR: the statistics launch of RCV_OP_LP_PAIR_PREP -- image b is frame b & 1 of pair b >> 1,
// its row is the pair's, and a pair with either index outside the store leaves 0 partials for both its frames.
template <bool STATS, int FORM>
__global__ __launch_bounds__(256) void rgb_prep_ident_kernel(RpArgs a) {
  __shared__ double s_c[256];
  __shared__ unsigned long long s_red[256];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.wpi, blk = blockIdx.x % a.wpi;
  int src = b;
  if (FORM != RP_PLAIN) {
    src = pil_source(a, (size_t)b);
    const bool bad = src < 0 || (FORM == RP_PAIR && pil_source(a, (size_t)(b ^ 1)) < 0);
    if (bad) {                                   // (the same for the whole workgroup, and in front of every barrier)
      if (STATS) {
        if (tid == 0) a.part[blockIdx.x] = 0u;
        return;
      }
      const int start = blk * PIL_IDENT_PIX, end = start + min(PIL_IDENT_PIX, a.H * a.W - start);
      for (int p = start + tid; p < end; p += 256) pil_zero(a, b, p / a.W, p % a.W);
      if (blk == 0 && tid == 0) atomicAdd(a.bad, 1);
      return;
    }
  }
  const RpRow j = rp_row(a, FORM == RP_PAIR ? b >> 1 : b);
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
  const uint8_t* fb = a.frames + (size_t)src * npix * 3;
  const int start = blk * PIL_IDENT_PIX, end = start + min(PIL_IDENT_PIX, npix - start);
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
      rp_finish(a, j, s_c, b, src, y, x, r, g, bl);
    }
  }
  if (STATS) {
    const unsigned long long s = rp_block_sum(lsum, s_red);      // <= 2048 * 255
    if (tid == 0) a.part[blockIdx.x] = (uint32_t)s;
  }
}

// Every refusal that depends on the shape of the record, and the tables, sits in front of the `query` return (what rcv_batch_prep
// refuses is refused here); the batch operands are checked at launch.
int rcv_launch_rgb_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], Hs = op->i[RCV_I_H], Ws = op->i[RCV_I_W], H = op->i[RCV_I_HO], W = op->i[RCV_I_WO];
  const int kx = op->i[RCV_I_CIN], ky = op->i[RCV_I_COUT], lab_bytes = op->i[RCV_I_INMODE2];
  const int train = op->i[RCV_I_AUX0], mask = op->i[RCV_I_AUX1], stats = op->i[RCV_I_COUNT];
  const bool with_labels = lab_bytes != 0;
  // RCV_OP_RGB_PREP_IDX (rcv_rgb_prep_indexed): images picked from a store of i[STRIDE] images
  const bool indexed = op->kind == RCV_OP_RGB_PREP_IDX;
  const int nsrc = indexed ? op->i[RCV_I_STRIDE] : B;          // images behind p[IN] / p[IN2]
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), indexed ? "rgb_prep_idx" : "rgb_prep");
  }
  if (const int e = pil_check_record("rgb prep", "STRIDE", B, nsrc, Hs, Ws, H, W, kx, ky, indexed, op->i[RCV_I_INMODE], op->p[RCV_P_IN_AUX],
                                     op->p[RCV_P_EPI_AUX]))
    return e;
  RCV_CHECK_ARG(lab_bytes == 0 || lab_bytes == 1 || lab_bytes == 4,
                "rgb prep: label element size %d unsupported (1 = uint8, 4 = int32, 0 = no labels)", lab_bytes);
  RCV_CHECK_ARG((train == 0 || train == 1) && mask >= 0 && mask <= 15 && (stats == 0 || stats == 1),
                "rgb prep: train %d / maskLabel flags %d / statistics %d out of range", train, mask, stats);
  if (with_labels)
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2] && op->p[RCV_P_X3] && op->p[RCV_P_X4],
                  "rgb prep: null table (frame taps of x / y, label index of x / y)");
  else
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2], "rgb prep: null table (frame taps of x / y)");
  const int tiles_x = ceil_div(W, PIL_TC), tiles_y = ceil_div(H, PIL_TR);
  const bool ident = H == Hs && W == Ws;
  const int wpi = ident ? ceil_div(H * W, PIL_IDENT_PIX) : tiles_x * tiles_y;
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
  a.nsrc = nsrc; a.idx_bytes = 0; a.index = nullptr; a.bad = nullptr;
  if (indexed) { a.index = op->p[RCV_P_IN_AUX]; a.idx_bytes = op->i[RCV_I_INMODE]; a.bad = (int*)op->p[RCV_P_EPI_AUX]; }
  const dim3 grid(B * wpi), block(256);
  if (ident) {
    void (*stat_ident)(RpArgs) = rgb_prep_ident_kernel<true, RP_PLAIN>;
    void (*main_ident)(RpArgs) = rgb_prep_ident_kernel<false, RP_PLAIN>;
    if (indexed) { stat_ident = rgb_prep_ident_kernel<true, RP_IDX>; main_ident = rgb_prep_ident_kernel<false, RP_IDX>; }
    if (two) hipLaunchKernelGGL(stat_ident, grid, block, 0, s, a);
    hipLaunchKernelGGL(main_ident, grid, block, 0, s, a);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  a.rows_cap = pil_rows_cap(Hs, H);
  const bool stage = pil_stage(kx);
  void (*stat_kernel)(RpArgs) = stage ? rgb_prep_kernel<true, true, RP_PLAIN> : rgb_prep_kernel<true, false, RP_PLAIN>;
  void (*main_kernel)(RpArgs) = stage ? rgb_prep_kernel<false, true, RP_PLAIN> : rgb_prep_kernel<false, false, RP_PLAIN>;
  if (indexed) {
    stat_kernel = stage ? rgb_prep_kernel<true, true, RP_IDX> : rgb_prep_kernel<true, false, RP_IDX>;
    main_kernel = stage ? rgb_prep_kernel<false, true, RP_IDX> : rgb_prep_kernel<false, false, RP_IDX>;
  }
  if (two) hipLaunchKernelGGL(stat_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(main_kernel, grid, block, 0, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}

// ------------------------------------------------------------------------------------------
// RCV_OP_LP_PAIR_PREP (rcv_lp_pair_prep): the store's bytes -> LabelProp's input.  Per pair p = (ia, ib) of store indices, with ONE
// parameter row (labelPropTrain.py:36-66 for both frames, then labelPropTrain.py:162-193):
//   both frames and both label planes through steps 2-5 above with row p -- the same mirrors for all four planes, the same colour
//   operations on both frames, the contrast mean of EACH FRAME ON ITS OWN (ColorJitter is applied per image) -- Y only; then
//   sample 2p = [Ya, Yb, Ya - Yb, labelToPred(label_b)], target label_a; sample 2p + 1 = [Yb, Ya, Yb - Ya, labelToPred(label_a)], target
//   label_b, NHWC with 8 floats per pixel, as lp_batch_kernel of csrc/lp_tail.hip writes them.
// The statistics launch is rgb_prep_ident_kernel<true, RP_PAIR> over the 2B frames (partials [2B][wpi]).  Here one workgroup handles the
// same RP_PAIR_PIX pixels of both frames of a pair (fewer than the statistics launch takes: 8 pairs of 120 x 160 are 304 workgroups
// instead of 80 on 256 compute units); a thread writes the two 32-byte pixels with four 16-byte stores.  Grid: B * bpp.
__global__ __launch_bounds__(256) void lp_pair_prep_kernel(RpArgs a, int bpp) {
  __shared__ double s_c[256];
  __shared__ unsigned long long s_red[256];
  const int tid = threadIdx.x;
  const int pr = blockIdx.x / bpp, blk = blockIdx.x % bpp;
  const int npix = a.H * a.W;
  const int start = blk * RP_PAIR_PIX, end = start + min(RP_PAIR_PIX, npix - start);
  const int sa = pil_source(a, (size_t)2 * pr), sb = pil_source(a, (size_t)2 * pr + 1);
  float* out0 = a.imgs + (size_t)2 * pr * npix * 8;
  float* out1 = out0 + (size_t)npix * 8;
  int64_t* tgt0 = a.tgt + (size_t)2 * pr * npix;
  int64_t* tgt1 = tgt0 + npix;
  if (sa < 0 || sb < 0) {                        // (the same for the whole workgroup, and in front of every barrier)
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = start + tid; p < end; p += 256) {
      float4* o0 = (float4*)(out0 + (size_t)p * 8);
      float4* o1 = (float4*)(out1 + (size_t)p * 8);
      o0[0] = z; o0[1] = z; o1[0] = z; o1[1] = z;
      tgt0[p] = 0; tgt1[p] = 0;
    }
    if (blk == 0 && tid == 0) atomicAdd(a.bad, 1);
    return;
  }
  const RpRow j = rp_row(a, pr);
  s_c[tid] = (double)tid / 255.0;
  const int ma = rp_mean(a, j, 2 * pr, s_red);
  const int mb = rp_mean(a, j, 2 * pr + 1, s_red);
  __syncthreads();
  const uint8_t* fa = a.frames + (size_t)sa * npix * 3;
  const uint8_t* fb = a.frames + (size_t)sb * npix * 3;
  for (int p = start + tid; p < end; p += 256) {
    const uint8_t* qa = fa + (size_t)p * 3;
    const uint8_t* qb = fb + (size_t)p * 3;
    int ra = qa[0], ga = qa[1], ba = qa[2], rb = qb[0], gb = qb[1], bb = qb[2];
    rp_ops(j, j.n_ops, ma, ra, ga, ba);
    rp_ops(j, j.n_ops, mb, rb, gb, bb);
    float ya, yb, uv0, uv1;                        // Y only: U and V are dropped
    pil_yuv_norm(s_c[ra], s_c[ga], s_c[ba], ya, uv0, uv1);
    pil_yuv_norm(s_c[rb], s_c[gb], s_c[bb], yb, uv0, uv1);
    const int la = pil_label_at(a.labels, a.lab_bytes, (size_t)sa * npix + p), lb = pil_label_at(a.labels, a.lab_bytes, (size_t)sb * npix + p);
    const int y = p / a.W, x = p - y * a.W;
    const int xo = j.hflip ? a.W - 1 - x : x, yo = j.vflip ? a.H - 1 - y : y;
    const size_t o = (size_t)yo * a.W + xo;
    float pa[5], pb[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) { pa[c] = la == c ? 1.f : -1.f; pb[c] = lb == c ? 1.f : -1.f; }
    float4* o0 = (float4*)(out0 + o * 8);
    float4* o1 = (float4*)(out1 + o * 8);
    o0[0] = make_float4(ya, yb, ya - yb, pb[0]);
    o0[1] = make_float4(pb[1], pb[2], pb[3], pb[4]);
    o1[0] = make_float4(yb, ya, yb - ya, pa[0]);
    o1[1] = make_float4(pa[1], pa[2], pa[3], pa[4]);
    tgt0[o] = (int64_t)la;
    tgt1[o] = (int64_t)lb;
  }
}

int rcv_launch_lp_pair_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], Hs = op->i[RCV_I_H], Ws = op->i[RCV_I_W], H = op->i[RCV_I_HO], W = op->i[RCV_I_WO];
  const int nClass = op->i[RCV_I_COUT], nsrc = op->i[RCV_I_STRIDE], lab_bytes = op->i[RCV_I_INMODE2], idx_bytes = op->i[RCV_I_INMODE];
  const int train = op->i[RCV_I_AUX0], stats = op->i[RCV_I_COUNT];
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), "lp_pair_prep");
  }
  RCV_CHECK_ARG(nClass == 5, "lp pair prep: %d classes unsupported (the network's first conv reads 3 + 5 channels)", nClass);
  RCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "lp pair prep: B %d, store %d x %d, output %d x %d: every size must be >= 1", B, Hs,
                Ws, H, W);
  RCV_CHECK_ARG(nsrc >= 1, "lp pair prep: a store of %d images (i[STRIDE]): there must be at least 1", nsrc);
  RCV_CHECK_ARG(H == Hs && W == Ws,
                "lp pair prep: a store of %d x %d frames for a network input of %d x %d: only the no-resize form is built; build the store at the "
                "network's size (ResidentDataset(..., img_size=(%d, %d)))", Hs, Ws, H, W, H, W);
  RCV_CHECK_ARG(lab_bytes == 1 || lab_bytes == 4, "lp pair prep: label element size %d unsupported (1 = uint8, 4 = int32)", lab_bytes);
  RCV_CHECK_ARG(idx_bytes == 4 || idx_bytes == 8, "lp pair prep: index element size %d unsupported (4 = int32, 8 = int64)", idx_bytes);
  RCV_CHECK_ARG((train == 0 || train == 1) && (stats == 0 || stats == 1), "lp pair prep: train %d / statistics %d out of range", train, stats);
  RCV_CHECK_ARG((double)nsrc * H * W < 2147483647.0 && (double)B * 2.0 * H * W * 8.0 < 2147483647.0,
                "lp pair prep: a store of %d images, %d pairs of %d x %d: more than 2^31 pixels (or output floats)", nsrc, B, H, W);
  RCV_CHECK_ARG(op->p[RCV_P_IN_AUX] && op->p[RCV_P_EPI_AUX], "lp pair prep: null index or null bad-index counter");
  const int wpi = ceil_div(H * W, PIL_IDENT_PIX), bpp = ceil_div(H * W, RP_PAIR_PIX);
  RCV_CHECK_ARG((double)B * 2.0 * wpi < 2147483647.0 && (double)B * bpp < 2147483647.0, "lp pair prep: grid too large");
  const bool two = train && stats;
  const int n_part = two ? 2 * B * wpi : 0;
  if (query) {
    query->n_part = n_part;
    query->part_bytes = (size_t)n_part * sizeof(uint32_t);
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT] && op->p[RCV_P_X0], "lp pair prep: null operand");
  RCV_CHECK_ARG(((uintptr_t)op->p[RCV_P_OUT] & 15) == 0, "lp pair prep: inputs must be 16-byte aligned");
  RCV_CHECK_ARG(!train || op->p[RCV_P_IN_C], "lp pair prep: training mode needs the parameter rows float[B][%d]", RP_NPAR);
  RCV_CHECK_ARG(!two || (op->p[RCV_P_PART] && ((uintptr_t)op->p[RCV_P_PART] & 3) == 0 && op->i[RCV_I_NPART] == n_part),
                "lp pair prep: workspace missing, unaligned or of %d partial sums where %d are needed (rcv_op_workspace)", op->i[RCV_I_NPART], n_part);
  RpArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = (const uint8_t*)op->p[RCV_P_IN]; a.labels = op->p[RCV_P_IN2];
  a.imgs = (float*)op->p[RCV_P_OUT]; a.tgt = (int64_t*)op->p[RCV_P_X0];
  a.params = train ? (const float*)op->p[RCV_P_IN_C] : nullptr; a.part = two ? (uint32_t*)op->p[RCV_P_PART] : nullptr;
  a.B = 2 * B; a.Hs = H; a.Ws = W; a.H = H; a.W = W; a.kx = 3; a.ky = 3; a.lab_bytes = lab_bytes; a.train = train;
  a.stats = two ? 1 : 0; a.wpi = wpi;
  a.nsrc = nsrc; a.index = op->p[RCV_P_IN_AUX]; a.idx_bytes = idx_bytes; a.bad = (int*)op->p[RCV_P_EPI_AUX];
  if (two) hipLaunchKernelGGL((rgb_prep_ident_kernel<true, RP_PAIR>), dim3(2 * B * wpi), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lp_pair_prep_kernel, dim3(B * bpp), dim3(256), 0, s, a, bpp);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
