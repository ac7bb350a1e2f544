// RCV_OP_BATCH_PREP (rcv_batch_prep; RCV_OP_FRAME_PREP / rcv_frame_prep is its validation form without labels): the per-image work of the reference's loader, dataset.py:107-133 (SSYUVDataset.__getitem__), with
// ColorJitter (dataset.py:19-39) and the training loop's maskLabel (transform.py:26-49, train.py:43-46), for a whole batch in one launch:
//   uint8 RGB frames [B][Hs][Ws][3] + label planes [B][Hs][Ws] (uint8 / int32)  ->  fp32 NCHW [B][3][H][W] + int64 targets [B][H][W].
// Arithmetic in the reference's order:
//   1. Pillow's 8-bit BILINEAR resize as two integer passes (horizontal, rounded to uint8, then vertical): per output index a first tap,
//      a tap count and 22-bit integer coefficients, all made on the host (robocupvision_amd/data.py); out = clip((sum + 2^21) >> 22).
//      A pass whose two sizes are equal has the one-tap table {i, 1, 2^22}, which returns the byte unchanged (Pillow skips the pass).
//   2. to_tensor + Normalize as a [3][256] fp32 table lookup;  3. mirrored x when flip;  4. y = (y + b) * c;
//   5. u' = m00 u + m01 v, v' = m10 u + m11 v (one fused multiply-add each: within 2^-23 (|m0 u| + |m1 v|) of exact, as the reference's);
//   6. label: gather through the NEAREST index tables, mirror, maskLabel as the reference's sequential rule, widen to int64.
// Nothing random and no trigonometry here: the parameter row {flip, b, c, m00, m01, m10, m11, uv_off} per image comes from the host.
//
// Step 1, its tile (one workgroup = 8 output rows x 64 output columns of one image, lane = output x), the staging of source rows in
// LDS, the label gather, maskLabel and the index test are csrc/pil_resize.h's, shared with csrc/rgb_prep.hip; this file holds what
// follows the resized bytes (steps 2-6, the byte stores) and the launcher.  The vertical pass, the lookup and the jitter read the
// horizontal pass back from LDS, and the three plane stores and the target store are each contiguous over the lanes (reversed when
// flipped).
//
// Two more records run the same passes (the kernels are instantiated per form; nothing is copied):
//   RCV_OP_RESIZE_U8 (rcv_resize_u8) stops after step 1: the three bytes go out as uint8 NHWC [B][H][W][3] and the label is gathered,
//     not masked, and written as uint8 or int32 -- what a device-resident dataset keeps (everything random comes after the bytes);
//   RCV_OP_BATCH_PREP_IDX (rcv_batch_prep_indexed) takes image b from store[index[b]]: the index is read from device memory and tested
//     against [0, N) before it forms an address; an image whose index fails is written as zeros (targets 0) and counted.
#include "pil_resize.h"

enum { BP_PREP = 0, BP_PREP_IDX = 1, BP_BYTES = 2 };          // the form a kernel is instantiated for

struct BpArgs {
  const uint8_t* frames; const void* labels; float* imgs; int64_t* tgt;
  const int32_t* xtab; const int32_t* ytab; const int32_t* lx; const int32_t* ly; const float* norm; const float* params;
  int B, Hs, Ws, H, W, kx, ky, lab_bytes, train, mask, rows_cap, tiles_x, tiles_y;
  int nsrc;                                 // images behind `frames` / `labels`: B, or the N of the store (BP_PREP_IDX)
  const void* index; int idx_bytes; int* bad;          // BP_PREP_IDX: index [B] of 4 / 8 byte elements, counter of the refused ones
  uint8_t* out8; void* lab_out; int lab_out_bytes;     // BP_BYTES: bytes [B][H][W][3], labels [B][H][W] of 1 / 4 byte elements (or null)
};

struct BpJitter { bool flip, uv; float b, c, m00, m01, m10, m11; };

__device__ __forceinline__ BpJitter bp_jitter(const BpArgs& a, int b) {
  BpJitter j;
  j.flip = false; j.uv = false; j.b = 0.f; j.c = 1.f; j.m00 = 1.f; j.m01 = 0.f; j.m10 = 0.f; j.m11 = 1.f;
  if (a.train) {
    const float* p = a.params + (size_t)b * 8;
    j.flip = p[0] != 0.f; j.b = p[1]; j.c = p[2]; j.m00 = p[3]; j.m01 = p[4]; j.m10 = p[5]; j.m11 = p[6]; j.uv = p[7] == 0.f;
  }
  return j;
}

// BP_BYTES: the three resized bytes and the gathered label of one output pixel, as they are
__device__ __forceinline__ void bp_store_bytes(const BpArgs& a, int b, int y, int x, int c0, int c1, int c2) {
  const size_t o = ((size_t)b * a.H + y) * a.W + x;
  uint8_t* q = a.out8 + o * 3;
  q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
  if (!a.lab_out) return;                  // frames without labels (uniform over the launch)
  const int lv = pil_label(a, b, y, x);
  if (a.lab_out_bytes == 1) ((uint8_t*)a.lab_out)[o] = (uint8_t)lv;
  else ((int32_t*)a.lab_out)[o] = lv;
}

// steps 2-6 for one output pixel (x, y: coordinates before the mirror) of batch row b from the three resized bytes of image src
template <typename LUT>
__device__ __forceinline__ void bp_finish(const BpArgs& a, const BpJitter& j, LUT lut, int b, int src, int y, int x, int c0, int c1, int c2) {
  float v0 = lut[c0], v1 = lut[256 + c1], v2 = lut[512 + c2];
  const int xo = j.flip ? a.W - 1 - x : x;
  if (a.train) {
    v0 = (v0 + j.b) * j.c;
    if (j.uv) {
      const float u = v1, v = v2;
      v1 = fmaf(j.m00, u, j.m01 * v);
      v2 = fmaf(j.m10, u, j.m11 * v);
    }
  }
  const size_t plane = (size_t)a.H * a.W, o = (size_t)y * a.W + xo;
  float* img = a.imgs + (size_t)b * 3 * plane + o;
  img[0] = v0; img[plane] = v1; img[2 * plane] = v2;
  if (!a.tgt) return;                      // RCV_OP_FRAME_PREP: frames without labels (uniform over the launch)
  a.tgt[(size_t)b * plane + o] = (int64_t)pil_mask_label(pil_label(a, src, y, x), a.mask);
}

template <bool STAGE, int FORM>
__global__ __launch_bounds__(256) void batch_prep_kernel(BpArgs a) {
  __shared__ float s_lut[FORM == BP_BYTES ? 1 : 768];
  __shared__ int32_t s_xc[PIL_TC * (2 + PIL_MAXK)];
  __shared__ int32_t s_yc[PIL_TR * (2 + PIL_MAXK)];
  __shared__ uint8_t s_h[PIL_ROWS_MAX * PIL_TC * 3];
  __shared__ __align__(16) uint8_t s_src[STAGE ? PIL_RC * PIL_SEG : 16];
  const int tid = threadIdx.x;
  const int bid = blockIdx.x;
  const int tx = bid % a.tiles_x, ty = (bid / a.tiles_x) % a.tiles_y, b = bid / (a.tiles_x * a.tiles_y);
  PilTile t = pil_tile(a, tx, ty);
  int src = b;
  if (FORM == BP_PREP_IDX) {
    src = pil_source(a, (size_t)b);
    if (src < 0) {                          // (the same for the whole workgroup, and in front of every barrier)
      pil_zero_tile(a, b, t);
      if (tx == 0 && ty == 0 && tid == 0) atomicAdd(a.bad, 1);
      return;
    }
  }
  if (FORM != BP_BYTES)                     // (in front of the barrier that closes pil_horizontal's table loads)
    for (int i = tid; i < 768; i += 256) s_lut[i] = a.norm[i];
  BpJitter j = {};
  if (FORM != BP_BYTES) j = bp_jitter(a, b);
  pil_horizontal<STAGE>(a, src, a.nsrc, t, s_xc, s_yc, s_h, s_src);

  // ---- vertical pass + steps 2-6
  const int x = tid & (PIL_TC - 1);
  for (int idx = tid; idx < t.th * PIL_TC; idx += 256) {
    const int yl = idx >> 6;
    if (x >= t.tw) continue;
    int c0, c1, c2;
    pil_vertical(a, t, s_yc, s_h, yl, x, c0, c1, c2);
    if (FORM == BP_BYTES) bp_store_bytes(a, b, t.y0 + yl, t.x0 + x, c0, c1, c2);
    else bp_finish(a, j, s_lut, b, src, t.y0 + yl, t.x0 + x, c0, c1, c2);
  }
}

// H == Hs and W == Ws: no resize (dataset.py:118-121); one thread per pixel, PIL_IDENT_PIX pixels of one image per workgroup
template <int FORM>
__global__ __launch_bounds__(256) void batch_prep_ident_kernel(BpArgs a, int blocks_per_image) {
  const int b = blockIdx.x / blocks_per_image, blk = blockIdx.x % blocks_per_image;
  const int npix = a.H * a.W;
  const int end = min(npix, (blk + 1) * PIL_IDENT_PIX);
  int src = b;
  if (FORM == BP_PREP_IDX) {
    src = pil_source(a, (size_t)b);
    if (src < 0) {
      for (int p = blk * PIL_IDENT_PIX + threadIdx.x; p < end; p += 256) pil_zero(a, b, p / a.W, p % a.W);
      if (blk == 0 && threadIdx.x == 0) atomicAdd(a.bad, 1);
      return;
    }
  }
  const BpJitter j = bp_jitter(a, b);
  const uint8_t* fb = a.frames + (size_t)src * npix * 3;
  for (int p = blk * PIL_IDENT_PIX + threadIdx.x; p < end; p += 256) {
    const int y = p / a.W, x = p - y * a.W;
    const uint8_t* q = fb + (size_t)p * 3;
    bp_finish(a, j, a.norm, b, src, y, x, (int)q[0], (int)q[1], (int)q[2]);
  }
}

// RCV_OP_RESIZE_U8 with H == Hs and W == Ws, labels whose width changes: out[i] = in[i] narrowed (4 -> 1, the low byte) or widened
__global__ __launch_bounds__(256) void resize_u8_label_width_kernel(const void* in, void* out, int in_bytes, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (in_bytes == 4) ((uint8_t*)out)[i] = (uint8_t)((const int32_t*)in)[i];
    else ((int32_t*)out)[i] = (int32_t)((const uint8_t*)in)[i];
  }
}

template <int FORM>
static void bp_launch_tiles(bool stage, const BpArgs& a, hipStream_t s) {
  void (*kern)(BpArgs) = batch_prep_kernel<false, FORM>;
  if (stage) kern = batch_prep_kernel<true, FORM>;
  hipLaunchKernelGGL(kern, dim3(a.B * a.tiles_x * a.tiles_y), dim3(256), 0, s, a);
}

// Every refusal that depends on the shape of the record, and the tables (a plan without them has nothing to read), sits in front of
// the `query` return; the batch operands are checked at launch.
int rcv_launch_batch_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], Hs = op->i[RCV_I_H], Ws = op->i[RCV_I_W], H = op->i[RCV_I_HO], W = op->i[RCV_I_WO];
  // RCV_OP_FRAME_PREP (rcv_frame_prep): the validation form for frames alone -- no label, no label table, no target
  const bool frames_only = op->kind == RCV_OP_FRAME_PREP;
  // RCV_OP_RESIZE_U8 (rcv_resize_u8): the resize alone, bytes out; RCV_OP_BATCH_PREP_IDX (rcv_batch_prep_indexed): images picked from a store
  const bool bytes = op->kind == RCV_OP_RESIZE_U8, indexed = op->kind == RCV_OP_BATCH_PREP_IDX;
  const int kx = op->i[RCV_I_CIN], ky = op->i[RCV_I_COUT], lab_bytes = frames_only ? 1 : op->i[RCV_I_INMODE2];
  const bool no_labels = frames_only || (bytes && lab_bytes == 0);
  const int train = frames_only || bytes ? 0 : op->i[RCV_I_AUX0], mask = frames_only || bytes ? 0 : op->i[RCV_I_AUX1];
  const int nsrc = indexed ? op->i[RCV_I_COUNT] : B;          // images behind p[IN] / p[IN2]
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), frames_only ? "frame_prep" : bytes ? "resize_u8" : indexed ? "batch_prep_idx" : "batch_prep");
  }
  if (const int e = pil_check_record("batch prep", "COUNT", B, nsrc, Hs, Ws, H, W, kx, ky, indexed, op->i[RCV_I_INMODE], op->p[RCV_P_IN_AUX],
                                     op->p[RCV_P_EPI_AUX]))
    return e;
  RCV_CHECK_ARG(lab_bytes == 1 || lab_bytes == 4 || (bytes && lab_bytes == 0), "batch prep: label element size %d unsupported (1 = uint8, 4 = int32)",
                lab_bytes);
  if (bytes && !no_labels)
    RCV_CHECK_ARG(op->i[RCV_I_INMODE] == 1 || op->i[RCV_I_INMODE] == 4,
                  "resize u8: label element size out %d cannot hold the %d-byte labels (1 = uint8, also the narrowing of int32 planes whose "
                  "values are <= 255; 4 = int32)", op->i[RCV_I_INMODE], lab_bytes);
  RCV_CHECK_ARG((train == 0 || train == 1) && mask >= 0 && mask <= 15, "batch prep: train %d / maskLabel flags %d out of range", train, mask);
  if (no_labels)
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2] && (bytes || op->p[RCV_P_X5]),
                  bytes ? "resize u8: null table (frame taps of x / y)" : "frame prep: null table (frame taps of x / y, normalisation)");
  else
    RCV_CHECK_ARG(op->p[RCV_P_X1] && op->p[RCV_P_X2] && op->p[RCV_P_X3] && op->p[RCV_P_X4] && (bytes || op->p[RCV_P_X5]),
                  bytes ? "resize u8: null table (frame taps of x / y, label index of x / y)"
                        : "batch prep: null table (frame taps of x / y, label index of x / y, normalisation)");
  if (query) return RCV_OK;
  if (no_labels) RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_OUT], bytes ? "resize u8: null operand" : "frame prep: null operand");
  else RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT] && op->p[RCV_P_X0], bytes ? "resize u8: null operand" : "batch prep: null operand");
  RCV_CHECK_ARG(!train || op->p[RCV_P_IN_C], "batch prep: training mode needs the parameter rows float[B][8]");
  BpArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = (const uint8_t*)op->p[RCV_P_IN];
  a.labels = no_labels ? nullptr : op->p[RCV_P_IN2];
  a.xtab = (const int32_t*)op->p[RCV_P_X1]; a.ytab = (const int32_t*)op->p[RCV_P_X2];
  a.lx = no_labels ? nullptr : (const int32_t*)op->p[RCV_P_X3]; a.ly = no_labels ? nullptr : (const int32_t*)op->p[RCV_P_X4];
  if (bytes) {
    a.out8 = (uint8_t*)op->p[RCV_P_OUT]; a.lab_out = no_labels ? nullptr : op->p[RCV_P_X0]; a.lab_out_bytes = op->i[RCV_I_INMODE];
  } else {
    a.imgs = (float*)op->p[RCV_P_OUT]; a.tgt = frames_only ? nullptr : (int64_t*)op->p[RCV_P_X0];
    a.norm = (const float*)op->p[RCV_P_X5]; a.params = frames_only ? nullptr : (const float*)op->p[RCV_P_IN_C];
  }
  if (indexed) { a.index = op->p[RCV_P_IN_AUX]; a.idx_bytes = op->i[RCV_I_INMODE]; a.bad = (int*)op->p[RCV_P_EPI_AUX]; }
  a.B = B; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.kx = kx; a.ky = ky; a.lab_bytes = no_labels ? 1 : lab_bytes; a.train = train; a.mask = mask;
  a.tiles_x = ceil_div(W, PIL_TC); a.tiles_y = ceil_div(H, PIL_TR); a.nsrc = nsrc;
  if (H == Hs && W == Ws && bytes) {          // nothing to resize: copies, and one launch where the label width changes
    const size_t npix = (size_t)B * H * W;
    if (a.out8 != a.frames) RCV_HIP(hipMemcpyAsync(a.out8, a.frames, npix * 3, hipMemcpyDeviceToDevice, s));
    if (a.lab_out && a.lab_out_bytes == lab_bytes) {
      if (a.lab_out != a.labels) RCV_HIP(hipMemcpyAsync(a.lab_out, a.labels, npix * lab_bytes, hipMemcpyDeviceToDevice, s));
    } else if (a.lab_out) {
      const size_t blocks = (npix + 255) / 256;
      hipLaunchKernelGGL(resize_u8_label_width_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, a.labels, a.lab_out, lab_bytes,
                         npix);
      RCV_HIP(hipGetLastError());
    }
    return RCV_OK;
  }
  if (H == Hs && W == Ws) {
    const int bpi = ceil_div(H * W, PIL_IDENT_PIX);
    RCV_CHECK_ARG((double)B * bpi < 2147483647.0, "batch prep: grid too large");
    if (indexed) hipLaunchKernelGGL(batch_prep_ident_kernel<BP_PREP_IDX>, dim3(B * bpi), dim3(256), 0, s, a, bpi);
    else hipLaunchKernelGGL(batch_prep_ident_kernel<BP_PREP>, dim3(B * bpi), dim3(256), 0, s, a, bpi);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  a.rows_cap = pil_rows_cap(Hs, H);
  bool stage = pil_stage(kx);          // RCV_BP_STAGE=0 / 1 overrides it in diagnostic builds
  if (const char* e = RCV_ENV("RCV_BP_STAGE")) stage = e[0] != '0';
  if (bytes) bp_launch_tiles<BP_BYTES>(stage, a, s);
  else if (indexed) bp_launch_tiles<BP_PREP_IDX>(stage, a, s);
  else bp_launch_tiles<BP_PREP>(stage, a, s);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
