// RCV_OP_LP_INPUT: LabelProp's 8-channel input built from a PREDICTION of the previous frame (makeLPImages.py:94-102, the network
// branch of validLabelProp.py:116-135, and the prior that stands commented at labelPropTrain.py:179,250 / validLabelProp.py:118).
//
//   out[s] = [ Ycur[s], Yprev[s], Ycur[s] - Yprev[s], prior_0 .. prior_4 ]      float[B][H][W][8], NHWC: what the first conv reads
//
// Y = channel 0 of a float[B][C][H][W] frame tensor; the difference is one fp32 subtraction.  The prior comes from
//   * a class map, uint8 or int64 [B][H][W]: labelToPred (transform.py:172-183), +1 at the class and -1 elsewhere.  The range is decided
//     on the full 64-bit value: a value outside [0, 5) selects no class (all five channels -1) and is never used as an index;
//   * fp32 logits [B][5][H][W] (NCHW, an eval-mode model(x)): 2 * softmax(z) - 1 with the arithmetic fixed as the contract,
//       m = max_c z_c,  e_c = expf(z_c - m),  S = (((e_0 + e_1) + e_2) + e_3) + e_4,  out_c = 2 * (e_c / S) - 1,
//     expf and an IEEE division, no fast intrinsics.  (2 * q is exact, so whether the compiler contracts 2 * q - 1 into one fused
//     multiply-add or not, the result is the one rounding of the subtraction.)
// Pairing: the stream form reads Ycur[s], Yprev[s] and prior[s] from three operands; the pair form views ONE tensor
// float[B/2][2][C][H][W] as B frames and gives sample s the frames s, s ^ 1 and prior[s ^ 1] (labelPropTrain.py:181-182).
// An optional second output keeps Ycur as a dense float[B][H][W] plane: next frame's Yprev, with no launch of its own.
//
// HBM-bound stream: per pixel 8 bytes of frame + 1 / 8 / 20 bytes of prior in, 32 (+ 4) bytes out.  One thread per pixel, grid-stride,
// 256 threads; consecutive lanes read consecutive pixels of every plane (the five logit planes each coalesced) and write one 32-byte
// pixel each with two 16-byte stores -- the store shape of lp_batch_kernel (csrc/lp_tail.hip).  Every operand holds fewer than 2^31
// elements (checked when planned), so the pixel walk is 32-bit arithmetic.
#include "rcv_internal.h"

#define LPI_CLASSES 5
#define LPI_U8 1
#define LPI_LOGITS 4
#define LPI_I64 8

__device__ __forceinline__ void lpi_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

template <int MODE, bool PAIR>
__global__ __launch_bounds__(256) void lp_input_kernel(const float* __restrict__ cur, const float* __restrict__ prev, const void* __restrict__ prior,
                                                       float* __restrict__ out, float* __restrict__ plane, int B, int C, int Cprev, int HW) {
  const unsigned total = (unsigned)B * (unsigned)HW;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const unsigned s = e / (unsigned)HW, hw = e - s * (unsigned)HW;
    const size_t o = PAIR ? (size_t)(s ^ 1u) : (size_t)s;      // the sample whose frame and prior stand for "previous" (B even when PAIR)
    const float yc = cur[(size_t)s * C * HW + hw];
    const float yp = PAIR ? cur[o * C * HW + hw] : prev[o * Cprev * HW + hw];
    float p[LPI_CLASSES];
    if (MODE == LPI_LOGITS) {
      const float* z = (const float*)prior + o * LPI_CLASSES * HW + hw;
      float v[LPI_CLASSES];
#pragma unroll
      for (int c = 0; c < LPI_CLASSES; ++c) v[c] = z[(size_t)c * HW];
      float m = v[0];
#pragma unroll
      for (int c = 1; c < LPI_CLASSES; ++c) m = fmaxf(m, v[c]);
#pragma unroll
      for (int c = 0; c < LPI_CLASSES; ++c) v[c] = expf(v[c] - m);
      const float S = (((v[0] + v[1]) + v[2]) + v[3]) + v[4];
#pragma unroll
      for (int c = 0; c < LPI_CLASSES; ++c) p[c] = 2.f * __fdiv_rn(v[c], S) - 1.f;
    } else {
      const int64_t l = MODE == LPI_U8 ? (int64_t)((const uint8_t*)prior)[o * HW + hw] : ((const int64_t*)prior)[o * HW + hw];
#pragma unroll
      for (int c = 0; c < LPI_CLASSES; ++c) p[c] = l == (int64_t)c ? 1.f : -1.f;
    }
    float* o8 = out + (size_t)e * 8;
    lpi_st4(o8, make_float4(yc, yp, yc - yp, p[0]));
    lpi_st4(o8 + 4, make_float4(p[1], p[2], p[3], p[4]));
    if (plane) plane[e] = yc;
  }
}

typedef void (*lpi_fn)(const float*, const float*, const void*, float*, float*, int, int, int, int);
static lpi_fn lpi_pick(int mode, bool pair) {
  switch (mode) {
    case LPI_U8: return pair ? lp_input_kernel<LPI_U8, true> : lp_input_kernel<LPI_U8, false>;
    case LPI_I64: return pair ? lp_input_kernel<LPI_I64, true> : lp_input_kernel<LPI_I64, false>;
    case LPI_LOGITS: return pair ? lp_input_kernel<LPI_LOGITS, true> : lp_input_kernel<LPI_LOGITS, false>;
  }
  return nullptr;
}

// Every refusal that depends on the SHAPE of the record sits in front of the `query` return (what rcv_op_workspace / the planner accepts,
// the launch accepts); only operand pointers are checked after it.
int rcv_launch_lp_input(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const int B = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_CIN], nClass = op->i[RCV_I_COUT];
  const int mode = op->i[RCV_I_INMODE], pair = op->i[RCV_I_AUX0], c2 = op->i[RCV_I_AUX1];
  if (query) { query->n_part = 0; query->n_split = 0; query->part_bytes = 0; }
  RCV_CHECK_ARG(nClass == LPI_CLASSES, "labelprop input: %d classes unsupported (the network's first conv reads 3 + 5 channels)", nClass);
  RCV_CHECK_ARG(mode == LPI_U8 || mode == LPI_LOGITS || mode == LPI_I64,
                "labelprop input: prior form %d unsupported (1 = uint8 class map, 8 = int64 class map, 4 = fp32 logits)", mode);
  RCV_CHECK_ARG(pair == 0 || pair == 1, "labelprop input: pairing %d unsupported (0 = stream form, 1 = pair form)", pair);
  RCV_CHECK_ARG(c2 >= 0 && (pair == 0 || c2 == 0 || c2 == C),
                "labelprop input: %d channels in the previous frames unsupported (0 = as the current ones; the pair form has one frame tensor)", c2);
  const int Cprev = c2 ? c2 : C;
  const int widest = C > Cprev ? (C > 8 ? C : 8) : (Cprev > 8 ? Cprev : 8);      // (8 output channels >= the 5 logit planes)
  RCV_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && (double)B * H * W * widest < 2147483647.0,
                "labelprop input: shape %d x %d x %d x %d unsupported (every operand holds fewer than 2^31 elements)", B, C, H, W);
  RCV_CHECK_ARG(!pair || B % 2 == 0, "labelprop input: the pair form takes an even number of frames (got %d)", B);
  if (query) {
    snprintf(query->label, sizeof(query->label), "lp_input<%s,%s>", mode == LPI_U8 ? "u8" : mode == LPI_I64 ? "i64" : "logits",
             pair ? "pair" : "stream");
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && (pair || op->p[RCV_P_IN2]) && op->p[RCV_P_X0] && op->p[RCV_P_OUT], "labelprop input: null operand");
  RCV_CHECK_ARG(((uintptr_t)op->p[RCV_P_OUT] & 15) == 0, "labelprop input: the output must be 16-byte aligned");
  size_t g = ((size_t)B * H * W + 255) / 256;      // the grid of lp_grid(h, pixels, 8) in csrc/lp_tail.hip
  const size_t cap = (size_t)h->num_cus * 8;
  if (g > cap) g = cap;
  hipLaunchKernelGGL(lpi_pick(mode, pair != 0), dim3((unsigned)g), dim3(256), 0, s, (const float*)op->p[RCV_P_IN], (const float*)op->p[RCV_P_IN2],
                     (const void*)op->p[RCV_P_X0], (float*)op->p[RCV_P_OUT], (float*)op->p[RCV_P_X1], B, C, Cprev, H * W);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
