// fp32 products on the bf16 matrix pipe: the arithmetic shared by conv_bf3.hip, convn_bf3.hip, wgrad_bf3.hip and wgradn_bf3.hip.
//
// gfx950 issues v_mfma_f32_16x16x4_f32 at 1/16 of the bf16 MFMA rate.  An fp32 value splits EXACTLY into three bf16 values,
// x = h + m + l (8 + 8 + 8 significand bits, round-to-nearest at each step, every remainder exact); a product a*b is then the sum of nine
// bf16 x bf16 products, each exact in the fp32 accumulator.  The kernels issue the six largest (hh, hm, mh, hl, lh, mm): what they leave
// out (ml, lm, ll) is below 2^-24 |ab|, the size of ONE fp32 rounding of the product.  Measured against fp64
// (scripts/micro/split_mfma.hip, K = 1152 and 9216, Gaussian and post-ReLU / wide-dynamic-range operands): max and rms error <= those of
// the fp32 MFMA chain in every case; six bf16 MFMAs (v_mfma_f32_16x16x32_bf16) per K = 32 against eight fp32 MFMAs of four times the
// cycles each -- 2.0-2.5 x the fp32 matrix-pipe rate.
//
// Here: the split, the order of the six products, and the transposing LDS read of the kernels whose contraction index is the pixel.  The
// MFMA loops stay in the kernels: how they interleave with the LDS reads is tuned per kernel.
#pragma once
#include "rcv_internal.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(3))) char lds_char;

// x = h + m + l for two values at once; each output word holds the two bf16 of one plane (element 0 in the low half)
struct Bf3Tri { uint32_t h, m, l; };
__device__ __forceinline__ uint32_t bf3_pack(float a, float b) {
  const bf16x2 v = {(__bf16)a, (__bf16)b};            // v_cvt_pk_bf16_f32 (round to nearest even)
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ Bf3Tri bf3_split2(float x0, float x1) {
  Bf3Tri t;
  t.h = bf3_pack(x0, x1);
  const float r0 = x0 - __uint_as_float(t.h << 16), r1 = x1 - __uint_as_float(t.h & 0xffff0000u);       // exact
  t.m = bf3_pack(r0, r1);
  const float s0 = r0 - __uint_as_float(t.m << 16), s1 = r1 - __uint_as_float(t.m & 0xffff0000u);       // exact, <= 8 significant bits
  t.l = bf3_pack(s0, s1);
  return t;
}

// The six products of one multiply-add as (plane of A, plane of B), 0 = h, 1 = m, 2 = l: lh, hl, mm, mh, hm, hh -- smallest products
// first.
constexpr int BF3_TA[6] = {2, 0, 1, 1, 0, 0}, BF3_TB[6] = {0, 2, 1, 0, 1, 0};

// One MFMA operand (eight consecutive k of the lane's row / column) from a [pixel][channel] LDS image whose contraction index is the
// pixel: two transposing reads (ds_read_b64_tr_b16: 4 pixel rows x 16 channels per 16-lane group, each lane gets 4 pixels of its channel).
__device__ __forceinline__ bf16x8 bf3_read_tr(const lds_char* p, int off0, int off1) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + off0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + off1));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
