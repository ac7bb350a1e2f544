// Loads shared by the classifier kernels (small_kernels.hip: logits; cls_label.hip: class maps): the 16-byte accessors and the
// formation of the 1x1 classifier's input, so that every kernel that forms logits rounds them the same way.
#pragma once
#include "stream_hint.h"      // sld4 / sst4 and their streaming forms

#define CLS_MAX_OUT 8
// FUSED: the classifier input up = relu(t*c0+c1) + f(r) (decoder block output + skip, model.py:509) is formed here from the
// block's raw tensors instead of being materialised by RCV_OP_COMBINE (saves one tensor write and one read at full resolution).
// (raw loads and the arithmetic are separate so that the streaming loops can request pixel i+1 before they work on pixel i)
template <int CIN, bool FUSED>
struct ClsRaw { float4 a[CIN / 4]; float4 b[FUSED ? CIN / 4 : 1]; };

// rch: channels per pixel of the skip tensor r (CIN for the decoder's skip add; fewer for LabelProp's `x[:, 0:8] += top`, model.py:565:
// the skip then reaches only the first rch input channels)
template <int CIN, bool FUSED>
__device__ __forceinline__ void cls_load_raw(ClsRaw<CIN, FUSED>& o, const float* __restrict__ x, const float* __restrict__ r, size_t p, int rch = CIN) {
#pragma unroll
  for (int q = 0; q < CIN / 4; ++q) {
    o.a[q] = sld4_nt(x + p * CIN + 4 * q);
    if (FUSED) o.b[FUSED ? q : 0] = 4 * q < rch ? sld4_nt(r + p * rch + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int CIN, bool FUSED>
__device__ __forceinline__ void cls_form_up(float (&v)[CIN], const ClsRaw<CIN, FUSED>& raw, const float* __restrict__ tc,
                                            const float* __restrict__ rc, int mode2, int rch = CIN) {
#pragma unroll
  for (int q = 0; q < CIN / 4; ++q) {
    float4 a = raw.a[q];
    if (FUSED) {
      const float4 s = sld4(tc + 4 * q), h = sld4(tc + CIN + 4 * q);
      a.x = fmaxf(fmaf(a.x, s.x, h.x), 0.f); a.y = fmaxf(fmaf(a.y, s.y, h.y), 0.f);
      a.z = fmaxf(fmaf(a.z, s.z, h.z), 0.f); a.w = fmaxf(fmaf(a.w, s.w, h.w), 0.f);
      float4 b = raw.b[FUSED ? q : 0];
      if (4 * q >= rch) b = make_float4(0.f, 0.f, 0.f, 0.f);                 // input channels the skip does not reach
      else if (mode2 != RCV_LOAD_PLAIN) {
        const float4 s2 = sld4(rc + 4 * q), h2 = sld4(rc + rch + 4 * q);
        b.x = fmaf(b.x, s2.x, h2.x); b.y = fmaf(b.y, s2.y, h2.y); b.z = fmaf(b.z, s2.z, h2.z); b.w = fmaf(b.w, s2.w, h2.w);
        if (mode2 == RCV_LOAD_AFFINE_RELU) { b.x = fmaxf(b.x, 0.f); b.y = fmaxf(b.y, 0.f); b.z = fmaxf(b.z, 0.f); b.w = fmaxf(b.w, 0.f); }
      }
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
  }
}

template <int CIN, bool FUSED>
__device__ __forceinline__ void cls_load_up(float (&v)[CIN], const float* __restrict__ x, const float* __restrict__ tc,
                                            const float* __restrict__ r, const float* __restrict__ rc, int mode2, size_t p, int rch = CIN) {
  ClsRaw<CIN, FUSED> raw;
  cls_load_raw<CIN, FUSED>(raw, x, r, p, rch);
  cls_form_up<CIN, FUSED>(v, raw, tc, rc, mode2, rch);
}
