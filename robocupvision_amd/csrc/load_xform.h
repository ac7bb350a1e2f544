// The operand transform of the convolution and filter-gradient kernels (RCV_LOAD_* in rcv.h): applied to every tile element on its way
// from global memory to LDS.  It is the numerical contract between the forward and the backward kernels, so it exists once.
#pragma once
#include <type_traits>
#include "rcv_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// x: the operand; a: the second tensor of a two-tensor gradient load (RCV_LOAD_GRAD_*); k: the five constant rows of the channel quad.
template <int MODE>
__device__ __forceinline__ float4 xform4(float4 x, float4 a, const float4 (&k)[5]) {
  float4 v;
  if (MODE == RCV_LOAD_PLAIN || MODE == RCV_LOAD_NCHW) {
    v = x;
  } else if (MODE == RCV_LOAD_AFFINE) {
    v.x = fmaf(x.x, k[0].x, k[1].x); v.y = fmaf(x.y, k[0].y, k[1].y);
    v.z = fmaf(x.z, k[0].z, k[1].z); v.w = fmaf(x.w, k[0].w, k[1].w);
  } else if (MODE == RCV_LOAD_AFFINE_RELU) {
    v.x = fmaxf(fmaf(x.x, k[0].x, k[1].x), 0.f); v.y = fmaxf(fmaf(x.y, k[0].y, k[1].y), 0.f);
    v.z = fmaxf(fmaf(x.z, k[0].z, k[1].z), 0.f); v.w = fmaxf(fmaf(x.w, k[0].w, k[1].w), 0.f);
  } else if (MODE == RCV_LOAD_GRAD_ENC) {
    v.x = a.x > 0.f ? fmaf(k[0].x, x.x, fmaf(k[2].x, a.x, k[1].x)) : 0.f;
    v.y = a.y > 0.f ? fmaf(k[0].y, x.y, fmaf(k[2].y, a.y, k[1].y)) : 0.f;
    v.z = a.z > 0.f ? fmaf(k[0].z, x.z, fmaf(k[2].z, a.z, k[1].z)) : 0.f;
    v.w = a.w > 0.f ? fmaf(k[0].w, x.w, fmaf(k[2].w, a.w, k[1].w)) : 0.f;
  } else {  // RCV_LOAD_GRAD_DEC
    v.x = fmaf(k[0].x, (fmaf(a.x, k[3].x, k[4].x) > 0.f ? x.x : 0.f), fmaf(k[2].x, a.x, k[1].x));
    v.y = fmaf(k[0].y, (fmaf(a.y, k[3].y, k[4].y) > 0.f ? x.y : 0.f), fmaf(k[2].y, a.y, k[1].y));
    v.z = fmaf(k[0].z, (fmaf(a.z, k[3].z, k[4].z) > 0.f ? x.z : 0.f), fmaf(k[2].z, a.z, k[1].z));
    v.w = fmaf(k[0].w, (fmaf(a.w, k[3].w, k[4].w) > 0.f ? x.w : 0.f), fmaf(k[2].w, a.w, k[1].w));
  }
  return v;
}

// the load mode as a runtime value (kernels that do not instantiate their staging per mode)
__device__ __forceinline__ float4 xform_rt(int mode, float4 x, float4 a, const float4 (&k)[5]) {
  switch (mode) {
    case RCV_LOAD_PLAIN: case RCV_LOAD_NCHW: return x;
    case RCV_LOAD_AFFINE: return xform4<RCV_LOAD_AFFINE>(x, a, k);
    case RCV_LOAD_AFFINE_RELU: return xform4<RCV_LOAD_AFFINE_RELU>(x, a, k);
    case RCV_LOAD_GRAD_ENC: return xform4<RCV_LOAD_GRAD_ENC>(x, a, k);
    default: return xform4<RCV_LOAD_GRAD_DEC>(x, a, k);
  }
}

// The load mode of a launch as a compile-time value: calls f(std::integral_constant<int, MODE>).  TWO: the kernel instantiation of the
// two-tensor gradient loads (RCV_LOAD_GRAD_*); the other one serves the single-tensor modes.
template <bool TWO, typename F>
__device__ __forceinline__ void with_load_mode(int mode, F&& f) {
  if (TWO) {
    if (mode == RCV_LOAD_GRAD_ENC) f(std::integral_constant<int, RCV_LOAD_GRAD_ENC>());
    else f(std::integral_constant<int, RCV_LOAD_GRAD_DEC>());
  } else {
    switch (mode) {
      case RCV_LOAD_PLAIN: f(std::integral_constant<int, RCV_LOAD_PLAIN>()); break;
      case RCV_LOAD_AFFINE: f(std::integral_constant<int, RCV_LOAD_AFFINE>()); break;
      default: f(std::integral_constant<int, RCV_LOAD_AFFINE_RELU>()); break;
    }
  }
}
