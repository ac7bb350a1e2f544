// Producer-wave staging of the split-bf16 convolutions (conv_bf3.hip, convn_bf3.hip): CH channels of the input tile, global -> load
// transform -> split -> LDS image [pixel][plane h|m|l][CH] bf16 (6 * CH bytes per pixel).  256 threads, CH / 4 of them per pixel (one
// 16-byte channel quad each), NU passes of 256 / (CH / 4) pixels.  In two steps, so that every load of the tile is in flight before the
// first is consumed.
#pragma once
#include "conv_common.h"
#include "split_bf16.h"

template <int NU, bool TWO>
struct Bf3ConvRegs {
  float4 x[NU], ax[TWO ? NU : 1];
  bool ok[NU];
};

// C: channel stride of the tensor; c0: first staged channel
template <int CH, int NU, bool TWO>
__device__ __forceinline__ void bf3_conv_load(Bf3ConvRegs<NU, TWO>& r, const ConvArgs& a, const TileInfo& ti, int C, int c0, int tid, int npix) {
  constexpr int Q = CH / 4, PP = 256 / Q;
  const int q = tid % Q, lp = tid / Q;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int pix = u * PP + lp;
    const int iy = fd_div(pix, a.fdIW), ix = pix - iy * a.IW;
    const int gy = ti.oy0 + iy, gx = ti.ox0 + ix;
    r.ok[u] = pix < npix && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
    const uint32_t o = r.ok[u] ? (uint32_t)(((ti.n * a.H + gy) * a.W + gx) * C + c0 + 4 * q) : 0u;
    r.x[u] = ld4(a.in + o);
    if (TWO) r.ax[u] = ld4(a.in_aux + o);
  }
}
template <int MODE, int CH, int NU, bool TWO>
__device__ __forceinline__ void bf3_conv_store(const Bf3ConvRegs<NU, TWO>& r, const ConvArgs& a, char* img, int C, int c0, int tid, int npix) {
  constexpr int Q = CH / 4, PP = 256 / Q;
  const int q = tid % Q, lp = tid / Q;
  float4 k[5];
  if (MODE != RCV_LOAD_PLAIN) {
#pragma unroll
    for (int j = 0; j < 5; ++j) k[j] = ld4(a.in_c + (size_t)j * C + c0 + 4 * q);
  }
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int pix = u * PP + lp;
    float4 v = xform4<MODE>(r.x[u], r.ax[TWO ? u : 0], k);
    if (!r.ok[u]) v = make_float4(0.f, 0.f, 0.f, 0.f);          // zero padding AFTER the transform
    if (pix < npix) {
      const Bf3Tri lo = bf3_split2(v.x, v.y), hi = bf3_split2(v.z, v.w);
      char* d = img + pix * (6 * CH) + 8 * q;
      *reinterpret_cast<uint2*>(d) = make_uint2(lo.h, hi.h);
      *reinterpret_cast<uint2*>(d + 2 * CH) = make_uint2(lo.m, hi.m);
      *reinterpret_cast<uint2*>(d + 4 * CH) = make_uint2(lo.l, hi.l);
    }
  }
}

// one tile chunk into `img`, the store instantiated for the launch's load mode (TWO: a two-tensor gradient load)
template <int CH, int NU, bool TWO>
__device__ __forceinline__ void bf3_conv_stage(const ConvArgs& a, const TileInfo& ti, char* img, int C, int c0, int tid, int npix) {
  Bf3ConvRegs<NU, TWO> r;
  bf3_conv_load<CH, NU, TWO>(r, a, ti, C, c0, tid, npix);
  with_load_mode<TWO>(a.in_mode, [&](auto mode) { bf3_conv_store<mode(), CH, NU, TWO>(r, a, img, C, c0, tid, npix); });
}
