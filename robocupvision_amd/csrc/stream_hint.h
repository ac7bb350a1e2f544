// Streaming (nontemporal) hints: ONE policy for every kernel family.
//
// A tensor that one kernel writes (or reads) exactly once and that is too large to still be cached when its consumer asks for it gains
// nothing from default-policy accesses, and its lines push out what IS re-read soon: tile halos, packed filters, BatchNorm partial
// rows, labels.  Such accesses are issued as nontemporal.  A hint changes where a line lives, never a bit of a result.
//
// Host half (rcv_internal.h): rcv_stream_once(h, bytes) -- the tensor reaches the handle's threshold (default 128 MiB) -- and
// rcv_stream_hints(h, op), the per-record decision from the record's own N*H*W*C.  It reaches the launch code as the uniform values
// nt_out (final activation / gradient store) and nt_pw (pointwise operands read once per element, no halo).
// RCV_F_STREAM_OUT / RCV_F_STREAM_PW on a record force a hint whatever the size.
//
// Device half (below): the 16-byte accessors, plain and streaming side by side.  The conv kernels take the choice as a template
// parameter (STREAM), picked by nt_out at the launch: behind a run-time branch the epilogues of convs_mfma, convn_bf3 and conv_first
// were rescheduled (+-5 registers, more spills in the 64-virtual-channel tiles); as a parameter the plain instantiation is the
// kernel it was, and the streaming one has the same register counts.  The pointwise kernels (combine, concat) branch on the uniform
// arguments (sst4_hint / sld4_hint): 28..42 registers, nothing to disturb.  Families that honour the hints: DESIGN 4.1.
#pragma once
#include "rcv_internal.h"

__device__ __forceinline__ float4 sld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void sst4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// measured on this part (scripts/micro/stream_bw.hip): a 2-reads-1-write stream gains 4-5 % and a read-only one 8 % over plain accesses
typedef float sv4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 sld4_nt(const float* p) {
  const sv4f v = __builtin_nontemporal_load(reinterpret_cast<const sv4f*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void sst4_nt(float* p, float4 v) {
  sv4f u;
  u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
  __builtin_nontemporal_store(u, reinterpret_cast<sv4f*>(p));
}
// `nt` is wave uniform (a kernel argument): a scalar branch around one of two store / load instructions
__device__ __forceinline__ void sst4_hint(float* p, float4 v, bool nt) {
  if (nt) sst4_nt(p, v);
  else sst4(p, v);
}
__device__ __forceinline__ float4 sld4_hint(const float* p, bool nt) { return nt ? sld4_nt(p) : sld4(p); }
