// Internal declarations shared by the librcv translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <unordered_map>
#include "../../include/rcv.h"

// Experiment knobs (tile overrides, kernel-family switches) exist only in diagnostic builds (make EXPERIMENTS=1): the shipped
// library never reads the environment on its launch path.
#ifdef RCV_EXPERIMENTS
#define RCV_ENV(name) getenv(name)
#else
#define RCV_ENV(name) ((const char*)nullptr)
#endif

#define RCV_MAX_DEVICES 64

// Tiling plans are a pure function of the integer slots of an op record: computed once per distinct record and kept in the handle
// (a 160x120 step enqueues ~150 kernels; re-planning each of them every step was a measurable share of the host time).
struct rcv_plan_cache {
  std::mutex mu;
  std::unordered_map<std::string, std::string> map;   // key: kind + i[] (workspace slots zeroed); value: the plan struct, bytewise
};

struct rcv_handle {
  int device;    // -1: planning-only handle (rcv_create_planner): workspace / label queries work, nothing can be enqueued
  int num_cus;
  int max_lds;   // bytes of LDS one workgroup may use
  rcv_plan_cache* plans;
  size_t stream_min_bytes;   // streaming-hint threshold (rcv_stream_once); 0: every hint off.  Set once, when the handle is created
  // RCV_F_SIDE_STREAM: ops off the critical path (filter gradients) run on this stream, forked from / joined to the caller's
  // stream with events inside rcv_run; created on first use
  hipStream_t side_stream;
  hipEvent_t ev_fork[8];
  hipEvent_t ev_join;
  int ev_next;
};

void rcv_set_error(const char* fmt, ...);

#define RCV_CHECK_ARG(cond, ...)                         \
  do {                                                   \
    if (!(cond)) {                                       \
      rcv_set_error(__VA_ARGS__);                        \
      return RCV_E_ARG;                                  \
    }                                                    \
  } while (0)

#define RCV_HIP(call)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      rcv_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return RCV_E_HIP;                                                                \
    }                                                                                  \
  } while (0)

// Exact n / d for 0 <= n < 65536, 1 <= d < 65536 (m = floor(2^32/d)+1; d == 1 handled apart).
struct FastDiv {
  uint32_t m, d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.m = (d <= 1) ? 0u : (uint32_t)((0x100000000ull / d) + 1ull);
  return f;
}
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t fd_div(uint32_t n, FastDiv f) {
  return f.d == 1 ? n : __umulhi(n, f.m);
}
// XCD-aware work mapping (MI355X: 8 XCDs, private 4 MiB L2 each; workgroups are dealt round-robin, so ids b and
// b+8 share an L2).  Maps dispatch id b to a logical id such that every XCD owns one CONTIGUOUS range of logical
// ids: workgroups that share operands (parity phases / channel tiles of one pixel tile, halo neighbours) then hit in
// the same L2.  Bijective for any n (cdna guide T1).  Affects speed only.
__device__ __forceinline__ int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7;
  const int xcd = b & 7, i = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}
#endif

// ---- streaming hints, host half (device half and the reasoning: stream_hint.h) ----
// Default threshold.  The Infinity Cache holds 256 MiB, and a line survives only while everything touched between two uses fits in it.
// The kernel that writes a tensor of 128 MiB reads at least as many bytes again, and so does its consumer before it comes back to a
// given line: 128 MiB + the producer's and the consumer's other traffic exceeds 256 MiB, so nothing of such a tensor is still cached
// when it is asked for, and caching it only evicts what is re-read (halos, filters, partial rows).
#define RCV_STREAM_MIN_MB_DEFAULT 128.0
// MiB (may be fractional) -> the handle's threshold in bytes: 0 switches every hint off (the A/B lever); anything positive is at least
// one byte.  The library itself reads no environment (tests/test_lib_abi.py): the binding hands RCV_STREAM_MIN_MB over ONCE per handle,
// when it creates it (rcv_set_stream_min_mb; _lib.py).
static inline size_t rcv_stream_min_bytes(double mb) {
  if (!(mb > 0.0)) return 0;
  const double b = mb * 1048576.0;
  return b < 1.0 ? (size_t)1 : (b > 1e18 ? (size_t)1e18 : (size_t)b);
}
// true when a tensor of `bytes` is too large to be found in cache by whoever touches it next
static inline bool rcv_stream_once(const rcv_handle* h, size_t bytes) { return h->stream_min_bytes != 0 && bytes >= h->stream_min_bytes; }
// The hints of one record (RCV_F_STREAM_OUT | RCV_F_STREAM_PW), from its own N*H*W*C: the output tensor of a conv / transposed conv /
// combine record, the pointwise operand of a filter-gradient record.  The record's own flag bits force a hint whatever the size.
// Kinds without hinted kernels answer 0.  Whether a family honours a hint is the family's business (DESIGN 4.1 has the table).
static inline uint32_t rcv_stream_hints(const rcv_handle* h, const rcv_op* op) {
  uint32_t f = op->flags & (RCV_F_STREAM_OUT | RCV_F_STREAM_PW);
  const size_t n = (size_t)(op->i[RCV_I_N] > 0 ? op->i[RCV_I_N] : 0);
  const size_t c_out = (size_t)(op->i[RCV_I_COUT] > 0 ? op->i[RCV_I_COUT] : 0);
  switch (op->kind) {
    case RCV_OP_CONV:
    case RCV_OP_TCONV:
      if (rcv_stream_once(h, n * op->i[RCV_I_HO] * op->i[RCV_I_WO] * c_out * sizeof(float))) f |= RCV_F_STREAM_OUT;
      break;
    case RCV_OP_COMBINE:      // out: [N][H][W][C], twice the channels with RCV_F_CONCAT; the two inputs have the size of a plain output
      if (rcv_stream_once(h, n * op->i[RCV_I_H] * op->i[RCV_I_W] * c_out * sizeof(float) * ((op->flags & RCV_F_CONCAT) ? 2 : 1))) f |= RCV_F_STREAM_OUT;
      if (rcv_stream_once(h, n * op->i[RCV_I_H] * op->i[RCV_I_W] * c_out * sizeof(float))) f |= RCV_F_STREAM_PW;
      break;
    case RCV_OP_WGRAD:        // pointwise operand: [N][Hp][Wp][CB]
      if (rcv_stream_once(h, n * op->i[RCV_I_HO] * op->i[RCV_I_WO] * c_out * sizeof(float))) f |= RCV_F_STREAM_PW;
      break;
    default:
      f = 0;
      break;
  }
  return f;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

static inline std::string rcv_plan_key(const rcv_op* op) {
  int32_t k[1 + RCV_I__N];
  k[0] = op->kind | (int32_t)((op->flags & RCV_F_RESID) << 16) | (int32_t)((op->flags & RCV_F_MFMA_FP32) << 4);   // the flags a planner looks at
  memcpy(k + 1, op->i, sizeof(op->i));
  k[1 + RCV_I_NPART] = 0; k[1 + RCV_I_NSPLIT] = 0;    // outputs of the planning, not inputs
  return std::string(reinterpret_cast<const char*>(k), sizeof(k));
}
template <typename P>
static inline bool rcv_plan_get(const rcv_handle* h, const rcv_op* op, P* out) {
  if (!h->plans) return false;
  std::lock_guard<std::mutex> g(h->plans->mu);
  auto it = h->plans->map.find(rcv_plan_key(op));
  if (it == h->plans->map.end() || it->second.size() != sizeof(P)) return false;
  memcpy(out, it->second.data(), sizeof(P));
  return true;
}
template <typename P>
static inline void rcv_plan_put(const rcv_handle* h, const rcv_op* op, const P& pl) {
  if (!h->plans) return;
  std::lock_guard<std::mutex> g(h->plans->mu);
  h->plans->map[rcv_plan_key(op)] = std::string(reinterpret_cast<const char*>(&pl), sizeof(P));
}

// Raises the dynamic-LDS limit of one kernel on one device once (hipFuncSetAttribute is per device); `table` is a static
// size_t[RCV_MAX_DEVICES] next to the kernel's launch site.
#define RCV_ENSURE_LDS(kern, lds, dev, table)                                                                          \
  do {                                                                                                                 \
    const int d_ = ((dev) >= 0 && (dev) < RCV_MAX_DEVICES) ? (dev) : 0;                                                \
    if ((lds) > (table)[d_]) {                                                                                         \
      RCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds))); \
      (table)[d_] = (lds);                                                                                             \
    }                                                                                                                  \
  } while (0)

#if defined(__HIPCC__)
// Launches a 512-thread (4 producer + 4 consumer waves) kernel with `lds` bytes of dynamic LDS, raising its limit first where needed.
// KERN is a template argument: every kernel instantiation has its own table.
template <auto KERN, typename Args>
static int rcv_launch_with_lds(const Args& a, dim3 grid, size_t lds, int dev, hipStream_t s) {
  static size_t configured[RCV_MAX_DEVICES];
  RCV_ENSURE_LDS(KERN, lds, dev, configured);
  hipLaunchKernelGGL(KERN, grid, dim3(512), lds, s, a);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
#endif

// A row of a kernel-family table (conv_common.h, wgrad_common.h): host data; the device pass must not see it (it would emit it, host function names and all)
#ifdef __HIP_DEVICE_COMPILE__
#define RCV_HOST_ROW(type, name, ...)
#else
#define RCV_HOST_ROW(type, name, ...) extern const type name = {__VA_ARGS__}
#endif

// ---- launchers implemented in the .hip files; each validates, picks a tiling and enqueues ----
// `query` != nullptr: do not launch, only fill tiling dependent outputs (n_part / n_split / bytes).
struct OpQuery {
  int n_part;
  int n_split;
  size_t part_bytes;
  char label[64];
};
int rcv_launch_conv(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_wgrad(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_filter_layout(const rcv_handle* h, const rcv_op* op, int force);     // rcv_op_filter_layout (conv_dispatch.hip)
int rcv_launch_conv5(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);     // the 5x5 classifier family (conv5.hip)
int rcv_launch_pw(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);        // the pointwise family and the cross filters (conv_pw.hip)
int rcv_launch_small(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_pool_cls(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_objdet(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_lp_batch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_lp_tail(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_lp_input(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_batch_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_rgb_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_lp_pair_prep(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_cls_label(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_cls_valid(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);      // cls_valid.hip
int rcv_launch_cls_proba(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);      // cls_proba.hip
int rcv_launch_cls_calib(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);      // cls_calib.hip
int rcv_launch_valid_fold(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_bnn(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_prune(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_objects(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_flow(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_object_patches(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);
int rcv_launch_map_filter(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query);      // map_filter.hip
// small_kernels.hip: ce_finalize_kernel / rows_reduce_kernel for the translation units that share them
int rcv_enqueue_ce_finalize(const float* part, int n_part, float* loss_out, hipStream_t s);
int rcv_enqueue_rows_reduce(const float* part, int n_rows, int width, float* out0, int n0, float* out1, hipStream_t s);
