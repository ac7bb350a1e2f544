// C ABI of librcv.so (declared in include/rcv.h): handle, error text, op dispatch and the named
// convenience entry points.  Nothing here allocates device memory or synchronises the device.
#include <stdarg.h>
#include <string.h>
#include "rcv_internal.h"

static thread_local char g_err[512] = "";

void rcv_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// Every entry point that creates streams / events or launches kernels makes the handle's device current for the duration of the
// call and restores the caller's device afterwards (a process that drives cuda:1 while cuda:0 is current would otherwise get its
// side stream, its events and its kernel launches on the wrong GPU).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = err == hipSuccess;
    }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define RCV_GUARD(h, what)                                                                                            \
  RCV_CHECK_ARG((h)->device >= 0, what ": this is a planning-only handle (rcv_create_planner); it cannot enqueue work"); \
  DeviceGuard guard_((h)->device);                                                                                    \
  if (guard_.err != hipSuccess) { rcv_set_error(what ": cannot make device %d current: %s", (h)->device, hipGetErrorString(guard_.err)); return RCV_E_HIP; }

extern "C" {

const char* rcv_last_error(void) { return g_err; }
int rcv_version(void) { return RCV_VERSION; }

int rcv_create(int device, rcv_handle** out) {
  RCV_CHECK_ARG(out != nullptr, "rcv_create: out is NULL");
  int count = 0;
  RCV_HIP(hipGetDeviceCount(&count));
  RCV_CHECK_ARG(device >= 0 && device < count, "rcv_create: device %d out of range (%d visible)", device, count);
  hipDeviceProp_t prop;
  RCV_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    rcv_set_error("rcv_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return RCV_E_UNSUPPORTED;
  }
  rcv_handle* h = new rcv_handle;
  h->device = device;
  h->num_cus = prop.multiProcessorCount;
  h->max_lds = 160 * 1024;
  h->plans = new rcv_plan_cache;
  h->stream_min_bytes = rcv_stream_min_bytes(RCV_STREAM_MIN_MB_DEFAULT);
  h->side_stream = nullptr;
  h->ev_join = nullptr;
  h->ev_next = 0;
  for (auto& e : h->ev_fork) e = nullptr;
  *out = h;
  return RCV_OK;
}

int rcv_create_planner(int num_cus, rcv_handle** out) {
  RCV_CHECK_ARG(out != nullptr, "rcv_create_planner: out is NULL");
  RCV_CHECK_ARG(num_cus > 0 && num_cus <= 4096, "rcv_create_planner: num_cus %d out of range", num_cus);
  rcv_handle* h = new rcv_handle;
  h->device = -1;
  h->num_cus = num_cus;
  h->max_lds = 160 * 1024;
  h->plans = new rcv_plan_cache;
  h->stream_min_bytes = rcv_stream_min_bytes(RCV_STREAM_MIN_MB_DEFAULT);
  h->side_stream = nullptr;
  h->ev_join = nullptr;
  h->ev_next = 0;
  for (auto& e : h->ev_fork) e = nullptr;
  *out = h;
  return RCV_OK;
}

int rcv_destroy(rcv_handle* h) {
  if (h && h->side_stream) {
    DeviceGuard guard(h->device);
    (void)hipStreamDestroy(h->side_stream);
    (void)hipEventDestroy(h->ev_join);
    for (auto& e : h->ev_fork) (void)hipEventDestroy(e);
  }
  if (h) delete h->plans;
  delete h;
  return RCV_OK;
}

int rcv_num_cus(const rcv_handle* h) { return h ? h->num_cus : 0; }

static int dispatch(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* q) {
  switch (op->kind) {
    case RCV_OP_CONV:
    case RCV_OP_TCONV:
      return rcv_launch_conv(h, op, s, q);
    case RCV_OP_WGRAD:
    case RCV_OP_WGRAD_REDUCE:
    case RCV_OP_WGRAD_REDUCE_BATCH:
      return rcv_launch_wgrad(h, op, s, q);
    case RCV_OP_CONV5:
    case RCV_OP_WGRAD5:
    case RCV_OP_WGRAD5_REDUCE:
    case RCV_OP_PACK5:
      return rcv_launch_conv5(h, op, s, q);
    case RCV_OP_PW:
    case RCV_OP_PW_WGRAD:
    case RCV_OP_PW_WGRAD_REDUCE:
    case RCV_OP_CROSS_PACK:
    case RCV_OP_CROSS_GRAD:
      return rcv_launch_pw(h, op, s, q);
    case RCV_OP_POOL_CLS_FWD:
    case RCV_OP_POOL_CLS_BWD:
      return rcv_launch_pool_cls(h, op, s, q);
    case RCV_OP_OBJECT_MATCH:
      return rcv_launch_objdet(h, op, s, q);
    case RCV_OP_LP_TAIL_FWD:
    case RCV_OP_LP_TAIL_BWD:
      return rcv_launch_lp_tail(h, op, s, q);
    case RCV_OP_LP_BATCH:
      return rcv_launch_lp_batch(h, op, s, q);
    case RCV_OP_LP_INPUT:
      return rcv_launch_lp_input(h, op, s, q);
    case RCV_OP_BATCH_PREP:
    case RCV_OP_FRAME_PREP:
    case RCV_OP_RESIZE_U8:
    case RCV_OP_BATCH_PREP_IDX:
      return rcv_launch_batch_prep(h, op, s, q);
    case RCV_OP_RGB_PREP:
    case RCV_OP_RGB_PREP_IDX:
      return rcv_launch_rgb_prep(h, op, s, q);
    case RCV_OP_LP_PAIR_PREP:
      return rcv_launch_lp_pair_prep(h, op, s, q);
    case RCV_OP_CLS_LABEL:
      return rcv_launch_cls_label(h, op, s, q);
    case RCV_OP_CLS_VALID:
      return rcv_launch_cls_valid(h, op, s, q);
    case RCV_OP_CLS_PROBA:
      return rcv_launch_cls_proba(h, op, s, q);
    case RCV_OP_CLS_CALIB:
      return rcv_launch_cls_calib(h, op, s, q);
    case RCV_OP_VALID_FOLD:
      return rcv_launch_valid_fold(h, op, s, q);
    case RCV_OP_BNN_STAGE_FWD:
    case RCV_OP_BNN_STAGE_BWD:
    case RCV_OP_BNN_HEAD_FWD:
    case RCV_OP_BNN_HEAD_BWD:
      return rcv_launch_bnn(h, op, s, q);
    case RCV_OP_PRUNE:
      return rcv_launch_prune(h, op, s, q);
    case RCV_OP_OBJECTS:
      return rcv_launch_objects(h, op, s, q);
    case RCV_OP_FARNEBACK:
    case RCV_OP_REMAP_LABELS:
      return rcv_launch_flow(h, op, s, q);
    case RCV_OP_OBJECT_PATCHES:
      return rcv_launch_object_patches(h, op, s, q);
    case RCV_OP_MAP_FILTER:
      return rcv_launch_map_filter(h, op, s, q);
    case RCV_OP_NOP:
      if (q) { snprintf(q->label, sizeof(q->label), "nop"); q->n_part = 0; q->n_split = 0; q->part_bytes = 0; }
      return RCV_OK;
    default:
      return rcv_launch_small(h, op, s, q);
  }
}

int rcv_op_workspace(const rcv_handle* h, rcv_op* op, size_t* part_bytes) {
  RCV_CHECK_ARG(h && op && part_bytes, "rcv_op_workspace: NULL argument");
  OpQuery q;
  memset(&q, 0, sizeof(q));
  const int rc = dispatch(h, op, nullptr, &q);
  if (rc) return rc;
  op->i[RCV_I_NPART] = q.n_part;
  if (op->kind == RCV_OP_WGRAD || op->kind == RCV_OP_WGRAD5 || op->kind == RCV_OP_PW_WGRAD) op->i[RCV_I_NSPLIT] = q.n_split;
  *part_bytes = q.part_bytes;
  return RCV_OK;
}

static int run_ops(rcv_handle* h, const rcv_op* ops, int n, void* stream, bool join);

int rcv_run(rcv_handle* h, const rcv_op* ops, int n, void* stream) { return run_ops(h, ops, n, stream, true); }

int rcv_run_ex(rcv_handle* h, const rcv_op* ops, int n, void* stream, uint32_t run_flags) {
  return run_ops(h, ops, n, stream, !(run_flags & RCV_RUN_NO_JOIN));
}

int rcv_join_side(rcv_handle* h, void* stream) {
  RCV_CHECK_ARG(h, "rcv_join_side: NULL handle");
  if (!h->side_stream) return RCV_OK;         // nothing was ever forked
  RCV_GUARD(h, "rcv_join_side");
  RCV_HIP(hipEventRecord(h->ev_join, h->side_stream));
  RCV_HIP(hipStreamWaitEvent((hipStream_t)stream, h->ev_join, 0));
  return RCV_OK;
}

}  // extern "C"

static int run_ops(rcv_handle* h, const rcv_op* ops, int n, void* stream, bool join) {
  RCV_CHECK_ARG(h && (ops || n == 0) && n >= 0, "rcv_run: bad arguments");
  RCV_GUARD(h, "rcv_run");
  hipStream_t s = (hipStream_t)stream;
  // Ops flagged RCV_F_SIDE_STREAM run on the handle's side stream: it is forked from `stream` in front of every run of such ops
  // (event record on `stream`, wait on the side stream) and joined back before rcv_run returns, so the caller keeps seeing ONE
  // stream-ordered call.  No host synchronisation; capturable (the side stream joins the capture through the events).
  bool prev_side = false, side_used = false;
  for (int k = 0; k < n; ++k) {
    if (ops[k].kind == RCV_OP_NOP) continue;    // (does not end a run of side-stream ops either: no extra fork around an empty slot)
    const bool side = (ops[k].flags & RCV_F_SIDE_STREAM) != 0;
    if (side && !h->side_stream) {
      RCV_HIP(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
      RCV_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
      for (auto& e : h->ev_fork) RCV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (side && !prev_side) {
      hipEvent_t e = h->ev_fork[h->ev_next];
      h->ev_next = (h->ev_next + 1) % 8;
      RCV_HIP(hipEventRecord(e, s));
      RCV_HIP(hipStreamWaitEvent(h->side_stream, e, 0));
      side_used = true;
    }
    prev_side = side;
    const int rc = dispatch(h, &ops[k], side ? h->side_stream : s, nullptr);
    if (rc) {
      char tmp[400];
      strncpy(tmp, g_err, sizeof(tmp) - 1);
      tmp[sizeof(tmp) - 1] = 0;
      rcv_set_error("op %d (kind %d): %s", k, ops[k].kind, tmp);
      if (side_used) { (void)hipEventRecord(h->ev_join, h->side_stream); (void)hipStreamWaitEvent(s, h->ev_join, 0); }
      return rc;
    }
  }
  if (side_used && join) {
    RCV_HIP(hipEventRecord(h->ev_join, h->side_stream));
    RCV_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
  }
  return RCV_OK;
}

extern "C" {

int rcv_op_filter_layout(const rcv_handle* h, const rcv_op* op, int force) { return h && op ? rcv_filter_layout(h, op, force) : 0; }

int rcv_set_stream_min_mb(rcv_handle* h, double mb) {
  RCV_CHECK_ARG(h && mb >= 0.0, "rcv_set_stream_min_mb: NULL handle or negative threshold");
  h->stream_min_bytes = rcv_stream_min_bytes(mb);
  return RCV_OK;
}

int rcv_op_stream_hints(const rcv_handle* h, const rcv_op* op) {
  RCV_CHECK_ARG(h && op, "rcv_op_stream_hints: bad arguments");
  OpQuery q;
  memset(&q, 0, sizeof(q));
  const int rc = dispatch(h, op, nullptr, &q);      // refuses what a launch would refuse
  if (rc) return rc;
  return (int)rcv_stream_hints(h, op);
}

int rcv_op_kernel_label(const rcv_handle* h, const rcv_op* op, char* buf, int size) {
  RCV_CHECK_ARG(h && op && buf && size > 0, "rcv_op_kernel_label: bad arguments");
  OpQuery q;
  memset(&q, 0, sizeof(q));
  const int rc = dispatch(h, op, nullptr, &q);
  if (rc) return rc;
  strncpy(buf, q.label, size - 1);
  buf[size - 1] = 0;
  return RCV_OK;
}

int rcv_run_timed(rcv_handle* h, const rcv_op* ops, int n, void* stream, float* ms) {
  RCV_CHECK_ARG(h && ops && n > 0 && ms, "rcv_run_timed: bad arguments");
  RCV_GUARD(h, "rcv_run_timed");
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t* ev = new hipEvent_t[n + 1];
  for (int k = 0; k <= n; ++k) {
    if (hipEventCreate(&ev[k]) != hipSuccess) { rcv_set_error("rcv_run_timed: hipEventCreate failed"); delete[] ev; return RCV_E_HIP; }
  }
  int rc = RCV_OK;
  (void)hipEventRecord(ev[0], s);
  int last = 0;                      // index of the event that closes the latest op that launched something
  int* opens = new int[n];           // event that opens op k (RCV_OP_NOP slots launch nothing and take no event: rcv_run skips them too)
  for (int k = 0; k < n && rc == RCV_OK; ++k) {
    opens[k] = last;
    if (ops[k].kind == RCV_OP_NOP) continue;
    rc = dispatch(h, &ops[k], s, nullptr);
    (void)hipEventRecord(ev[k + 1], s);
    last = k + 1;
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == RCV_OK) { rcv_set_error("rcv_run_timed: stream sync failed"); rc = RCV_E_HIP; }
  if (rc == RCV_OK)
    for (int k = 0; k < n; ++k) {
      if (ops[k].kind == RCV_OP_NOP) ms[k] = 0.f;
      else (void)hipEventElapsedTime(&ms[k], ev[opens[k]], ev[k + 1]);
    }
  delete[] opens;
  for (int k = 0; k <= n; ++k) (void)hipEventDestroy(ev[k]);
  delete[] ev;
  return rc;
}

// ------------------------------ named entry points ------------------------------
int rcv_conv3x3(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_CONV, "rcv_conv3x3: record kind must be RCV_OP_CONV");
  return rcv_run(h, op, 1, stream);
}
int rcv_convT3x3s2(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_TCONV, "rcv_convT3x3s2: record kind must be RCV_OP_TCONV");
  return rcv_run(h, op, 1, stream);
}
int rcv_wgrad3x3(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_WGRAD, "rcv_wgrad3x3: record kind must be RCV_OP_WGRAD");
  return rcv_run(h, op, 1, stream);
}

int rcv_conv5x5(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_CONV5, "rcv_conv5x5: record kind must be RCV_OP_CONV5");
  return rcv_run(h, op, 1, stream);
}
int rcv_wgrad5x5(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_WGRAD5, "rcv_wgrad5x5: record kind must be RCV_OP_WGRAD5");
  return rcv_run(h, op, 1, stream);
}
int rcv_conv_pw(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_PW, "rcv_conv_pw: record kind must be RCV_OP_PW");
  return rcv_run(h, op, 1, stream);
}
int rcv_wgrad_pw(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_PW_WGRAD, "rcv_wgrad_pw: record kind must be RCV_OP_PW_WGRAD");
  return rcv_run(h, op, 1, stream);
}

int rcv_bn_finalize(rcv_handle* h, const float* part, int n_part, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, int training, float* consts,
                    float* save_mean, float* save_istd, void* stream) {
  RCV_CHECK_ARG(count == (double)(long long)count && count < 2147483647.0, "rcv_bn_finalize: count must be an integer < 2^31");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_BN_FINALIZE;
  op.flags = training ? RCV_F_TRAINING : 0;
  op.i[RCV_I_N] = (int)count; op.i[RCV_I_HO] = 1; op.i[RCV_I_WO] = 1;
  op.i[RCV_I_COUT] = C; op.i[RCV_I_NPART] = n_part;
  op.f[0] = momentum; op.f[1] = eps;
  op.p[RCV_P_PART] = (void*)part; op.p[RCV_P_OUT] = consts;
  op.p[RCV_P_X0] = (void*)gamma; op.p[RCV_P_X1] = (void*)beta; op.p[RCV_P_X2] = running_mean; op.p[RCV_P_X3] = running_var;
  op.p[RCV_P_X4] = save_mean; op.p[RCV_P_X5] = save_istd;
  return rcv_run(h, &op, 1, stream);
}

int rcv_bn_backward(rcv_handle* h, const float* part, int n_part, int C, double count, const float* gamma, const float* save_mean,
                    const float* save_istd, const float* fwd_consts, int decoder, float* consts, float* dgamma, float* dbeta,
                    void* stream) {
  (void)decoder;
  RCV_CHECK_ARG(count == (double)(long long)count && count < 2147483647.0, "rcv_bn_backward: count must be an integer < 2^31");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_BN_BWD;
  op.i[RCV_I_N] = (int)count; op.i[RCV_I_HO] = 1; op.i[RCV_I_WO] = 1;
  op.i[RCV_I_COUT] = C; op.i[RCV_I_NPART] = n_part;
  op.p[RCV_P_PART] = (void*)part; op.p[RCV_P_OUT] = consts; op.p[RCV_P_IN_C] = (void*)fwd_consts;
  op.p[RCV_P_X0] = (void*)gamma; op.p[RCV_P_X1] = dgamma; op.p[RCV_P_X2] = dbeta;
  op.p[RCV_P_X4] = (void*)save_mean; op.p[RCV_P_X5] = (void*)save_istd;
  return rcv_run(h, &op, 1, stream);
}

int rcv_maxpool2x2_fwd(rcv_handle* h, const float* r, const float* consts, float* out, int N, int H, int W, int C, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_POOL_FWD;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C;
  op.i[RCV_I_INMODE] = consts ? RCV_LOAD_AFFINE : RCV_LOAD_PLAIN;
  op.p[RCV_P_IN] = (void*)r; op.p[RCV_P_IN_C] = (void*)consts; op.p[RCV_P_OUT] = out;
  return rcv_run(h, &op, 1, stream);
}

int rcv_softmax_ce_argmax_fwd(rcv_handle* h, const float* logits, const int64_t* target, const float* class_weight, int N, int C,
                              int H, int W, float* part, int n_part, float* loss_out, uint8_t* argmax, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CE_FWD;
  op.flags = argmax ? RCV_F_ARGMAX : 0;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C; op.i[RCV_I_NPART] = n_part;
  op.p[RCV_P_IN] = (void*)logits; op.p[RCV_P_IN2] = (void*)target; op.p[RCV_P_W] = (void*)class_weight;
  op.p[RCV_P_PART] = part; op.p[RCV_P_OUT] = loss_out; op.p[RCV_P_X0] = argmax;
  return rcv_run(h, &op, 1, stream);
}

int rcv_softmax_ce_bwd(rcv_handle* h, const float* logits, const int64_t* target, const float* class_weight, const float* loss_out,
                       const float* grad_out, int N, int C, int H, int W, float* dlogits, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CE_BWD;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C;
  op.p[RCV_P_IN] = (void*)logits; op.p[RCV_P_IN2] = (void*)target; op.p[RCV_P_W] = (void*)class_weight;
  op.p[RCV_P_X0] = (void*)loss_out; op.p[RCV_P_X1] = (void*)grad_out; op.p[RCV_P_OUT] = dlogits;
  return rcv_run(h, &op, 1, stream);
}

int rcv_dice_fwd(rcv_handle* h, const float* logits, const int64_t* target, const float* class_weight, float eps, int N, int C, int H,
                 int W, float* part, int n_part, float* out, uint8_t* argmax, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_DICE_FWD;
  op.flags = argmax ? RCV_F_ARGMAX : 0;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C; op.i[RCV_I_NPART] = n_part;
  op.f[1] = eps;
  op.p[RCV_P_IN] = (void*)logits; op.p[RCV_P_IN2] = (void*)target; op.p[RCV_P_W] = (void*)class_weight;
  op.p[RCV_P_PART] = part; op.p[RCV_P_OUT] = out; op.p[RCV_P_X0] = argmax;
  return rcv_run(h, &op, 1, stream);
}

int rcv_dice_bwd(rcv_handle* h, const float* logits, const int64_t* target, const float* fwd_out, const float* grad_out, int N, int C,
                 int H, int W, float* dlogits, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_DICE_BWD;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C;
  op.p[RCV_P_IN] = (void*)logits; op.p[RCV_P_IN2] = (void*)target;
  op.p[RCV_P_X0] = (void*)fwd_out; op.p[RCV_P_X1] = (void*)grad_out; op.p[RCV_P_OUT] = dlogits;
  return rcv_run(h, &op, 1, stream);
}

int rcv_confusion(rcv_handle* h, const uint8_t* argmax, const int64_t* target, int N, int C, int H, int W, int32_t* counts, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CONFUSION;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C;
  op.p[RCV_P_IN] = (void*)argmax; op.p[RCV_P_IN2] = (void*)target; op.p[RCV_P_OUT] = counts;
  return rcv_run(h, &op, 1, stream);
}

int rcv_object_match(rcv_handle* h, const void* pred, int pred_bytes, const void* target, int target_bytes, int N, int C, int H, int W,
                     const double* iou_thr, const double* dist_thr, int K, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_OBJECT_MATCH;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C; op.i[RCV_I_COUNT] = K;
  op.i[RCV_I_INMODE] = pred_bytes; op.i[RCV_I_INMODE2] = target_bytes;
  op.p[RCV_P_IN] = (void*)pred; op.p[RCV_P_IN2] = (void*)target; op.p[RCV_P_OUT] = counts; op.p[RCV_P_PART] = ws;
  op.p[RCV_P_X0] = (void*)iou_thr; op.p[RCV_P_X1] = (void*)dist_thr;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(ws_bytes >= need, "rcv_object_match: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", ws_bytes, need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_find_objects(rcv_handle* h, const void* classmap, int elem_bytes, int N, int C, int H, int W, const int32_t* min_area,
                     const double* min_ratio, const int32_t* cap, int M, int32_t* rows, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_OBJECTS;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = C; op.i[RCV_I_COUNT] = M; op.i[RCV_I_INMODE] = elem_bytes;
  op.p[RCV_P_IN] = (void*)classmap; op.p[RCV_P_OUT] = rows; op.p[RCV_P_X0] = counts; op.p[RCV_P_PART] = workspace;
  op.p[RCV_P_X1] = (void*)min_ratio; op.p[RCV_P_X2] = (void*)min_area; op.p[RCV_P_X3] = (void*)cap;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_find_objects: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes,
                need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_object_patches(rcv_handle* h, const uint8_t* frames, int N, int Hs, int Ws, const int32_t* rows, const int32_t* counts, int C,
                       int M, int H, int W, int Sh, int Sw, int margin, float* images, uint8_t* bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_OBJECT_PATCHES;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_COUT] = C - 1;
  op.i[RCV_I_COUNT] = M; op.i[RCV_I_AUX0] = Sh; op.i[RCV_I_AUX1] = Sw; op.i[RCV_I_CIN] = margin;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)rows; op.p[RCV_P_X0] = (void*)counts; op.p[RCV_P_OUT] = images;
  op.p[RCV_P_X1] = bytes;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);      // (no workspace: the record's refusals, on any handle)
  if (rc) return rc;
  return rcv_run(h, &op, 1, stream);
}

int rcv_farneback_flow(rcv_handle* h, const uint8_t* prev, const uint8_t* next, int channels, int B, int H, int W, float pyr_scale,
                       int levels, int winsize, int iterations, int poly_n, float poly_sigma, int flags, float* flow, void* workspace,
                       size_t workspace_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_FARNEBACK;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = channels; op.i[RCV_I_COUNT] = levels; op.i[RCV_I_AUX0] = winsize;
  op.i[RCV_I_AUX1] = iterations; op.i[RCV_I_STRIDE] = poly_n; op.i[RCV_I_DIL] = flags;
  op.f[0] = pyr_scale; op.f[1] = poly_sigma;
  op.p[RCV_P_IN] = (void*)prev; op.p[RCV_P_IN2] = (void*)next; op.p[RCV_P_OUT] = flow; op.p[RCV_P_PART] = workspace;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_farneback_flow: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes,
                need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_update_labels(rcv_handle* h, const void* labels, int elem_bytes, const float* flow, int N, int H, int W, void* out, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_REMAP_LABELS;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_INMODE] = elem_bytes;
  op.p[RCV_P_IN] = (void*)labels; op.p[RCV_P_IN2] = (void*)flow; op.p[RCV_P_OUT] = out;
  return rcv_run(h, &op, 1, stream);
}

int rcv_map_filter(rcv_handle* h, const void* in, const void* original, int elem_bytes, int N, int H, int W, int num_class, int window,
                   int rule, int set, int arg0, int arg1, void* out, int32_t* changed, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_MAP_FILTER;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = num_class; op.i[RCV_I_COUNT] = window;
  op.i[RCV_I_INMODE] = elem_bytes; op.i[RCV_I_INMODE2] = (rule == RCV_MF_OPEN_FINISH || rule == RCV_MF_CLOSE_FINISH) ? 1 : 0;
  op.i[RCV_I_AUX0] = rule; op.i[RCV_I_AUX1] = set; op.i[RCV_I_STRIDE] = arg0; op.i[RCV_I_DIL] = arg1;
  op.p[RCV_P_IN] = (void*)in; op.p[RCV_P_IN2] = (void*)original; op.p[RCV_P_OUT] = out; op.p[RCV_P_X0] = changed;
  return rcv_run(h, &op, 1, stream);
}

int rcv_labelprop_batch(rcv_handle* h, const float* images, const int64_t* labels, int B, int C, int H, int W, int num_class,
                        float* inputs, int64_t* targets, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_LP_BATCH;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = C; op.i[RCV_I_COUT] = num_class;
  op.p[RCV_P_IN] = (void*)images; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = inputs; op.p[RCV_P_X0] = targets;
  return rcv_run(h, &op, 1, stream);
}

int rcv_lp_input(rcv_handle* h, const float* cur, const float* prev, int prev_C, const void* prior, int prior_bytes, int pair, int B, int C,
                 int H, int W, int num_class, float* inputs, float* plane, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_LP_INPUT;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = C; op.i[RCV_I_COUT] = num_class;
  op.i[RCV_I_INMODE] = prior_bytes; op.i[RCV_I_AUX0] = pair; op.i[RCV_I_AUX1] = prev_C;
  op.p[RCV_P_IN] = (void*)cur; op.p[RCV_P_IN2] = (void*)prev; op.p[RCV_P_X0] = (void*)prior; op.p[RCV_P_OUT] = inputs; op.p[RCV_P_X1] = plane;
  return rcv_run(h, &op, 1, stream);
}

int rcv_batch_prep(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int B, int Hs, int Ws, int H, int W,
                   const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y,
                   const float* norm, const float* params, int train, int mask_flags, float* imgs, int64_t* targets, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_BATCH_PREP;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.i[RCV_I_INMODE2] = label_bytes; op.i[RCV_I_AUX0] = train; op.i[RCV_I_AUX1] = mask_flags;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = imgs; op.p[RCV_P_X0] = targets;
  op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y; op.p[RCV_P_X3] = (void*)label_x; op.p[RCV_P_X4] = (void*)label_y;
  op.p[RCV_P_X5] = (void*)norm; op.p[RCV_P_IN_C] = (void*)params;
  return rcv_run(h, &op, 1, stream);
}

int rcv_frame_prep(rcv_handle* h, const uint8_t* frames, int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx,
                   const int32_t* frame_y, int ky, const float* norm, float* imgs, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_FRAME_PREP;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_OUT] = imgs; op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y;
  op.p[RCV_P_X5] = (void*)norm;
  return rcv_run(h, &op, 1, stream);
}

int rcv_resize_u8(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int B, int Hs, int Ws, int H, int W,
                  const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y, uint8_t* out,
                  void* labels_out, int label_out_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_RESIZE_U8;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.i[RCV_I_INMODE2] = labels ? label_bytes : 0; op.i[RCV_I_INMODE] = labels ? label_out_bytes : 1;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = out; op.p[RCV_P_X0] = labels_out;
  op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y; op.p[RCV_P_X3] = (void*)label_x; op.p[RCV_P_X4] = (void*)label_y;
  return rcv_run(h, &op, 1, stream);
}

int rcv_batch_prep_indexed(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int N, const void* index, int index_bytes,
                           int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx, const int32_t* frame_y, int ky,
                           const int32_t* label_x, const int32_t* label_y, const float* norm, const float* params, int train, int mask_flags,
                           float* imgs, int64_t* targets, int32_t* bad_count, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_BATCH_PREP_IDX;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.i[RCV_I_INMODE2] = label_bytes; op.i[RCV_I_AUX0] = train; op.i[RCV_I_AUX1] = mask_flags;
  op.i[RCV_I_COUNT] = N; op.i[RCV_I_INMODE] = index_bytes;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = imgs; op.p[RCV_P_X0] = targets;
  op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y; op.p[RCV_P_X3] = (void*)label_x; op.p[RCV_P_X4] = (void*)label_y;
  op.p[RCV_P_X5] = (void*)norm; op.p[RCV_P_IN_C] = (void*)params; op.p[RCV_P_IN_AUX] = (void*)index; op.p[RCV_P_EPI_AUX] = bad_count;
  return rcv_run(h, &op, 1, stream);
}

int rcv_rgb_prep(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int B, int Hs, int Ws, int H, int W,
                 const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y,
                 const float* params, int train, int stats, int mask_flags, float* imgs, int64_t* targets, void* workspace,
                 size_t workspace_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_RGB_PREP;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.i[RCV_I_INMODE2] = labels ? label_bytes : 0; op.i[RCV_I_AUX0] = train; op.i[RCV_I_AUX1] = mask_flags; op.i[RCV_I_COUNT] = stats;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = imgs; op.p[RCV_P_X0] = targets;
  op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y; op.p[RCV_P_X3] = (void*)label_x; op.p[RCV_P_X4] = (void*)label_y;
  op.p[RCV_P_IN_C] = (void*)params; op.p[RCV_P_PART] = workspace;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_rgb_prep: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes, need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_rgb_prep_indexed(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int N, const void* index, int index_bytes,
                         int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx, const int32_t* frame_y, int ky,
                         const int32_t* label_x, const int32_t* label_y, const float* params, int train, int stats, int mask_flags,
                         float* imgs, int64_t* targets, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_RGB_PREP_IDX;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_CIN] = kx; op.i[RCV_I_COUT] = ky;
  op.i[RCV_I_INMODE2] = labels ? label_bytes : 0; op.i[RCV_I_AUX0] = train; op.i[RCV_I_AUX1] = mask_flags; op.i[RCV_I_COUNT] = stats;
  op.i[RCV_I_STRIDE] = N; op.i[RCV_I_INMODE] = index_bytes;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = imgs; op.p[RCV_P_X0] = targets;
  op.p[RCV_P_X1] = (void*)frame_x; op.p[RCV_P_X2] = (void*)frame_y; op.p[RCV_P_X3] = (void*)label_x; op.p[RCV_P_X4] = (void*)label_y;
  op.p[RCV_P_IN_C] = (void*)params; op.p[RCV_P_PART] = workspace; op.p[RCV_P_IN_AUX] = (void*)index; op.p[RCV_P_EPI_AUX] = bad_count;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_rgb_prep_indexed: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes,
                need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_lp_pair_prep(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int N, const void* pairs, int pair_bytes, int B,
                     int Hs, int Ws, int H, int W, int num_class, const float* params, int train, int stats, float* inputs, int64_t* targets,
                     int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_LP_PAIR_PREP;
  op.i[RCV_I_N] = B; op.i[RCV_I_H] = Hs; op.i[RCV_I_W] = Ws; op.i[RCV_I_HO] = H; op.i[RCV_I_WO] = W; op.i[RCV_I_COUT] = num_class;
  op.i[RCV_I_INMODE2] = label_bytes; op.i[RCV_I_AUX0] = train; op.i[RCV_I_COUNT] = stats; op.i[RCV_I_STRIDE] = N; op.i[RCV_I_INMODE] = pair_bytes;
  op.p[RCV_P_IN] = (void*)frames; op.p[RCV_P_IN2] = (void*)labels; op.p[RCV_P_OUT] = inputs; op.p[RCV_P_X0] = targets;
  op.p[RCV_P_IN_C] = (void*)params; op.p[RCV_P_PART] = workspace; op.p[RCV_P_IN_AUX] = (void*)pairs; op.p[RCV_P_EPI_AUX] = bad_count;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_lp_pair_prep: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes, need);
  return rcv_run(h, &op, 1, stream);
}

int rcv_cls_label(rcv_handle* h, const float* x, const float* w, const float* bias, int N, int H, int W, int CIN, int COUT, uint8_t* labels,
                  uint8_t* colour, const uint8_t* palette, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CLS_LABEL;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = CIN; op.i[RCV_I_COUT] = COUT; op.i[RCV_I_INMODE] = 0;
  op.p[RCV_P_IN] = (void*)x; op.p[RCV_P_W] = (void*)w; op.p[RCV_P_BIAS] = (void*)bias; op.p[RCV_P_OUT] = labels; op.p[RCV_P_X0] = colour;
  op.p[RCV_P_X1] = (void*)palette;
  return rcv_run(h, &op, 1, stream);
}

int rcv_colorize(rcv_handle* h, const void* classmap, int elem_bytes, int N, int H, int W, uint8_t* colour, const uint8_t* palette,
                 void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CLS_LABEL;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = 1; op.i[RCV_I_COUT] = 8; op.i[RCV_I_INMODE] = 2;
  op.i[RCV_I_INMODE2] = elem_bytes;
  op.p[RCV_P_IN] = (void*)classmap; op.p[RCV_P_X0] = colour; op.p[RCV_P_X1] = (void*)palette;
  return rcv_run(h, &op, 1, stream);
}

int rcv_cls_valid(rcv_handle* h, const float* x, const float* w, const float* bias, int N, int H, int W, int CIN, int COUT, const int64_t* targets,
                  const float* class_weights, int32_t* counts, uint8_t* labels, void* workspace, size_t workspace_bytes, int* n_rows,
                  void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CLS_VALID;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = CIN; op.i[RCV_I_COUT] = COUT; op.i[RCV_I_INMODE] = 0;
  op.p[RCV_P_IN] = (void*)x; op.p[RCV_P_W] = (void*)w; op.p[RCV_P_BIAS] = (void*)bias; op.p[RCV_P_IN2] = (void*)targets;
  op.p[RCV_P_X0] = (void*)class_weights; op.p[RCV_P_X2] = counts; op.p[RCV_P_OUT] = labels; op.p[RCV_P_PART] = workspace;
  size_t need = 0;
  const int rc = rcv_op_workspace(h, &op, &need);
  if (rc) return rc;
  RCV_CHECK_ARG(workspace_bytes >= need, "rcv_cls_valid: workspace of %zu bytes given, %zu needed (rcv_op_workspace)", workspace_bytes, need);
  if (n_rows) *n_rows = op.i[RCV_I_NPART];
  return rcv_run(h, &op, 1, stream);
}

int rcv_cls_proba(rcv_handle* h, const float* x, const float* w, const float* bias, int N, int H, int W, int CIN, int COUT, float* proba,
                  uint8_t* labels, float* confidence, int64_t* pseudo, float threshold, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CLS_PROBA;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = CIN; op.i[RCV_I_COUT] = COUT; op.i[RCV_I_INMODE] = 0;
  op.f[0] = threshold;
  op.p[RCV_P_IN] = (void*)x; op.p[RCV_P_W] = (void*)w; op.p[RCV_P_BIAS] = (void*)bias; op.p[RCV_P_X0] = proba; op.p[RCV_P_OUT] = labels;
  op.p[RCV_P_X1] = confidence; op.p[RCV_P_X2] = pseudo;
  return rcv_run(h, &op, 1, stream);
}

int rcv_cls_calib(rcv_handle* h, const float* x, const float* w, const float* bias, int N, int H, int W, int CIN, int COUT, const int64_t* targets,
                  const float* edges, int K, int64_t* state, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_CLS_CALIB;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_CIN] = CIN; op.i[RCV_I_COUT] = COUT; op.i[RCV_I_INMODE] = 0;
  op.i[RCV_I_COUNT] = K;
  op.p[RCV_P_IN] = (void*)x; op.p[RCV_P_W] = (void*)w; op.p[RCV_P_BIAS] = (void*)bias; op.p[RCV_P_IN2] = (void*)targets;
  op.p[RCV_P_X0] = (void*)edges; op.p[RCV_P_X2] = state;
  return rcv_run(h, &op, 1, stream);
}

int rcv_valid_fold(rcv_handle* h, int32_t* counts, const float* rows, int n_rows, const float* loss, int N, int H, int W, int num_class,
                   double* state, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_VALID_FOLD;
  op.i[RCV_I_N] = N; op.i[RCV_I_H] = H; op.i[RCV_I_W] = W; op.i[RCV_I_COUT] = num_class; op.i[RCV_I_NPART] = n_rows;
  op.p[RCV_P_IN] = counts; op.p[RCV_P_IN2] = (void*)rows; op.p[RCV_P_X0] = (void*)loss; op.p[RCV_P_OUT] = state;
  return rcv_run(h, &op, 1, stream);
}

int rcv_bnn_stage_fwd(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_BNN_STAGE_FWD, "rcv_bnn_stage_fwd: record kind must be RCV_OP_BNN_STAGE_FWD");
  return rcv_run(h, op, 1, stream);
}
int rcv_bnn_stage_bwd(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_BNN_STAGE_BWD, "rcv_bnn_stage_bwd: record kind must be RCV_OP_BNN_STAGE_BWD");
  return rcv_run(h, op, 1, stream);
}
int rcv_bnn_head_fwd(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_BNN_HEAD_FWD, "rcv_bnn_head_fwd: record kind must be RCV_OP_BNN_HEAD_FWD");
  return rcv_run(h, op, 1, stream);
}
int rcv_bnn_head_bwd(rcv_handle* h, const rcv_op* op, void* stream) {
  RCV_CHECK_ARG(op && op->kind == RCV_OP_BNN_HEAD_BWD, "rcv_bnn_head_bwd: record kind must be RCV_OP_BNN_HEAD_BWD");
  return rcv_run(h, op, 1, stream);
}

int rcv_sgd_step(rcv_handle* h, float* param, const float* grad, float* momentum_buf, const float* lr_elem, int64_t n, float lr,
                 float momentum, float weight_decay, int step, float grad_scale, void* stream) {
  RCV_CHECK_ARG(n > 0 && n < ((int64_t)1 << 32), "rcv_sgd_step: n out of range");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_SGD;
  op.i[RCV_I_COUNT] = (int32_t)(uint32_t)n; op.i[RCV_I_AUX0] = step;
  op.f[0] = lr; op.f[1] = momentum; op.f[2] = weight_decay; op.f[5] = grad_scale;
  op.p[RCV_P_IN] = param; op.p[RCV_P_IN2] = (void*)grad; op.p[RCV_P_X0] = momentum_buf; op.p[RCV_P_X2] = (void*)lr_elem;
  return rcv_run(h, &op, 1, stream);
}

int rcv_sgd_step_pruned(rcv_handle* h, float* param, const float* grad, float* momentum_buf, const float* lr_elem,
                        const uint8_t* prune_mask, int64_t n, float lr, float momentum, float weight_decay, int step, float grad_scale,
                        void* stream) {
  RCV_CHECK_ARG(n > 0 && n < ((int64_t)1 << 32), "rcv_sgd_step_pruned: n out of range");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_SGD;
  op.i[RCV_I_COUNT] = (int32_t)(uint32_t)n; op.i[RCV_I_AUX0] = step;
  op.f[0] = lr; op.f[1] = momentum; op.f[2] = weight_decay; op.f[5] = grad_scale;
  op.p[RCV_P_IN] = param; op.p[RCV_P_IN2] = (void*)grad; op.p[RCV_P_X0] = momentum_buf; op.p[RCV_P_X2] = (void*)lr_elem;
  op.p[RCV_P_X5] = (void*)prune_mask;
  return rcv_run(h, &op, 1, stream);
}

int rcv_prune_check(const rcv_prune_job* jobs, int n_jobs, int rule) {
  RCV_CHECK_ARG(rule >= RCV_PRUNE_MAX_RATIO && rule <= RCV_PRUNE_SMALLEST_K, "rcv_prune: rule %d unknown (0 = pruneModelNew, 1 = pruneModel, 2 = pruneModel2)", rule);
  RCV_CHECK_ARG(jobs && n_jobs > 0 && n_jobs <= 65535, "rcv_prune: %d jobs (1..65535) or a null table", n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    const rcv_prune_job& b = jobs[j];
    RCV_CHECK_ARG(b.w && b.mask, "rcv_prune: job %d: null pointer", j);
    RCV_CHECK_ARG(((uintptr_t)b.w & 3) == 0, "rcv_prune: job %d: weights are not 4-byte aligned", j);
    RCV_CHECK_ARG(b.n >= 1 && b.n < ((int64_t)1 << 31), "rcv_prune: job %d: %lld elements (1 .. 2^31 - 1)", j, (long long)b.n);
    if (rule == RCV_PRUNE_MAX_RATIO) RCV_CHECK_ARG(b.ratio == b.ratio && b.ratio - b.ratio == 0.f, "rcv_prune: job %d: ratio is not finite", j);
    if (rule == RCV_PRUNE_STD_SEARCH) {
      RCV_CHECK_ARG(b.n >= 2, "rcv_prune: job %d: the standard deviation of %lld element is NaN (pruneModel needs two)", j, (long long)b.n);
      RCV_CHECK_ARG(b.lower - b.lower == 0.0 && b.upper - b.upper == 0.0, "rcv_prune: job %d: the window [lower, upper] is not finite", j);
    }
    if (rule == RCV_PRUNE_SMALLEST_K)
      RCV_CHECK_ARG(b.amount >= 0 && b.amount <= b.n, "rcv_prune: job %d: amount %lld out of range for %lld elements (torch.topk: k not in range)", j,
                    (long long)b.amount, (long long)b.n);
  }
  return RCV_OK;
}

int rcv_prune(rcv_handle* h, rcv_prune_job* jobs, int n_jobs, int rule, void* stream) {
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_PRUNE;
  op.i[RCV_I_COUNT] = n_jobs; op.i[RCV_I_AUX0] = rule;
  op.p[RCV_P_IN] = jobs;
  return rcv_run(h, &op, 1, stream);
}

int rcv_adam_l1_step(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* lr_elem,
                     int64_t n, float lr, float beta1, float beta2, float eps, float decay, int step, float grad_scale,
                     void* stream) {
  RCV_CHECK_ARG(n > 0 && n < 2147483647LL, "rcv_adam_l1_step: n out of range");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_ADAM_L1;
  op.i[RCV_I_COUNT] = (int)n; op.i[RCV_I_AUX0] = step;
  op.f[0] = lr; op.f[1] = beta1; op.f[2] = beta2; op.f[3] = eps; op.f[4] = decay; op.f[5] = grad_scale;
  op.p[RCV_P_IN] = param; op.p[RCV_P_IN2] = (void*)grad; op.p[RCV_P_X0] = exp_avg; op.p[RCV_P_X1] = exp_avg_sq;
  op.p[RCV_P_X2] = (void*)lr_elem;
  return rcv_run(h, &op, 1, stream);
}

int rcv_adam_l1_step_pruned(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* lr_elem,
                            const uint8_t* prune_mask, int64_t n, float lr, float beta1, float beta2, float eps, float decay, int step,
                            float grad_scale, void* stream) {
  RCV_CHECK_ARG(n > 0 && n < 2147483647LL, "rcv_adam_l1_step_pruned: n out of range");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_ADAM_L1;
  op.i[RCV_I_COUNT] = (int)n; op.i[RCV_I_AUX0] = step;
  op.f[0] = lr; op.f[1] = beta1; op.f[2] = beta2; op.f[3] = eps; op.f[4] = decay; op.f[5] = grad_scale;
  op.p[RCV_P_IN] = param; op.p[RCV_P_IN2] = (void*)grad; op.p[RCV_P_X0] = exp_avg; op.p[RCV_P_X1] = exp_avg_sq;
  op.p[RCV_P_X2] = (void*)lr_elem; op.p[RCV_P_X5] = (void*)prune_mask;
  return rcv_run(h, &op, 1, stream);
}

int rcv_adam_l1_step_metrics(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* lr_elem,
                             int64_t n, float lr, float beta1, float beta2, float eps, float decay, int step, float grad_scale,
                             double* metrics, const float* loss_stats, void* workspace, int workspace_rows, void* stream) {
  RCV_CHECK_ARG(n > 0 && n < 2147483647LL, "rcv_adam_l1_step_metrics: n out of range");
  RCV_CHECK_ARG(metrics && loss_stats && workspace, "rcv_adam_l1_step_metrics: null operand");
  rcv_op op;
  memset(&op, 0, sizeof(op));
  op.kind = RCV_OP_ADAM_L1;
  op.i[RCV_I_COUNT] = (int)n; op.i[RCV_I_AUX0] = step; op.i[RCV_I_NPART] = workspace_rows;
  op.f[0] = lr; op.f[1] = beta1; op.f[2] = beta2; op.f[3] = eps; op.f[4] = decay; op.f[5] = grad_scale;
  op.p[RCV_P_IN] = param; op.p[RCV_P_IN2] = (void*)grad; op.p[RCV_P_X0] = exp_avg; op.p[RCV_P_X1] = exp_avg_sq;
  op.p[RCV_P_X2] = (void*)lr_elem; op.p[RCV_P_X3] = metrics; op.p[RCV_P_X4] = (void*)loss_stats; op.p[RCV_P_PART] = workspace;
  return rcv_run(h, &op, 1, stream);
}

}  // extern "C"
