// The softmax arithmetic of the classifier tails, stated once for RCV_OP_CLS_PROBA (cls_proba.hip) and RCV_OP_CLS_CALIB (cls_calib.hip):
//   m = the first maximum of z in class order (`z_c > m` from -inf; a NaN never wins), cls = its index,
//   e_c = expf(z_c - m),  S = ((e_0 + e_1) + e_2) + ... in class order,  p_c = e_c / S with an IEEE division; no fast intrinsics.
// The confidence is p[cls], the very float of pr[]: a record that bins it sees bit for bit what RCV_OP_CLS_PROBA stores.
//
// CLS_SOFTMAX(lg, COUT, pr, am, cf) declares, in the scope that uses it, float pr[CLS_MAX_OUT] (p_c, 0 for c >= COUT), int am (cls)
// and float cf (pr[am]) from the logits float lg[CLS_MAX_OUT]; it also declares cls_sm_mx, cls_sm_e and cls_sm_S.  A macro on purpose:
// an inlined function is simplified on its own before it is inlined, which reorders the code around it, and cls_proba.hip's kernels
// keep the instruction stream they had when these lines stood in cp_tail (scripts/isa_diff.sh).
#pragma once
#include "cls_common.h"

#define CLS_SOFTMAX(lg, COUT, pr, am, cf)                                                                     \
  float cls_sm_mx = -INFINITY;                                                                                \
  int am = 0;                                                                                                 \
  _Pragma("unroll")                                                                                           \
  for (int c = 0; c < CLS_MAX_OUT; ++c) if (c < (COUT) && (lg)[c] > cls_sm_mx) { cls_sm_mx = (lg)[c]; am = c; } \
  float cls_sm_e[CLS_MAX_OUT];                                                                                \
  float cls_sm_S = 0.f;                                                                                       \
  _Pragma("unroll")                                                                                           \
  for (int c = 0; c < CLS_MAX_OUT; ++c) {                                                                     \
    cls_sm_e[c] = c < (COUT) ? expf((lg)[c] - cls_sm_mx) : 0.f;                                               \
    if (c == 0) cls_sm_S = cls_sm_e[0];                                                                       \
    else if (c < (COUT)) cls_sm_S += cls_sm_e[c];                                                             \
  }                                                                                                           \
  float pr[CLS_MAX_OUT];                                                                                      \
  float cf = 0.f;                                                                                             \
  _Pragma("unroll")                                                                                           \
  for (int c = 0; c < CLS_MAX_OUT; ++c) {                                                                     \
    pr[c] = c < (COUT) ? __fdiv_rn(cls_sm_e[c], cls_sm_S) : 0.f;                                              \
    if (c == am) cf = pr[c];                                                                                  \
  }
