"""RCV_OP_CLS_PROBA (include/rcv.h, csrc/cls_proba.hip) restated in float64 numpy: per pixel with logits z_0 .. z_{C-1}

    m = max z,  e_c = exp(z_c - m),  S = sum_c e_c,  p_c = e_c / S;  class = the first maximum (segment_restatement.first_argmax);
    confidence = p[class];  pseudo-label = class where confidence >= tau, else -100.

The probabilities are judged against ``softmax`` of the fp32 logits the device itself forms (RCV_OP_CLS_FWD / RCV_OP_NHWC_TO_NCHW
write them, bit for bit the ones the tail holds in registers), inside ``proba_bound(C)``; class, confidence and pseudo-label are exact
functions of stored values.  tests/test_proba.py pins ``softmax`` to torch.softmax in float64."""
import math

import numpy as np

import segment_restatement as S

U = 2.0 ** -24
IGNORE = -100


def softmax(logits, axis=-1):
    """float64 softmax over ``axis`` with the maximum subtracted first."""
    z = np.asarray(logits).astype(np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def proba_bound(C):
    """|p_c(device) - p_c(float64)| for fp32 logits, C classes, by counted roundings in units of u = 2^-24 (first order; the derivation
    of lp_input_restatement.SOFT_BOUND with C in place of 5): m = max z exact, d_c = z_c - m <= 0, e_c = expf(d_c), S = ((e_0 + e_1) +
    ...) in [1, C], q_c = e_c / S <= 1.
      * d_c: one rounding, relative u, which moves e_c by the relative amount |d_c| u;
      * expf: 2 ulp ASSUMED (ROCm's table of device-function accuracy is not on hand), relative 2 * 2^-23 = 4 u;
      * S: C - 1 additions, every term passes through at most C - 1 of them: relative (C - 1) u on top of the terms' own errors,
        (sum_j |d_j| e_j u + 4 u S) / S <= ((C - 1) / e) u + 4 u, since |d| exp(d) <= 1 / e, S >= 1 and at most C - 1 classes have d != 0;
      * the division: relative u.
    relative error of q_c <= (|d_c| + 4 + (C - 1) / e + 4 + (C - 1) + 1) u, and with q_c |d_c| <= 1 / e and q_c <= 1:
      |dq_c| <= (C / e + C + 8) u        (C = 5: 14.84 u, the figure SOFT_BOUND doubles),
    rounded up to the next integer and one more u for the second-order terms."""
    return (math.ceil(C / math.e + C + 8) + 1) * U


def confidence(prob, classes):
    """prob [N, C, H, W], classes [N, H, W] -> prob[n, classes[n, h, w], h, w], the dtype of prob."""
    prob = np.asarray(prob)
    return np.take_along_axis(prob, np.asarray(classes).astype(np.int64)[:, None], axis=1)[:, 0]


def pseudo_labels(conf, classes, tau):
    """int64: the class where the STORED fp32 confidence >= fp32(tau), else -100 (a NaN confidence passes nothing)."""
    conf = np.asarray(conf, np.float32)
    return np.where(conf >= np.float32(tau), np.asarray(classes).astype(np.int64), IGNORE).astype(np.int64)


def proba(logits_nchw):
    """fp32 (or float64) logits [N, C, H, W] -> (float64 probabilities [N, C, H, W], uint8 classes [N, H, W])."""
    lg = np.asarray(logits_nchw)
    return softmax(lg, axis=1), S.first_argmax(np.moveaxis(lg, 1, -1))
