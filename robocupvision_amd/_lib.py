"""ctypes binding of librcv.so (include/rcv.h).  No fallback: if the HIP library is missing or a
call fails, an exception is raised -- the package never computes the hot path any other way."""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCV_LIBRARY: another build of the same library (A/B timing of two builds on one GPU box, scripts/ab.sh); product code never sets it
LIB_PATH = os.environ.get("RCV_LIBRARY") or os.path.join(_HERE, "librcv.so")

RCV_I_N, RCV_I_H, RCV_I_W, RCV_I_CIN, RCV_I_COUT, RCV_I_HO, RCV_I_WO, RCV_I_STRIDE, RCV_I_DIL, \
    RCV_I_INMODE, RCV_I_INMODE2, RCV_I_STATS, RCV_I_NPART, RCV_I_NSPLIT, RCV_I_COUNT, RCV_I_AUX0, RCV_I_AUX1 = range(17)
RCV_I__N = 20
(RCV_P_IN, RCV_P_IN_AUX, RCV_P_IN_C, RCV_P_W, RCV_P_BIAS, RCV_P_OUT, RCV_P_RESID, RCV_P_EPI_AUX, RCV_P_EPI_C,
 RCV_P_PART, RCV_P_IN2, RCV_P_IN2_AUX, RCV_P_IN2_C, RCV_P_X0, RCV_P_X1, RCV_P_X2, RCV_P_X3, RCV_P_X4, RCV_P_X5) = range(19)
RCV_P__N = 20

(OP_CONV, OP_TCONV, OP_WGRAD, OP_WGRAD_REDUCE, OP_PACK, OP_BN_FINALIZE, OP_BN_EVAL, OP_BN_BWD, OP_COMBINE, OP_CLS_FWD,
 OP_CLS_BWD, OP_CE_FWD, OP_CE_BWD, OP_POOL_FWD, OP_POOL_BWD, OP_ADAM_L1, OP_MEMSET, OP_CONV1X1, OP_ADD_SLICE,
 OP_MATERIALIZE, OP_BWD_STATS, OP_CONFUSION, OP_DICE_FWD, OP_DICE_BWD, OP_NHWC_TO_NCHW, OP_NCHW_TO_NHWC, OP_SGD, OP_NOP,
 OP_WGRAD_REDUCE_BATCH, OP_POOL_CLS_FWD, OP_POOL_CLS_BWD) = range(1, 32)
OP_OBJECT_MATCH = 32       # object-detection counts (rcv.h RCV_OP_OBJECT_MATCH, csrc/objdet.hip)
OP_LP_TAIL_FWD, OP_LP_TAIL_BWD, OP_LP_BATCH = 33, 34, 35      # LabelProp's training tail and batch assembly (rcv.h, csrc/lp_tail.hip)
OP_BATCH_PREP = 36          # the loader's per-image work for a whole batch (rcv.h RCV_OP_BATCH_PREP, csrc/batch_prep.hip)
OP_CLS_LABEL = 37           # classifier tail -> uint8 class map (+ colour image), no logits (rcv.h RCV_OP_CLS_LABEL, csrc/cls_label.hip)
OP_FRAME_PREP = 38          # OP_BATCH_PREP's validation form for frames without labels (rcv.h RCV_OP_FRAME_PREP)
OP_BNN_STAGE_FWD, OP_BNN_STAGE_BWD, OP_BNN_HEAD_FWD, OP_BNN_HEAD_BWD = 39, 40, 41, 42      # BNN-L / BNN-M-C stages and head (rcv.h, csrc/bnn.hip)
OP_CE_NORM, OP_CLS_STEP = 43, 44     # the classifier's forward + loss + backward in one pass, and its normaliser pre-pass (rcv.h, csrc/small_kernels.hip)
OP_PRUNE = 45               # the three mask builders of the prune stage, one workgroup per weight tensor (rcv.h RCV_OP_PRUNE, csrc/prune.hip)
OP_OBJECTS = 46             # boxes, areas and centres of the components of a class map (rcv.h RCV_OP_OBJECTS, csrc/objects.hip)
OP_RGB_PREP = 47            # the RGB loader of trainer.py / pruner.py for a whole batch: PIL ColorJitter, rgb2yuv (rcv.h RCV_OP_RGB_PREP, csrc/rgb_prep.hip)
OP_FARNEBACK, OP_REMAP_LABELS = 48, 49      # dense optical flow and the label remap through it (rcv.h RCV_OP_FARNEBACK / RCV_OP_REMAP_LABELS, csrc/flow.hip)
OP_OBJECT_PATCHES = 50      # the boxes of OP_OBJECTS cut out of the frames -> 32x32 YUV patches (rcv.h RCV_OP_OBJECT_PATCHES, csrc/patches.hip)
OP_RESIZE_U8 = 51           # OP_BATCH_PREP's resize stage alone: uint8 NHWC bytes and unmasked labels, what a resident dataset keeps (rcv.h RCV_OP_RESIZE_U8)
OP_BATCH_PREP_IDX = 52      # OP_BATCH_PREP whose image b is store[index[b]], the index in device memory (rcv.h RCV_OP_BATCH_PREP_IDX)
OP_RGB_PREP_IDX = 53        # OP_RGB_PREP whose image b is store[index[b]]: trainer.py:75-123's loader from a resident store (rcv.h RCV_OP_RGB_PREP_IDX)
OP_LP_PAIR_PREP = 54        # both frames of a LabelProp pair from the store -> the 8-channel input of labelPropTrain.py:36-66, 162-193 (rcv.h RCV_OP_LP_PAIR_PREP)
OP_CONV5, OP_WGRAD5, OP_WGRAD5_REDUCE, OP_PACK5 = 55, 56, 57, 58      # the 5x5 classifier convolution family (rcv.h RCV_OP_CONV5 ..., csrc/conv5.hip)
OP_LP_INPUT = 59            # LabelProp's input from a prediction of the previous frame: class map or logits as the prior (rcv.h RCV_OP_LP_INPUT, csrc/lp_input.hip)
OP_CLS_VALID, OP_VALID_FOLD = 60, 61      # the validation tail: loss rows, class map and per-image confusion counts from the logits in registers; its fold into the running state (rcv.h, csrc/cls_valid.hip)
OP_PW, OP_PW_WGRAD, OP_PW_WGRAD_REDUCE = 62, 63, 64      # pointwise (1x1) convolution between feature maps: forward / data gradient, filter gradient, its reduction (rcv.h, csrc/conv_pw.hip)
OP_CROSS_PACK, OP_CROSS_GRAD = 65, 66     # two 1-D filters <-> one dense 3x3 filter with a cross of taps (ConvSep / trConvSep; rcv.h, csrc/conv_pw.hip)
OP_CLS_PROBA = 67           # the softmax tail: probabilities, class map, confidence and confidence-gated pseudo-label, no logits (rcv.h RCV_OP_CLS_PROBA, csrc/cls_proba.hip)
OP_CLS_CALIB = 68           # the calibration tail: counts per predicted class x label x confidence bin and fixed-point confidence sums, nothing per pixel stored (rcv.h RCV_OP_CLS_CALIB, csrc/cls_calib.hip)
CALIB_MAX_EDGES = 32        # i[COUNT] of OP_CLS_CALIB: 1..32 confidence edges; the state is int64 [K + 1][C][C + 3]
CALIB_Q_SCALE = 1 << 26     # its confidence sums are sums of (uint32)(confidence * 2^26)
OP_MAP_FILTER = 69          # a class map through a windowed class count and one decision rule: majority vote, erosion, opening, closing (rcv.h RCV_OP_MAP_FILTER, csrc/map_filter.hip)
MF_MAJORITY, MF_ERODE, MF_ERODE_BITS, MF_DILATE_BITS, MF_OPEN_FINISH, MF_CLOSE_FINISH = range(6)      # i[AUX0] of OP_MAP_FILTER: the rule (rcv.h RCV_MF_*)
MAP_FILTER_TILE_H, MAP_FILTER_TILE_W = 32, 64      # the tile of one of its workgroups (rcv.h RCV_MAP_FILTER_TILE_H / _W)
MAP_FILTER_MAX_WINDOW = 15  # its largest window: 15 * 15 = 225 is what a byte lane of the packed counts holds
MF_OVER_VOID = 1 << 8       # the void bit of MF_CLOSE_FINISH's over set (i[DIL])
VALID_STATE = 76         # doubles of the state OP_VALID_FOLD keeps: loss sum, batches, images, pixels, iou_sum[8], conf[8][8]
LP_PRIOR_U8, LP_PRIOR_LOGITS, LP_PRIOR_I64 = 1, 4, 8      # i[INMODE] of OP_LP_INPUT: the prior's form
PRUNE_MAX_RATIO, PRUNE_STD_SEARCH, PRUNE_SMALLEST_K = range(3)      # i[AUX0] of OP_PRUNE: pruneModelNew / pruneModel / pruneModel2
PRUNE_MAX_ITER = 4096
PRUNE_ST_OK, PRUNE_ST_NO_END, PRUNE_ST_ALL_ZERO, PRUNE_ST_BAD_JOB = range(4)
CLS_LABEL_FEATURES, CLS_LABEL_LOGITS, CLS_LABEL_CLASSMAP = range(3)      # i[INMODE] of OP_CLS_LABEL: the source form

LOAD_PLAIN, LOAD_AFFINE, LOAD_GRAD_ENC, LOAD_GRAD_DEC, LOAD_NCHW, LOAD_AFFINE_RELU = range(6)
STATS_NONE, STATS_FWD, STATS_BWD_ENC, STATS_BWD_DEC = range(4)
F_BIAS, F_RELU, F_RESID, F_OUT_NCHW, F_FLIP, F_TRANSPOSED_SRC, F_ARGMAX, F_TRAINING, F_CONCAT = 1, 2, 4, 8, 16, 32, 64, 128, 256
F_FUSED_UP = 512
F_FUSED_CE = 1024
F_SIDE_STREAM = 1 << 16
F_MFMA_FP32 = 1 << 17      # contract on the fp32 matrix instructions only (rcv.h RCV_F_MFMA_FP32)
F_STREAM_OUT, F_STREAM_PW = 1 << 18, 1 << 19      # force the streaming hints of a record whatever its size (rcv.h RCV_F_STREAM_OUT / _PW)


class RcvOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flags", C.c_uint32), ("i", C.c_int32 * RCV_I__N), ("f", C.c_float * 8),
                ("p", C.c_void_p * RCV_P__N)]


class RcvPackJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("D0", C.c_int32), ("D1", C.c_int32),
                ("rows_from_d1", C.c_int32), ("flip", C.c_int32), ("rows_pad", C.c_int32), ("cols_pad", C.c_int32),
                ("merged", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_void_p)]


class RcvReduceJob(C.Structure):      # struct rcv_reduce_job of include/rcv.h
    _fields_ = [("part", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("nsplit", C.c_int32), ("CB", C.c_int32),
                ("CA", C.c_int32), ("first_block", C.c_int32)]


class RcvPruneJob(C.Structure):       # struct rcv_prune_job of include/rcv.h
    _fields_ = [("w", C.c_void_p), ("mask", C.c_void_p), ("n", C.c_int64), ("amount", C.c_int64), ("lower", C.c_double),
                ("upper", C.c_double), ("ratio", C.c_float), ("thresh", C.c_float), ("result", C.c_int64 * 4)]


EXPORTS = [
    "rcv_create", "rcv_destroy", "rcv_last_error", "rcv_version", "rcv_num_cus", "rcv_op_workspace", "rcv_run",
    "rcv_run_timed", "rcv_op_kernel_label", "rcv_run_ex", "rcv_join_side",
    "rcv_conv3x3", "rcv_convT3x3s2", "rcv_wgrad3x3", "rcv_bn_finalize", "rcv_bn_backward", "rcv_maxpool2x2_fwd",
    "rcv_softmax_ce_argmax_fwd", "rcv_softmax_ce_bwd", "rcv_adam_l1_step", "rcv_adam_l1_step_metrics", "rcv_confusion",
    "rcv_dice_fwd", "rcv_dice_bwd", "rcv_sgd_step", "rcv_create_planner", "rcv_adam_l1_step_pruned", "rcv_op_filter_layout",
    "rcv_object_match", "rcv_labelprop_batch", "rcv_batch_prep", "rcv_frame_prep", "rcv_cls_label", "rcv_colorize",
    "rcv_bnn_stage_fwd", "rcv_bnn_stage_bwd", "rcv_bnn_head_fwd", "rcv_bnn_head_bwd",
    "rcv_sgd_step_pruned", "rcv_prune_check", "rcv_prune", "rcv_find_objects", "rcv_rgb_prep",
    "rcv_farneback_flow", "rcv_update_labels", "rcv_object_patches", "rcv_resize_u8", "rcv_batch_prep_indexed",
    "rcv_rgb_prep_indexed", "rcv_lp_pair_prep", "rcv_conv5x5", "rcv_wgrad5x5", "rcv_op_stream_hints", "rcv_set_stream_min_mb",
    "rcv_lp_input", "rcv_cls_valid", "rcv_valid_fold", "rcv_conv_pw", "rcv_wgrad_pw", "rcv_cls_proba",
    "rcv_cls_calib", "rcv_map_filter",
]


class RcvError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()
_handles = {}


def load():
    """dlopen librcv.so (raises if it has not been built: run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RcvError("librcv.so not found at %s -- build it with `make -C robocupvision_amd/csrc` "
                           "(there is no CPU fallback for the hot path)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.rcv_last_error.restype = C.c_char_p
        lib.rcv_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.rcv_create_planner.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.rcv_destroy.argtypes = [C.c_void_p]
        lib.rcv_num_cus.argtypes = [C.c_void_p]
        lib.rcv_op_workspace.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.POINTER(C.c_size_t)]
        lib.rcv_run.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_int, C.c_void_p]
        lib.rcv_run_ex.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_int, C.c_void_p, C.c_uint32]
        lib.rcv_join_side.argtypes = [C.c_void_p, C.c_void_p]
        lib.rcv_run_timed.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_int, C.c_void_p, C.POINTER(C.c_float)]
        lib.rcv_op_kernel_label.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_char_p, C.c_int]
        lib.rcv_op_filter_layout.argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_int]
        lib.rcv_object_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]
        lib.rcv_find_objects.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                                                  C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                                                                  C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rcv_object_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + \
            [C.c_void_p] * 3
        lib.rcv_farneback_flow.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                                                                                          C.c_size_t, C.c_void_p]
        lib.rcv_update_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.rcv_labelprop_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
        if hasattr(lib, "rcv_lp_input"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_lp_input.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
        lib.rcv_batch_prep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + \
            [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rcv_frame_prep.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        lib.rcv_resize_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + \
            [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        lib.rcv_batch_prep_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + \
            [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4
        lib.rcv_rgb_prep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + \
            [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rcv_rgb_prep_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + \
            [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        lib.rcv_lp_pair_prep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + \
            [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        lib.rcv_cls_label.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 4
        if hasattr(lib, "rcv_cls_valid"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_cls_valid.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_size_t, C.POINTER(C.c_int), C.c_void_p]
            lib.rcv_valid_fold.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2
        if hasattr(lib, "rcv_cls_proba"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_cls_proba.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_float, C.c_void_p]
        if hasattr(lib, "rcv_cls_calib"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_cls_calib.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(lib, "rcv_map_filter"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_map_filter.argtypes = [C.c_void_p] * 3 + [C.c_int] * 10 + [C.c_void_p] * 3
        lib.rcv_colorize.argtypes =[C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3
        lib.rcv_sgd_step.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p]
        lib.rcv_sgd_step_pruned.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p]
        lib.rcv_prune_check.argtypes = [C.POINTER(RcvPruneJob), C.c_int, C.c_int]
        lib.rcv_prune.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        for name in ("rcv_conv3x3", "rcv_convT3x3s2", "rcv_wgrad3x3", "rcv_bnn_stage_fwd", "rcv_bnn_stage_bwd", "rcv_bnn_head_fwd",
                     "rcv_bnn_head_bwd"):
            getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_void_p]
        for name in ("rcv_conv5x5", "rcv_wgrad5x5", "rcv_conv_pw", "rcv_wgrad_pw"):
            if hasattr(lib, name):      # (RCV_LIBRARY may name the build of an older revision: scripts/plan_diff.sh, scripts/ab.sh)
                getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(RcvOp), C.c_void_p]
        if hasattr(lib, "rcv_set_stream_min_mb"):      # (RCV_LIBRARY may name an older build)
            lib.rcv_set_stream_min_mb.argtypes = [C.c_void_p, C.c_double]
            lib.rcv_op_stream_hints.argtypes = [C.c_void_p, C.POINTER(RcvOp)]
        _lib = lib
    return _lib


def _apply_stream_min(h):
    """RCV_STREAM_MIN_MB (MiB; 0 = every streaming hint off, unset = the library's 128 MiB), read once per handle, here: the library
    reads no environment itself."""
    ev = os.environ.get("RCV_STREAM_MIN_MB")
    if ev is not None and hasattr(load(), "rcv_set_stream_min_mb"):
        check(load().rcv_set_stream_min_mb(h, float(ev)), "rcv_set_stream_min_mb")
    return h


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().rcv_last_error().decode("utf-8", "replace")
        raise RcvError("librcv %s failed (%d): %s" % (what, rc, msg))


def handle(device_index: int):
    """One library handle per device (created on first use)."""
    lib = load()
    h = _handles.get(device_index)
    if h is None:
        out = C.c_void_p()
        check(lib.rcv_create(device_index, C.byref(out)), "rcv_create")
        h = _apply_stream_min(out)
        _handles[device_index] = h
    return h


def planner_handle(num_cus: int = 256):
    """A handle without a device (rcv_create_planner): buffer layout / workspace queries only.  Used to lower a graph to its op
    lists on a host without a GPU (tests of the data-parallel bucket logic); every call that would enqueue work fails."""
    lib = load()
    h = _handles.get(("planner", num_cus))
    if h is None:
        out = C.c_void_p()
        check(lib.rcv_create_planner(num_cus, C.byref(out)), "rcv_create_planner")
        h = _apply_stream_min(out)
        _handles[("planner", num_cus)] = h
    return h


def join_side(h, stream_ptr: int):
    """Make the stream wait for everything the handle's side stream holds so far."""
    check(load().rcv_join_side(h, C.c_void_p(stream_ptr)), "rcv_join_side")


# RCV_MFMA_FP32=1: every contraction on the fp32 matrix instructions (the A/B switch for the split-bf16 kernels, rcv.h RCV_F_MFMA_FP32)
MATRIX_FLAGS = F_MFMA_FP32 if os.environ.get("RCV_MFMA_FP32") else 0


def make_op(kind: int, flags: int = 0, **kw) -> RcvOp:
    """Build a record; keyword names are the lower-cased slot names (n=, cin=, p_in=, f0=...)."""
    op = RcvOp()
    op.kind = kind
    op.flags = flags | (MATRIX_FLAGS if kind in (OP_CONV, OP_TCONV, OP_WGRAD) else 0)
    for k, v in kw.items():
        if k.startswith("p_"):
            idx = globals()["RCV_P_" + k[2:].upper()]
            op.p[idx] = v if v else None
        elif k.startswith("f") and k[1:].isdigit():
            op.f[int(k[1:])] = float(v)
        else:
            op.i[globals()["RCV_I_" + k.upper()]] = int(v)
    return op


def op_filter_layout(h, op: RcvOp, force: bool = False) -> int:
    """0: plain [9][Cin][Cout] filter; 2: the library wants the Winograd-transformed filter for this conv record."""
    return int(load().rcv_op_filter_layout(h, C.byref(op), 1 if force else 0))


def op_stream_hints(h, op: RcvOp) -> int:
    """F_STREAM_OUT | F_STREAM_PW bits the library applies to the record (by size against the handle's threshold, or forced)."""
    rc = int(load().rcv_op_stream_hints(h, C.byref(op)))
    if rc < 0:
        check(rc, "rcv_op_stream_hints")
    return rc


def op_workspace(h, op: RcvOp) -> int:
    nbytes = C.c_size_t(0)
    check(load().rcv_op_workspace(h, C.byref(op), C.byref(nbytes)), "rcv_op_workspace")
    return int(nbytes.value)


class OpList:
    """A cached array of records executed by one rcv_run call."""

    def __init__(self, ops):
        self.n = len(ops)
        self.arr = (RcvOp * max(self.n, 1))(*ops)

    def run(self, h, stream_ptr: int):
        if self.n:
            check(load().rcv_run(h, self.arr, self.n, C.c_void_p(stream_ptr)), "rcv_run")

    def run_slice(self, h, stream_ptr: int, start: int, end: int, join: bool = True):
        """Ops [start, end); join=False leaves the side stream un-joined (see join_side)."""
        if end > start:
            first = C.cast(C.byref(self.arr, start * C.sizeof(RcvOp)), C.POINTER(RcvOp))
            check(load().rcv_run_ex(h, first, end - start, C.c_void_p(stream_ptr), 0 if join else 1), "rcv_run_ex")

    def run_timed(self, h, stream_ptr: int):
        """Profiling aid: per-op milliseconds (HIP events around every op; synchronises)."""
        ms = (C.c_float * max(self.n, 1))()
        if self.n:
            check(load().rcv_run_timed(h, self.arr, self.n, C.c_void_p(stream_ptr), ms), "rcv_run_timed")
        return [float(ms[k]) for k in range(self.n)]

    def labels(self, h):
        out = []
        buf = C.create_string_buffer(64)
        for k in range(self.n):
            check(load().rcv_op_kernel_label(h, C.byref(self.arr[k]), buf, 64), "rcv_op_kernel_label")
            out.append(buf.value.decode())
        return out
