#!/usr/bin/env python
"""usage: [RCV_LIBRARY=other/librcv.so] python scripts/plan_dump.py > dump.txt
Every routing decision of the conv / transposed-conv / filter-gradient planners, one line per (CU count, record), on planning
handles of 256 and 64 CUs (rcv_create_planner: no GPU needed):

    cus kind flags i[0..16] | rc [error text] | workspace bytes, i[NPART], i[NSPLIT] | kernel label | filter layout (force 0, 1)

Two builds of the library that print the same dump route every record alike (scripts/plan_diff.sh REV compares the working tree
with another revision).  The records: the layer sweep and the dilated / decoder-order cases of tests/test_lib_abi.py, every conv shape
of those once more as an inference record (no statistics, plain load: conv_small's records) and under every filter layout 0..5,
the NCHW first-layer records, and records that must be refused."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from robocupvision_amd import _lib as L      # noqa: E402
import conv_record_cases as RC               # noqa: E402
import small_ops_cases as K                  # noqa: E402
from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT      # noqa: E402
from test_gpu_kernels import TCONV_SHAPES    # noqa: E402


def conv_op(shape, flags=L.F_BIAS, **kw):
    N, H, W, Cin, Cout, s, d = shape
    slots = dict(n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s, dil=d)
    slots.update(kw)
    return L.make_op(L.OP_CONV, flags, **slots)


def records():
    shapes = []        # every conv shape met, once
    for what, op in RC.network_layer_records():
        if what == "conv":
            shapes.append(tuple(op.i[k] for k in (L.RCV_I_N, L.RCV_I_H, L.RCV_I_W, L.RCV_I_CIN, L.RCV_I_COUT, L.RCV_I_STRIDE, L.RCV_I_DIL)))
        yield op
    # what test_planner_routes_the_dilated_and_decoder_order_records plans
    for shape in RC.CONV_RECORD_SHAPES:
        for mode_name in RC.CONV_RECORD_MODES:
            for layout in RC.conv_layouts(*shape[3:]):
                yield RC.conv_record(shape, mode_name, layout)
    for shape in TCONV_SHAPES:
        merged = 1 if shape[4] <= MERGED_TCONV_MAX_COUT else 0
        for layout in [merged] + ([4] if merged and (shape[3], (4 * shape[4] + 15) // 16 * 16) in ((16, 32), (32, 64)) else []):
            for mode_name in RC.TCONV_RECORD_MODES:
                yield RC.tconv_record(shape, mode_name, layout)
    for pair in RC.WGRAD_RECORD_PAIRS:
        for shape in RC.DILATED_WGRAD_SHAPES:
            yield RC.wgrad_record(shape, pair)
        for shape in RC.MATRIX_WGRAD_SHAPES:
            for matrix_flags in (0, L.F_MFMA_FP32):
                yield RC.wgrad_record(shape, pair, matrix_flags)
    for shape in K.DILATED_STATS_SHAPES:
        for kind, flags in K.STATS_VARIANTS:
            yield conv_op(shape, flags, inmode=L.LOAD_AFFINE, aux0=0, stats=kind)
    shapes = list(dict.fromkeys(shapes + RC.CONV_RECORD_SHAPES + K.DILATED_STATS_SHAPES))
    for shape in shapes:
        yield conv_op(shape, inmode=L.LOAD_PLAIN, stats=L.STATS_NONE)                 # inference
        for aux0 in range(6):                                                          # every filter layout, fitting or not
            yield conv_op(shape, inmode=L.LOAD_AFFINE, stats=L.STATS_FWD, aux0=aux0)
    # the first layer: the NCHW image (and what else may carry an NCHW operand)
    for (N, H, W) in RC.NETWORK_PLANES:
        for Cin, Cout, d, stats in ((3, 8, 1, L.STATS_FWD), (3, 8, 2, L.STATS_FWD), (3, 8, 1, L.STATS_NONE), (4, 8, 1, L.STATS_FWD), (3, 16, 1, L.STATS_FWD), (1, 8, 1, L.STATS_FWD)):
            yield conv_op((N, H, W, Cin, Cout, 1, d), inmode=L.LOAD_NCHW, stats=stats)
        yield conv_op((N, H, W, 3, 8, 1, 1), L.F_BIAS | L.F_RESID, inmode=L.LOAD_NCHW, stats=L.STATS_NONE)
        yield conv_op((N, H, W, 3, 8, 2, 1), inmode=L.LOAD_NCHW, stats=L.STATS_FWD)
    # refused records
    yield conv_op((2, 30, 40, 16, 6, 1, 1), inmode=L.LOAD_AFFINE)                      # Cout % 4
    yield conv_op((2, 30, 40, 16, 16, 3, 1), inmode=L.LOAD_AFFINE)                     # stride 3
    yield conv_op((2, 30, 40, 16, 16, 1, 3), inmode=L.LOAD_AFFINE)                     # dilation 3
    yield conv_op((2, 30, 40, 6, 16, 1, 1), inmode=L.LOAD_AFFINE)                      # NHWC Cin % 4
    yield conv_op((2, 30, 40, 8, 16, 1, 1), inmode=L.LOAD_NCHW)                        # NCHW with more than 4 channels
    yield conv_op((2, 30, 40, 16, 16, 1, 1), inmode=L.LOAD_AFFINE, ho=29)              # wrong output plane
    yield conv_op((0, 30, 40, 16, 16, 1, 1), inmode=L.LOAD_AFFINE)                     # empty
    yield RC.tconv_record((2, 15, 20, 64, 64), "plain", 1)                             # merged layout with more than 32 output channels
    yield L.make_op(L.OP_TCONV, L.F_BIAS, n=2, h=15, w=20, cin=64, cout=32, ho=30, wo=41, stride=2, dil=1, inmode=L.LOAD_PLAIN)
    wg = dict(n=2, h=30, w=40, cin=16, ho=30, wo=40, cout=16, stride=1, dil=1)
    yield L.make_op(L.OP_WGRAD, 0, inmode=L.LOAD_AFFINE, inmode2=L.LOAD_NCHW, **wg)      # pointwise NCHW operand
    yield L.make_op(L.OP_WGRAD, 0, inmode=L.LOAD_GRAD_DEC, inmode2=L.LOAD_GRAD_ENC, **wg)  # two gradient loads
    yield L.make_op(L.OP_WGRAD, 0, inmode=L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_DEC, **dict(wg, stride=3))
    yield L.make_op(L.OP_WGRAD, 0, inmode=L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_DEC, **dict(wg, cout=6))
    yield L.make_op(L.OP_WGRAD, 0, inmode=L.LOAD_NCHW, inmode2=L.LOAD_GRAD_DEC, **dict(wg, cin=8))
    yield L.make_op(L.OP_WGRAD_REDUCE, 0, cin=16, cout=16, nsplit=4)
    yield L.make_op(L.OP_WGRAD_REDUCE_BATCH, 0, count=3, npart=7)


def main():
    lib = L.load()
    label = C.create_string_buffer(64)
    for cus in (256, 64):
        h = L.planner_handle(cus)
        for op in records():
            head = "%d %d %#x %s" % (cus, op.kind, op.flags, ",".join(str(op.i[k]) for k in range(17)))
            layouts = "%d %d" % (lib.rcv_op_filter_layout(h, C.byref(op), 0), lib.rcv_op_filter_layout(h, C.byref(op), 1))
            nbytes = C.c_size_t(0)
            rc = lib.rcv_op_workspace(h, C.byref(op), C.byref(nbytes))
            if rc:
                print("%s | %d %s | %s" % (head, rc, lib.rcv_last_error().decode(), layouts))
                continue
            rc2 = lib.rcv_op_kernel_label(h, C.byref(op), label, 64)
            print("%s | 0 | %d %d %d | %s | %s" % (head, nbytes.value, op.i[L.RCV_I_NPART], op.i[L.RCV_I_NSPLIT],
                                                   label.value.decode() if rc2 == 0 else "label: %d %s" % (rc2, lib.rcv_last_error().decode()), layouts))


if __name__ == "__main__":
    main()
