"""CPU: the C-ABI library loads and exports every symbol include/rcv.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from robocupvision_amd import _lib as L


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "rcv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rcv_[A-Za-z0-9_]+)\s*\(", src)))


def test_library_exports_header_symbols():
    assert os.path.exists(L.LIB_PATH), "librcv.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    lib = ctypes.CDLL(L.LIB_PATH)
    names = _declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "include/rcv.h declares %s but librcv.so does not export it" % n
    assert set(L.EXPORTS) <= set(names)


def test_version_and_error_text():
    lib = L.load()
    assert lib.rcv_version() == 100
    assert isinstance(lib.rcv_last_error(), bytes)


def test_struct_layout_matches_header():
    # rcv_op: int32 kind, uint32 flags, int32 i[20], float f[8], void* p[20]
    assert ctypes.sizeof(L.RcvOp) == 4 + 4 + 4 * 20 + 4 * 8 + 8 * 20
    assert ctypes.sizeof(L.RcvPackJob) == 8 + 8 + 4 * 8 + 8      # ... + the per-output-channel scale pointer (inference BatchNorm folding)


def test_no_cpu_fallback():
    import torch
    import robocupvision_amd.model as M
    m = M.ROBO_UNet()
    with pytest.raises(L.RcvError):
        m(torch.zeros(1, 3, 16, 16))
    with pytest.raises(L.RcvError):
        M.CrossEntropyLoss2d()(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


def test_planner_handle_plans_but_cannot_enqueue():
    """rcv_create_planner: a handle without a device answers layout queries (identically to a 256-CU MI355X handle) and rejects
    every call that would enqueue work -- there is no way to reach a kernel launch without a real device handle."""
    h = L.planner_handle(256)
    op = L.make_op(L.OP_CONV, L.F_BIAS | L.F_RELU, n=2, h=30, w=40, cin=128, cout=128, ho=30, wo=40, stride=1, dil=1,
                   inmode=L.LOAD_AFFINE, stats=L.STATS_FWD)
    nbytes = L.op_workspace(h, op)
    assert nbytes > 0 and op.i[L.RCV_I_NPART] > 0 and nbytes == op.i[L.RCV_I_NPART] * 2 * 128 * 4
    again = L.make_op(L.OP_CONV, L.F_BIAS | L.F_RELU, n=2, h=30, w=40, cin=128, cout=128, ho=30, wo=40, stride=1, dil=1,
                      inmode=L.LOAD_AFFINE, stats=L.STATS_FWD)
    assert L.op_workspace(h, again) == nbytes and again.i[L.RCV_I_NPART] == op.i[L.RCV_I_NPART]      # cached plan, same answer
    lst = L.OpList([op])
    assert lst.labels(h)[0].startswith("conv_dma")
    with pytest.raises(L.RcvError, match="planning-only"):
        lst.run(h, 0)
    with pytest.raises(L.RcvError, match="planning-only"):
        lst.run_timed(h, 0)
    with pytest.raises(L.RcvError):
        L.planner_handle(0)


def test_shipped_library_does_not_read_the_environment():
    """Experiment knobs are compiled in only by `make EXPERIMENTS=1`: the shipped librcv.so has no getenv on its launch path."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", L.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("nm not available")
    assert not any(tok.split("@")[0] == "getenv" for tok in out.stdout.split()), "librcv.so imports getenv: an experiment build was left in the tree"


def test_planner_accepts_every_layer_shape_of_the_networks():
    """Planner sweep (no GPU): every conv / transposed-conv / filter-gradient record the ROBO-UNet, U-Net and PB_FCN graphs produce at the
    BASELINE sizes and at ragged / tiny planes gets a plan (tile within the LDS limit, workspace size, label), for 256 CUs and for a small
    part (64 CUs).  A shape for which tile selection finds nothing would otherwise only show up as a failed launch on the GPU."""
    import conv_record_cases as RC
    labels = set()
    for cus in (256, 64):
        h = L.planner_handle(cus)
        for what, op in RC.network_layer_records():
            if what == "conv":
                assert L.op_workspace(h, op) >= 0
            elif what == "wgrad":
                assert L.op_workspace(h, op) > 0 and op.i[L.RCV_I_NSPLIT] >= 1
            elif what == "wgrad_nchw":
                assert L.op_workspace(h, op) > 0
            else:
                assert L.op_workspace(h, op) >= 0
                continue
            labels.add(L.OpList([op]).labels(h)[0].split("<")[0])
    assert {"wgrad_mfma", "wgrad_first", "conv_dma", "convs_mfma"} <= labels, labels


def test_planner_routes_the_dilated_and_decoder_order_records():
    """Planner pin (no GPU) of the dilated and decoder-order cases of tests/test_gpu_kernels.py (tests/conv_record_cases.py) and of the
    dilated integer-grid statistics cases (tests/small_ops_cases.py): every record gets a plan, a workspace size and a label for 256 and
    for 64 CUs, and at 256 CUs the kernels reached are the ones written here -- a planner change that moves these cases onto another
    kernel shows as a failure of this test, not as a silent loss of coverage of the kernel they were chosen for."""
    import conv_record_cases as RC
    import small_ops_cases as K
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT
    from test_gpu_kernels import TCONV_SHAPES

    def plan(h, op, statistics=False):
        nbytes = L.op_workspace(h, op)
        if op.kind == L.OP_WGRAD:
            assert nbytes > 0 and op.i[L.RCV_I_NSPLIT] >= 1
        elif statistics:
            assert op.i[L.RCV_I_NPART] > 0 and nbytes == op.i[L.RCV_I_NPART] * 2 * op.i[L.RCV_I_COUT] * 4
        else:
            assert nbytes == 0
        label = L.OpList([op]).labels(h)[0]
        assert "<" in label, label
        return label

    reached = {}
    for cus in (256, 64):
        h = L.planner_handle(cus)
        conv, tconv, wgrad, stats, census = set(), set(), set(), set(), set()
        # 1. conv records: every shape x load mode x filter layout
        for shape in RC.CONV_RECORD_SHAPES:
            N, H, W, Cin, Cout, s, d = shape
            for mode_name, (_, _, st) in RC.CONV_RECORD_MODES.items():
                for layout in RC.conv_layouts(Cin, Cout, s, d):
                    label = plan(h, RC.conv_record(shape, mode_name, layout), st != L.STATS_NONE)
                    assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout in (3, 5)), (shape, label)
                    if cus == 256 and shape in RC.DILATED_CONV_LABELS:
                        assert label == RC.DILATED_CONV_LABELS[shape], (shape, mode_name, label)
                    if cus == 256 and (shape, layout) in RC.CENSUS_CONV_LABELS:      # the tilings only whole networks reached
                        assert label == RC.CENSUS_CONV_LABELS[(shape, layout)], (shape, layout, mode_name, label)
                        census.add((shape, layout))
                    conv.add(label.split("<")[0])
        for shape in TCONV_SHAPES:
            merged = 1 if shape[4] <= MERGED_TCONV_MAX_COUT else 0
            for layout in [merged] + ([4] if merged and (shape[3], (4 * shape[4] + 15) // 16 * 16) in ((16, 32), (32, 64)) else []):
                for mode_name in RC.TCONV_RECORD_MODES:
                    label = plan(h, RC.tconv_record(shape, mode_name, layout))
                    assert ("_bf3" in label) == (layout == 4), (shape, label)
                    if cus == 256 and (shape, layout) in RC.CENSUS_TCONV_LABELS:
                        assert label == RC.CENSUS_TCONV_LABELS[(shape, layout)], (shape, layout, mode_name, label)
                        census.add((shape, layout))
                    tconv.add(label.split("<")[0])
        assert cus != 256 or census == set(RC.CENSUS_CONV_LABELS) | set(RC.CENSUS_TCONV_LABELS)
        # 2. filter-gradient records: the dilated ones, and dilation 1 as routed and under RCV_F_MFMA_FP32
        dilated = set()
        for pair in RC.WGRAD_RECORD_PAIRS:
            for shape in RC.DILATED_WGRAD_SHAPES:
                label = plan(h, RC.wgrad_record(shape, pair))
                assert label.startswith("wgrad_mfma<"), (shape, label)
                dilated.add(label)
                wgrad.add(label.split("<")[0])
            for shape in RC.MATRIX_WGRAD_SHAPES:
                for k, matrix_flags in enumerate((0, L.F_MFMA_FP32)):
                    label = plan(h, RC.wgrad_record(shape, pair, matrix_flags))
                    if cus == 256:
                        assert label == RC.MATRIX_WGRAD_LABELS[shape][k], (shape, pair, matrix_flags, label)
                        assert label.split("<")[0] == RC.wgrad_kernel(shape, matrix_flags)
                    assert not (matrix_flags and "_bf3" in label), (shape, label)
                    wgrad.add(label.split("<")[0])
        if cus == 256:
            assert dilated == RC.DILATED_WGRAD_LABELS, sorted(dilated)
        # 3. the dilated integer-grid statistics cases, every variant
        for shape in K.DILATED_STATS_SHAPES:
            N, H, W, Cin, Cout, s, d = shape
            for kind, flags in K.STATS_VARIANTS:
                op = L.make_op(L.OP_CONV, flags, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s, dil=d,
                               inmode=L.LOAD_AFFINE, aux0=0, stats=kind)
                stats.add(plan(h, op, True).split("<")[0])
        reached[cus] = dict(conv=conv, tconv=tconv, wgrad=wgrad, stats=stats)
    assert reached[256] == dict(conv={"conv_dma", "conv_mfma", "convs_mfma", "conv_wino", "conv_bf3", "conv2_bf3", "convn_bf3"},
                                tconv={"tconva_dma", "tconvms_mfma", "tconvn_bf3", "tconv_dma", "tconvm_dma"},
                                wgrad={"wgrad_mfma", "wgrad_bf3", "wgradn_bf3"},
                                stats={"conv_dma", "conv_mfma", "convs_mfma"}), reached[256]


def test_planner_routes_the_flipped_and_folded_filter_records():
    """Planner pin (no GPU) of the records behind the packer's flip and scale branches (tests/conv_record_cases.py; run against float64
    by tests/test_gpu_kernels.py): the stride-1 data gradients under every filter layout and gradient load, the 3x3 classifier's data
    gradient, and the folded inference records.  Every record gets a plan and no workspace for 256 and for 64 CUs; at 256 CUs the label
    is the one written in the case tables."""
    import conv_record_cases as RC
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT

    def plan(h, op):
        assert L.op_workspace(h, op) == 0
        label = L.OpList([op]).labels(h)[0]
        assert "<" in label, label
        return label

    for cus in (256, 64):
        h = L.planner_handle(cus)
        pinned = cus == 256
        seen = set()
        for shape in RC.DGRAD_SHAPES:
            N, H, W, Cin, Cout, s, d = shape
            for layout in RC.conv_layouts(Cin, Cout, 1, d):
                for mode_name in RC.DGRAD_MODES:
                    label = plan(h, RC.dgrad_record(shape, mode_name, layout))
                    assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout == 3), (shape, label)
                    assert not label.startswith("conv_small"), (shape, label)
                    assert not pinned or label == RC.DGRAD_LABELS[(shape, layout)], (shape, layout, mode_name, label)
                seen.add((shape, layout))
        assert seen == set(RC.DGRAD_LABELS)
        for plane in RC.CLS_DGRAD_PLANES:
            for cout in RC.CLS_DGRAD_COUT:
                label = plan(h, RC.cls_dgrad_record(plane, cout))
                assert not pinned or label == RC.CLS_DGRAD_LABELS[(plane, cout)], (plane, cout, label)
        seen = set()
        for shape, load in RC.FOLDED_CONV_CASES:
            N, H, W, Cin, Cout, s, d = shape
            for layout in RC.conv_layouts(Cin, Cout, s, d):
                label = plan(h, RC.folded_conv_record(shape, load, layout))
                assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout in (3, 5)), (shape, label)
                assert not pinned or label == RC.FOLDED_CONV_LABELS[(shape, load, layout)], (shape, load, layout, label)
                seen.add((shape, load, layout))
        assert seen == set(RC.FOLDED_CONV_LABELS)
        seen = set()
        for shape in RC.FOLDED_TCONV_SHAPES:
            for layout in RC.tconv_layouts(shape[3], shape[4], MERGED_TCONV_MAX_COUT):
                label = plan(h, RC.folded_tconv_record(shape, layout))
                assert ("_bf3" in label) == (layout == 4), (shape, label)
                assert not pinned or label == RC.FOLDED_TCONV_LABELS[(shape, layout)], (shape, layout, label)
                seen.add((shape, layout))
        assert seen == set(RC.FOLDED_TCONV_LABELS)
