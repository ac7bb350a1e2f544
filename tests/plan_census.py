"""Census of conv / transposed-conv / filter-gradient records on the planning handle (no GPU): what the networks of bench.py,
LabelProp and PB_FCN run (workload_records), what the kernel-level float64 and exact tests run (kernel_case_records, from the very
case tables those tests parametrize over), and how many tiles a workgroup of a persistent kernel loops over (rounds).
tests/test_plan_census.py compares the two sides; the multi-round cases of tests/test_gpu_kernels.py guard themselves with rounds()
on the real handle."""
import ctypes

import conv_record_cases as RC
import small_ops_cases as K
from robocupvision_amd import _lib as L

# bench.py WORKLOADS (constructor arguments, batch, H, W) -- copied, not imported: bench.py parses its command line and imports the
# trainer; tests/test_plan_census.py asserts the copy equals the original
WORKLOAD_CTORS = {
    "robo_unet_640x480_bs32": (dict(noScale=True, planes=8, depth=4, levels=2, bellySize=5, bellyPlanes=128), 32, 480, 640),
    "robo_unet_160x120_bs64": (dict(noScale=False, planes=8, depth=4, levels=2, bellySize=5, bellyPlanes=128), 64, 120, 160),
    "unet_640x480_bs32": (dict(noScale=True, planes=8, depth=4, levels=3, bellySize=0, bellyPlanes=128, pool=True), 32, 480, 640),
    "robo_unet_320x240_bs32": (dict(noScale=True, planes=8, depth=4, levels=2, bellySize=5, bellyPlanes=128), 32, 240, 320),
    "robo_unet_v2_640x480_bs32": (dict(noScale=True, planes=8, depth=4, levels=1, bellySize=9, bellyPlanes=64, v2=True, classSize=3),
                                  32, 480, 640),
    "labelprop_160x120_b2": (None, 2, 120, 160),
    "labelprop_160x120_b64": (None, 64, 120, 160),
}
# the sizes of the PB_FCN / PB_FCN_2 goldens (tests/test_gpu_pbfcn.py): (noScale, v2, input shape)
PBFCN_GOLDEN_SIZES = [(False, False, (2, 3, 48, 64)), (True, False, (1, 3, 64, 96)), (False, False, (4, 3, 120, 160)),
                      (True, False, (2, 3, 240, 320)), (False, True, (2, 3, 48, 64))]

KINDS = {L.OP_CONV: "conv", L.OP_TCONV: "tconv", L.OP_WGRAD: "wgrad"}
FORWARD_LOADS = (L.LOAD_AFFINE, L.LOAD_AFFINE_RELU, L.LOAD_PLAIN, L.LOAD_NCHW)
GRADIENT_LOADS = (L.LOAD_GRAD_ENC, L.LOAD_GRAD_DEC)
# the kernels whose workgroups loop over tiles, and the tile count beyond which their grid stops growing at 4096 CUs: convs_mfma /
# tconvms_mfma 4096 x (at least one workgroup per CU), convn_bf3 / tconvn_bf3 one workgroup per CU, conv_first four
PERSISTENT_CAP = {"convs_mfma": 4096, "tconvms_mfma": 4096, "convn_bf3": 4096, "tconvn_bf3": 4096, "conv_first": 4 * 4096}


def copy_op(op):
    dup = L.RcvOp()
    ctypes.memmove(ctypes.byref(dup), ctypes.byref(op), ctypes.sizeof(L.RcvOp))
    return dup


def label_of(h, op):
    return L.OpList([op]).labels(h)[0]


def direction(op):
    m = op.i[L.RCV_I_INMODE]
    return "gradient" if m in GRADIENT_LOADS else "forward"


def _models():
    import robocupvision_amd.model as M
    for name, (ctor, B, H, W) in WORKLOAD_CTORS.items():
        if ctor is None:      # LabelProp(5, 32) on 8-channel frame pairs: bench.py measures its inference; its training step as well
            yield name, (lambda: M.LabelProp(5, 32)), (B, H, W, 8), (True, False)
        else:
            yield name, (lambda ctor=ctor: M.ROBO_UNet(**ctor)), (B, 3, H, W), (True, False)
    for no_scale, v2, shape in PBFCN_GOLDEN_SIZES:
        make = (lambda: M.PB_FCN_2(False, nClass=5)) if v2 else (lambda no_scale=no_scale: M.PB_FCN(32, 5, 1, no_scale, 0))
        yield "pbfcn%s_%s" % ("2" if v2 else "", "x".join(map(str, shape))), make, shape, (True, False)


_workload_cache = []


def workload_records():
    """[(network, training, kind name, 256-CU label, record)] of every RCV_OP_CONV / _TCONV / _WGRAD record the training and eval
    plans of the networks hold, lowered through the planning handle as tests/test_cls_step_plan.py does."""
    if _workload_cache:
        return _workload_cache
    import torch
    import robocupvision_amd.model as M
    from robocupvision_amd.engine import Engine
    for name, make, shape, modes in _models():
        for training in modes:
            torch.manual_seed(12345678)
            model = make()
            eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
            plan = eng._plan_for([torch.zeros(shape)], training)
            for lst in (plan.fwd, plan.bwd):
                if lst is None or not lst.n:
                    continue
                labels = lst.labels(eng.handle)
                for k in range(lst.n):
                    if lst.arr[k].kind in KINDS:
                        _workload_cache.append((name, training, KINDS[lst.arr[k].kind], labels[k], copy_op(lst.arr[k])))
    return _workload_cache


def kernel_case_records():
    """(test, record) of every conv / transposed-conv / filter-gradient record the kernel-level float64 and exact tests of
    tests/test_gpu_kernels.py run, built by the builders and from the tables those tests use.  (tests/test_gpu_stream_hints.py
    compares two runs of the library with each other, not with a reference: its records do not count.)"""
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT as MAXC
    for shape in RC.CONV_SHAPES:
        for mode_name in RC.CONV_KERNEL_MODES:
            for layout in RC.conv_layouts(shape[3], shape[4], shape[5], 1):
                yield "conv_kernels", RC.conv_kernel_record(shape, mode_name, layout)
    for shape in RC.CONV_RECORD_SHAPES:
        for mode_name in RC.CONV_RECORD_MODES:
            for layout in RC.conv_layouts(*shape[3:7]):
                yield "conv_records", RC.conv_record(shape, mode_name, layout)
    for shape in RC.NCHW_CONV_SHAPES:
        yield "conv_nchw", RC.nchw_conv_record(shape)
    for shape in RC.TINY_CONV_SHAPES:
        for mode_name, flags in RC.TINY_CONV_MODES:
            yield "conv_tiny", RC.tiny_conv_record(shape, mode_name, flags)
    for shape in RC.WGRAD_SHAPES:
        for modes in RC.WGRAD_KERNEL_MODES:
            op = RC.wgrad_kernel_record(shape, modes)
            if op is not None:
                yield "wgrad_kernels", op
    for shape in RC.DILATED_WGRAD_SHAPES + RC.MATRIX_WGRAD_SHAPES:
        for pair in RC.WGRAD_RECORD_PAIRS:
            for matrix_flags in ((0,) if shape[6] != 1 else (0, L.F_MFMA_FP32)):
                yield "wgrad_records", RC.wgrad_record(shape, pair, matrix_flags)
    for shape in RC.NCHW_WGRAD_SHAPES:
        for two in (False, True):
            yield "wgrad_nchw", RC.nchw_wgrad_record(shape, two)
    for shape in RC.TCONV_SHAPES:
        for mode_name in RC.TCONV_KERNEL_MODES:
            for layout in RC.tconv_layouts(shape[3], shape[4], MAXC):
                yield "tconv_kernels", RC.tconv_record(shape, mode_name, layout)
    for shape in RC.DGRAD_SHAPES:
        for mode_name in RC.DGRAD_MODES:
            for layout in RC.conv_layouts(shape[3], shape[4], 1, shape[6]):
                yield "dgrad_records", RC.dgrad_record(shape, mode_name, layout)
    for plane in RC.CLS_DGRAD_PLANES:
        for cout in RC.CLS_DGRAD_COUT:
            yield "cls_dgrad", RC.cls_dgrad_record(plane, cout)
    for shape, load in RC.FOLDED_CONV_CASES:
        for layout in RC.conv_layouts(*shape[3:7]):
            yield "folded_conv", RC.folded_conv_record(shape, load, layout)
    for shape in RC.FOLDED_TCONV_SHAPES:
        for layout in RC.tconv_layouts(shape[3], shape[4], MAXC):
            yield "folded_tconv", RC.folded_tconv_record(shape, layout)
    # epilogue statistics: exact (integer grid) and randn
    for family, shapes in K.STATS_FAMILIES.items():
        for shape in shapes:
            c = K.conv_stats_dims(shape, transposed=family == "tconv", nchw=family == "image")
            for layout, _ in RC.stats_layouts(family, c, MAXC):
                for kind, flags in K.STATS_VARIANTS:
                    yield "stats_exact", RC.stats_record(c, layout, kind, flags)
    for family, shape, layout, prefix in K.CONV_RANDN_CASES:
        c = K.conv_stats_dims(shape, transposed=family == "tconv", nchw=family == "image")
        source = "multi_round_stats_randn" if (family, shape, layout, prefix) == K.MULTI_ROUND_RANDN_CASE else "stats_randn"
        for kind, flags in K.randn_variants(prefix):
            yield source, RC.stats_record(c, layout, kind, flags)
    # the multi-round cases
    for case in RC.MULTI_ROUND_CASES:
        for mode_name in RC.multi_round_modes(case):
            yield "multi_round_fp64", RC.multi_round_record(case, mode_name)
    for case in K.MULTI_ROUND_STATS_CASES:
        c = K.conv_stats_dims(case[1], transposed=case[0] == "tconv", nchw=case[0] == "image")
        for kind, flags in K.multi_round_stats_variants(case):
            yield "multi_round_stats_exact", RC.stats_record(c, case[2], kind, flags)


def rounds(op, handle=None):
    """(grid, tiles) of a record on a persistent kernel: the workgroups it launches on `handle` (default: the 256-CU planning handle)
    and its tile count -- the grid of the 4096-CU planning handle, where every tile has a workgroup of its own.  Both are read from
    i[NPART] of a copy with the statistics forced on where the record has none (one partial row per workgroup).  That the 4096-CU
    grid IS the 256-CU tile count rests on the planner code: convs_plan (csrc/convs_mfma.hip), n3_geometry (csrc/convn_bf3.hip)
    and conv_first_plan (csrc/conv_first.hip) choose the tile from the shape and the LDS limit and read the CU count for the grid
    alone.  The labels, which carry the tile's block count but not its rows and columns, can only show a change of family or
    block count: they must be equal; and the tile count must lie below the family's grid limit at 4096 CUs."""
    def plan(h):
        q = copy_op(op)
        if q.i[L.RCV_I_STATS] == L.STATS_NONE:
            q.i[L.RCV_I_STATS] = L.STATS_FWD
        q.p[L.RCV_P_PART] = None
        L.op_workspace(h, q)
        return label_of(h, q), q.i[L.RCV_I_NPART]
    own = label_of(handle or L.planner_handle(256), copy_op(op))
    label, grid = plan(handle or L.planner_handle(256))
    label_big, tiles = plan(L.planner_handle(4096))
    family = label.split("<")[0]
    assert own == label == label_big, "tile choice differs: %s as it is, %s with statistics, %s at 4096 CUs" % (own, label, label_big)
    assert family in PERSISTENT_CAP, "%s is no persistent kernel" % label
    assert 0 < tiles < PERSISTENT_CAP[family], "%s: %d tiles reach the grid limit at 4096 CUs" % (label, tiles)
    assert 0 < grid <= tiles
    return grid, tiles


def multi_round(family, grid, tiles):
    """The condition of a multi-round case: three rounds or more with a ragged last one, so that the parity of the staging buffer
    returns to its first value (conv_first keeps no buffer across tiles: more than one round, the last ragged)."""
    return tiles % grid != 0 and tiles > (grid if family == "conv_first" else 2 * grid)


def assert_multi_round(op, handle, num_cus, pinned):
    """The guard of a multi-round GPU case: on the real handle the record still loops as its table says.  pinned: (label, grid, tiles)
    at 256 CUs."""
    grid, tiles = rounds(op, handle)
    label = label_of(handle, copy_op(op))
    assert label == pinned[0], "planned on %s, the case was chosen for %s" % (label, pinned[0])
    assert tiles == pinned[2], "%s: %d tiles, the table says %d" % (label, tiles, pinned[2])
    if num_cus == 256:
        assert grid == pinned[1], "%s: %d workgroups on 256 CUs, the table says %d" % (label, grid, pinned[1])
    assert multi_round(label.split("<")[0], grid, tiles), \
        "%s on %d CUs: %d tiles over %d workgroups is no multi-round case any more -- choose a larger shape" % (label, num_cus, tiles, grid)
    return grid, tiles
