"""CPU: what the networks run against what the kernel-level tests run (tests/plan_census.py), on the planning handle.

Label coverage: every kernel instantiation (full label, template arguments included) that a conv / transposed-conv / filter-gradient
record of the bench.py workloads, of LabelProp or of PB_FCN / PB_FCN_2 reaches is reached by a record of the kernel-level float64 /
exact tests of the same kind -- for the conv kernels under a forward load and, where the networks run it on a gradient (the
two-tensor template branch), under a gradient load as well.  No exceptions.

Round coverage: the persistent kernels loop over tiles inside a workgroup; every family has float64 cases and an exact-statistics case
on which, on 256 CUs, a workgroup runs three rounds or more with a ragged last one.  Their (label, workgroups, tiles) are pinned: a
planner change shows here, not as lost coverage.  The 5x5 classifier family and the pointwise family (RCV_OP_CONV5 / _WGRAD5 / _PW /
_PW_WGRAD, outside the census above) have their multi-round tables in tests/persistent_cases.py, checked further down."""
import ast
import os

import pytest

import conv_record_cases as RC
import persistent_cases as PCS
import plan_census as PC
import small_ops_cases as K
from conftest import ROOT
from robocupvision_amd import _lib as L

PERSISTENT = ("convs_mfma", "tconvms_mfma", "convn_bf3", "tconvn_bf3", "conv_first")
# The new case tables, entry for entry ((what, shape, filter layout, (label, workgroups, tiles on 256 CUs))): a case taken out of, or
# changed in, tests/conv_record_cases.py or tests/small_ops_cases.py fails here, also where another case still reaches its label.
MULTI_ROUND_PINS = [
    ("conv", (65, 64, 80, 8, 8, 1), 0, ("convs_mfma<1,5,8>", 347, 1040)),
    ("conv", (13, 96, 128, 8, 8, 1), 3, ("convn_bf3<8,1,5>", 256, 520)),
    ("conv", (65, 64, 80, 16, 16, 1), 0, ("convs_mfma<1,5,16>", 347, 1040)),
    ("conv", (13, 96, 128, 16, 16, 1), 3, ("convn_bf3<16,1,5>", 256, 520)),
    ("conv", (19, 64, 80, 32, 32, 1), 0, ("convs_mfma<2,3,32>", 178, 532)),
    ("conv", (19, 64, 80, 32, 32, 1), 3, ("convn_bf3<32,2,3>", 256, 532)),
    ("conv", (31, 100, 140, 16, 32, 2), 0, ("convs_mfma<2,2,16>", 352, 1054)),
    ("conv", (52, 64, 80, 16, 32, 2), 3, ("convn_bf3<16,2,3>", 256, 520)),
    ("conv", (52, 100, 140, 8, 16, 2), 0, ("convs_mfma<1,3,8>", 347, 1040)),
    ("conv", (43, 100, 140, 8, 16, 2), 3, ("convn_bf3<8,1,5>", 256, 516)),
    ("tconv", (65, 64, 80, 16, 8), 1, ("tconvms_mfma<2,5,16>", 347, 1040)),
    ("tconv", (12, 100, 140, 16, 8), 4, ("tconvn_bf3<16,2,5>", 256, 540)),
    ("tconv", (37, 64, 80, 32, 16), 1, ("tconvms_mfma<4,3,32>", 346, 1036)),
    ("tconv", (9, 96, 128, 32, 16), 4, ("tconvn_bf3<32,4,3>", 256, 576)),
    ("first", (73, 100, 140, 3, 8, 1), 0, ("conv_first<1>", 1024, 1533)),
]
MULTI_ROUND_STATS_PINS = [
    ("conv", (65, 64, 80, 8, 8, 1), 0, ("convs_mfma<1,5,8>", 347, 1040)),
    ("conv", (13, 96, 128, 8, 8, 1), 3, ("convn_bf3<8,1,5>", 256, 520)),
    ("tconv", (65, 64, 80, 16, 8), 1, ("tconvms_mfma<2,5,16>", 347, 1040)),
    ("tconv", (9, 96, 128, 32, 16), 4, ("tconvn_bf3<32,4,3>", 256, 576)),
    ("image", (73, 100, 140, 3, 8, 1, 1), 0, ("conv_first<1>", 1024, 1533)),
]
MULTI_ROUND_RANDN_PIN = (("conv", (19, 64, 80, 32, 32, 1), 3, "convn_bf3"), ("convn_bf3<32,2,3>", 256, 532))
CENSUS_CONV_PINS = {
    ((2, 128, 171, 64, 32, 1, 1), 0): "conv_mfma<2,5,1,4,8>", ((52, 44, 59, 16, 64, 2, 1), 0): "conv_mfma<2,5,2,2,8>",
    ((2, 15, 20, 16, 32, 1, 1), 3): "convn_bf3<16,2,5>", ((2, 30, 40, 32, 16, 1, 1), 3): "convn_bf3<32,1,5>",
    ((2, 8, 10, 16, 16, 2, 1), 0): "convs_mfma<1,2,16>", ((2, 16, 24, 16, 16, 1, 1), 0): "convs_mfma<1,3,16>",
    ((2, 16, 24, 16, 32, 1, 2), 0): "convs_mfma<2,3,16>", ((2, 8, 10, 8, 32, 2, 1), 0): "convs_mfma<2,3,8>",
    ((2, 15, 20, 16, 32, 1, 2), 0): "convs_mfma<2,5,16>",
}
CENSUS_TCONV_PINS = {
    ((64, 8, 11, 128, 64), 0): "tconv_dma<2,5,2,2,4>", ((64, 20, 27, 64, 16), 1): "tconvm_dma<2,5,2,2,4>",
    ((2, 16, 24, 16, 8), 1): "tconvms_mfma<2,3,16>", ((2, 8, 10, 32, 8), 1): "tconvms_mfma<2,3,32>",
    ((2, 30, 40, 32, 16), 4): "tconvn_bf3<32,4,5>",
}
WGRAD_FIRST_PIN = ((65, 64, 80, 3, 8, 1, 1), ("wgrad_first<1>", 347, 1040))


def test_the_new_case_tables_are_what_is_pinned_here():
    assert RC.MULTI_ROUND_CASES == MULTI_ROUND_PINS
    assert K.MULTI_ROUND_STATS_CASES == MULTI_ROUND_STATS_PINS
    assert (K.MULTI_ROUND_RANDN_CASE, K.MULTI_ROUND_RANDN_PIN) == MULTI_ROUND_RANDN_PIN and K.CONV_RANDN_CASES[-1] == K.MULTI_ROUND_RANDN_CASE
    assert RC.CENSUS_CONV_LABELS == CENSUS_CONV_PINS and set(RC.CENSUS_CONV_SHAPES) <= set(RC.CONV_RECORD_SHAPES)
    assert RC.CENSUS_TCONV_LABELS == CENSUS_TCONV_PINS and {sh for sh, _ in CENSUS_TCONV_PINS} <= set(RC.TCONV_SHAPES)
    assert RC.WGRAD_FIRST_MULTI_ROUND == WGRAD_FIRST_PIN and WGRAD_FIRST_PIN[0] in RC.NCHW_WGRAD_SHAPES


def _planned_label(h, op):
    q = PC.copy_op(op)
    if q.i[L.RCV_I_STATS] != L.STATS_NONE or q.kind == L.OP_WGRAD:
        L.op_workspace(h, q)
    return PC.label_of(h, q)


@pytest.fixture(scope="module")
def case_labels():
    """(kind name, label) -> directions, over every kernel-level case."""
    h = L.planner_handle(256)
    out = {}
    for test, op in PC.kernel_case_records():
        out.setdefault((PC.KINDS[op.kind], _planned_label(h, op)), set()).add(PC.direction(op))
    return out


def test_workload_constructor_arguments_equal_bench():
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    node = [n for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "WORKLOADS"]
    assert len(node) == 1
    workloads = eval(compile(ast.Expression(node[0].value), "bench.py", "eval"), {"__builtins__": {}, "dict": dict})
    assert workloads == PC.WORKLOAD_CTORS


def test_every_label_the_networks_reach_has_a_kernel_level_case(case_labels):
    need = {}
    for name, training, kind, label, op in PC.workload_records():
        need.setdefault((kind, label), {}).setdefault(PC.direction(op), (name, training, tuple(op.i[k] for k in range(9)), op.i[L.RCV_I_AUX0]))
    assert len(need) > 50 and {k for k, _ in need} == {"conv", "tconv", "wgrad"}
    missing = []
    for key in sorted(need):
        got = case_labels.get(key, set())
        if key[0] == "wgrad":
            want = set() if got else {"any load"}
        else:
            want = ({"forward"} | set(need[key])) - got
        if want:
            missing.append((key, sorted(want), need[key]))
    assert not missing, "no kernel-level case for:\n" + "\n".join(map(repr, missing))


def test_census_shapes_select_the_labels_they_were_added_for(case_labels):
    """(the same pins as tests/test_lib_abi.py, here against the census: the added shapes are what closes it)"""
    for (shape, layout), label in RC.CENSUS_CONV_LABELS.items():
        assert ("conv", label) in case_labels and case_labels[("conv", label)] == {"forward", "gradient"}, label
    for (shape, layout), label in RC.CENSUS_TCONV_LABELS.items():
        assert ("tconv", label) in case_labels and case_labels[("tconv", label)] == {"forward", "gradient"}, label


def _pinned(op, pin):
    grid, tiles = PC.rounds(op)
    label = _planned_label(L.planner_handle(256), op)
    assert (label, grid, tiles) == pin, ((label, grid, tiles), pin)
    assert PC.multi_round(label.split("<")[0], grid, tiles), (label, grid, tiles)
    return label.split("<")[0]


def test_multi_round_cases_are_pinned_and_cover_every_persistent_family():
    used = {f: set() for f in PERSISTENT}         # directions the networks run each family in
    for name, training, kind, label, op in PC.workload_records():
        if label.split("<")[0] in used:
            used[label.split("<")[0]].add(PC.direction(op))
    assert all(used.values()), used
    fp64 = {f: set() for f in PERSISTENT}
    for case in RC.MULTI_ROUND_CASES:
        for mode_name in RC.multi_round_modes(case):
            for stream in (False, True):
                op = RC.multi_round_record(case, mode_name, stream)
                family = _pinned(op, case[3])
                mode, flags, stats = RC.MULTI_ROUND_MODES[mode_name]
                # forward: with the partial rows of RCV_STATS_FWD; gradient: with the residual
                assert (stats == L.STATS_FWD) if PC.direction(op) == "forward" else bool(flags & L.F_RESID)
                fp64[family].add(PC.direction(op))
    for family in PERSISTENT:
        assert used[family] <= fp64[family], (family, used[family], fp64[family])
    exact = set()
    for case in K.MULTI_ROUND_STATS_CASES:
        c = K.conv_stats_dims(case[1], transposed=case[0] == "tconv", nchw=case[0] == "image")
        for kind, flags in K.multi_round_stats_variants(case):
            exact.add(_pinned(RC.stats_record(c, case[2], kind, flags), case[3]))
    assert exact == set(PERSISTENT), exact
    family, shape, layout, prefix = K.MULTI_ROUND_RANDN_CASE
    c = K.conv_stats_dims(shape)
    for kind, flags in K.randn_variants(prefix):
        assert _pinned(RC.stats_record(c, layout, kind, flags), K.MULTI_ROUND_RANDN_PIN) == prefix


def _wgradn_rounds(op, label, h):
    """(workgroups, tiles) of a record on wgradn_bf3<TH,stride> (csrc/wgradn_bf3.hip wgradn_bf3_plan): tiles of TH x 16 output pixels,
    N * ceil(Wo / 16) * ceil(Ho / TH) of them whatever the CU count; four splits (one per consumer wave) per workgroup.  The kernel
    declines planes with fewer 8 x 16 tiles than CUs, so the 4096-CU planner cannot be asked: it routes these records elsewhere."""
    th = int(label[len("wgradn_bf3<"):].split(",")[0])
    tiles = op.i[L.RCV_I_N] * -(-op.i[L.RCV_I_WO] // 16) * -(-op.i[L.RCV_I_HO] // th)
    assert op.i[L.RCV_I_NSPLIT] % 4 == 0
    return op.i[L.RCV_I_NSPLIT] // 4, tiles


def test_filter_gradient_rounds():
    """The filter-gradient kernels loop over pixel tiles per split.  Tiles per workgroup of the kernel-level cases on 256 CUs, the most
    per family (printed, pytest -s).  wgrad_mfma, wgrad_bf3, wgrad_first: i[NSPLIT] on 4096 CUs, where every tile is a split of its
    own, over i[NSPLIT] on 256 -- for the records whose label is the same on both (the tile choice of these planners reads no CU
    count); wgradn_bf3: from its plan's formula (_wgradn_rounds).  Asserted: wgrad_mfma reaches eight rounds, wgrad_bf3 and wgradn_bf3
    two ((8, 64, 128, 32, 32, 1): 512 tiles over 256 workgroups; never three) -- none of them stays at one, so they get no new case;
    wgrad_first ran ONE tile per workgroup at every earlier shape and has a three-round case now, pinned here."""
    h, big = L.planner_handle(256), L.planner_handle(4096)
    most = {}
    for test, op in PC.kernel_case_records():
        if op.kind != L.OP_WGRAD:
            continue
        a, b = PC.copy_op(op), PC.copy_op(op)
        L.op_workspace(h, a), L.op_workspace(big, b)
        label = PC.label_of(h, a)
        family = label.split("<")[0]
        if family == "wgradn_bf3":
            grid, tiles = _wgradn_rounds(a, label, h)
            assert grid <= 256 and grid <= tiles <= 2 * grid, (label, grid, tiles)
        elif label == PC.label_of(big, b):
            grid, tiles = a.i[L.RCV_I_NSPLIT], b.i[L.RCV_I_NSPLIT]
        else:
            continue
        if tiles / grid > most.get(family, (0.0,))[0]:
            most[family] = (tiles / grid, label, tuple(op.i[k] for k in range(9)), grid, tiles)
    print("most tiles per workgroup of the filter-gradient cases:")
    for family in sorted(most):
        print("  %s: %.2f  %s" % (family, most[family][0], most[family][1:]))
    assert set(most) == {"wgrad_mfma", "wgrad_bf3", "wgradn_bf3", "wgrad_first"}, sorted(most)
    assert most["wgrad_mfma"][0] >= 8 and most["wgrad_bf3"][0] >= 2 and most["wgrad_first"][0] > 2, most
    assert most["wgradn_bf3"][0] == 2.0 and most["wgradn_bf3"][3:] == (256, 512), most["wgradn_bf3"]
    shape, (label, splits, tiles) = RC.WGRAD_FIRST_MULTI_ROUND
    for two in (False, True):
        a, b = RC.nchw_wgrad_record(shape, two), RC.nchw_wgrad_record(shape, two)
        L.op_workspace(h, a), L.op_workspace(big, b)
        assert (PC.label_of(h, a), PC.label_of(big, b)) == (label, label)
        assert (a.i[L.RCV_I_NSPLIT], b.i[L.RCV_I_NSPLIT]) == (splits, tiles) and tiles > 2 * splits and tiles % splits and tiles < 4096
    # every other first-layer shape: one tile per workgroup
    for other in RC.NCHW_WGRAD_SHAPES:
        a, b = RC.nchw_wgrad_record(other, False), RC.nchw_wgrad_record(other, False)
        L.op_workspace(h, a), L.op_workspace(big, b)
        if other != shape and PC.label_of(h, a).startswith("wgrad_first"):
            assert PC.label_of(big, b) == PC.label_of(h, a) and a.i[L.RCV_I_NSPLIT] == b.i[L.RCV_I_NSPLIT], other


# ------------------------------------------------------------------ the 5x5 and the pointwise families (tests/persistent_cases.py)
# The tables entry for entry, as above: (label, workgroups, work items on 256 CUs).
C5_PLANE_PINS = [((11, 121, 161), "8x32", 1056), ((345, 33, 16), "16x16", 1035)]
CONV5_PINS = [
    ("forward", (11, 121, 161), 8, 8, ("conv5_mfma<8,8x32>", 512, 1056)), ("dgrad", (11, 121, 161), 8, 8, ("conv5_mfma<8,8x32>", 512, 1056)),
    ("forward", (11, 121, 161), 16, 8, ("conv5_mfma<16,8x32>", 512, 1056)), ("dgrad", (11, 121, 161), 8, 16, ("conv5_mfma<8,8x32>", 512, 1056)),
    ("forward", (345, 33, 16), 8, 8, ("conv5_mfma<8,16x16>", 512, 1035)), ("dgrad", (345, 33, 16), 8, 8, ("conv5_mfma<8,16x16>", 512, 1035)),
    ("forward", (345, 33, 16), 16, 8, ("conv5_mfma<16,16x16>", 512, 1035)), ("dgrad", (345, 33, 16), 8, 16, ("conv5_mfma<8,16x16>", 512, 1035)),
]
WGRAD5_PINS = [
    ((11, 121, 161), 8, ("wgrad5_mfma<8,8x32>", 256, 1056)), ((11, 121, 161), 16, ("wgrad5_mfma<16,8x32>", 256, 1056)),
    ((345, 33, 16), 8, ("wgrad5_mfma<8,16x16>", 256, 1035)), ((345, 33, 16), 16, ("wgrad5_mfma<16,16x16>", 256, 1035)),
]
PW_PINS = [
    (16, 8, (3, 300, 293), ("pw_mfma<1,4>", 512, 1031)), (16, 32, (3, 300, 293), ("pw_mfma<2,4>", 512, 1031)),
    (24, 40, (3, 300, 293), ("pw_mfma<4,4>", 512, 1031)), (32, 64, (3, 300, 293), ("pw_mfma<4,4>", 512, 1031)),
    (64, 128, (3, 150, 293), ("pw_mfma<8,2>", 512, 1031)),
]
PW_WGRAD_PINS = [
    (8, 8, (3, 300, 293), ("pw_wgrad_mfma<1,64,1>", 1024, 4121)), (64, 32, (3, 300, 293), ("pw_wgrad_mfma<2,64,1>", 1024, 4121)),
    (64, 64, (3, 300, 293), ("pw_wgrad_mfma<4,64,1>", 512, 4121)), (128, 128, (3, 150, 293), ("pw_wgrad_mfma<4,64,4>", 256, 2061)),
]


def test_the_5x5_and_pointwise_tables_are_what_is_pinned_here():
    assert PCS.C5_PLANES == C5_PLANE_PINS and PCS.CONV5_CASES == CONV5_PINS and PCS.WGRAD5_CASES == WGRAD5_PINS
    assert PCS.PW_CASES == PW_PINS and PCS.PW_WGRAD_CASES == PW_WGRAD_PINS
    assert PCS.PW_RANDOM_CASE in PW_PINS and PCS.PW_WGRAD_RANDOM_CASE in PW_WGRAD_PINS and PCS.WGRAD5_RANDOM_CASE in WGRAD5_PINS
    assert set(PCS.CONV5_RANDOM_CASES) <= set(CONV5_PINS) and {c[0] for c in PCS.CONV5_RANDOM_CASES} == {"forward", "dgrad"}
    assert PCS.PW_REDUCE_NSPLIT == (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1024) and PCS.PW_REDUCE_PAIRS == ((8, 8), (24, 40))
    assert PCS.WGRAD5_REDUCE_NSPLIT == (1, 2, 255, 256) and PCS.WGRAD5_REDUCE_CLASSES == (1, 5, 8)
    assert PCS.PW_CAP8_PAIRS == ((64, 64), (128, 64), (128, 128))


def test_5x5_and_pointwise_multi_round_cases_loop_on_256_cus():
    """Every row of the four tables, on the 256-CU planning handle: the label and the (workgroups, work items) it pins, three rounds or
    more with a ragged last one, and the restated rules against the plan query where both exist (i[NPART] = the restated tile
    count, i[NSPLIT] = pw_restatement.wgrad_rows / min(tiles, CUs): asserted inside the *_rounds functions).  Every template instance of
    the four kernels has a case: conv5_kernel<8 / 16>, wgrad5_kernel<8 / 16> on both tiles, pw_kernel<1,4> <2,4> <4,4> <8,2>,
    pw_wgrad_kernel<1> <2> <4> (the default cap reaches no other)."""
    h = L.planner_handle(256)
    assert L.load().rcv_num_cus(h) == 256
    seen = set()
    for case in PCS.CONV5_CASES:
        for extra in (dict(), dict(flags=L.F_BIAS), dict(flags=L.F_RESID), dict(stats=L.STATS_FWD), dict(inmode=L.LOAD_AFFINE_RELU)):
            assert PCS.assert_multi_round(PCS.conv5_record(case, **extra), h, case[4]) == case[4][1:]
        seen.add(case[4][0])
    for case in PCS.WGRAD5_CASES:
        for extra in (dict(), dict(inmode=L.LOAD_AFFINE_RELU)):
            assert PCS.assert_multi_round(PCS.wgrad5_record(case, **extra), h, case[2]) == case[2][1:]
        seen.add(case[2][0])
    for case in PCS.PW_CASES:
        for form in PCS.PW_FORMS:
            assert PCS.assert_multi_round(PCS.pw_record(case, form), h, PCS.pw_pin(case, form)) == case[3][1:]
        seen.add(case[3][0])
    for case in PCS.PW_WGRAD_CASES:
        for modes in ((L.LOAD_PLAIN, L.LOAD_PLAIN), (L.LOAD_AFFINE_RELU, L.LOAD_GRAD_DEC)):
            assert PCS.assert_multi_round(PCS.pw_wgrad_record(case, *modes), h, case[3]) == case[3][1:]
        assert case[3][0] == PCS.pw_cap_label(case[0], case[1], 4)
        seen.add(case[3][0])
    assert {"conv5_mfma<%d,%s>" % (c, t) for c in (8, 16) for t in ("8x32", "16x16")} <= seen
    assert {"wgrad5_mfma<%d,%s>" % (c, t) for c in (8, 16) for t in ("8x32", "16x16")} <= seen
    assert {"pw_mfma<1,4>", "pw_mfma<2,4>", "pw_mfma<4,4>", "pw_mfma<8,2>"} <= seen
    assert {"pw_wgrad_mfma<%d,64,1>" % nb for nb in (1, 2, 4)} <= seen
    # the default cap reaches NB = 1, 2, 4 and no other, over every channel pair the kernels take
    assert {PCS.pw_cap_label(a, b, 4).split(",")[0] for a in range(8, 129, 8) for b in range(8, 129, 8)} == \
        {"pw_wgrad_mfma<%d" % nb for nb in (1, 2, 4)}
    # what the issue of these cases counted: 75 rounds of the 5x5 classifier at 32 x 480 x 640
    grid, tiles = PCS.conv5_rounds(L.make_op(L.OP_CONV5, 0, n=32, h=480, w=640, cin=16, cout=8, ho=480, wo=640, stride=1, dil=1), h)
    assert (grid, tiles) == (512, 38400)


def test_the_cap_of_eight_filter_blocks_per_wave_plans_as_restated():
    """i[AUX0] = 8 on RCV_OP_PW_WGRAD: the label of the plan query is the restated rule's, pw_wgrad_kernel<8> at 128 input channels;
    the rows do not depend on the cap."""
    h = L.planner_handle(256)
    for cin, cout in PCS.PW_CAP8_PAIRS + ((8, 8), (24, 40), (128, 8), (8, 128)):
        for cap in (0, 4, 8):
            op = L.make_op(L.OP_PW_WGRAD, 0, n=3, h=16, w=20, cin=cin, cout=cout, aux0=cap)
            L.op_workspace(h, op)
            assert PC.label_of(h, op) == PCS.pw_cap_label(cin, cout, cap or 4), (cin, cout, cap)
            assert op.i[L.RCV_I_NSPLIT] == 15
    assert [PCS.pw_cap_label(a, b, 8) for a, b in PCS.PW_CAP8_PAIRS] == ["pw_wgrad_mfma<4,64,1>", "pw_wgrad_mfma<8,64,1>", "pw_wgrad_mfma<8,64,2>"]
    with pytest.raises(L.RcvError, match="filter blocks per wave"):
        PC.label_of(h, L.make_op(L.OP_PW_WGRAD, 0, n=3, h=16, w=20, cin=64, cout=64, aux0=3))


# sources of kernel_case_records() that are the multi-round cases themselves
NEW_SOURCES = ("multi_round_fp64", "multi_round_stats_exact", "multi_round_stats_randn")


def test_rounds_of_the_earlier_cases():
    """What the multi-round cases are for: every other record of the kernel-level tests gives a workgroup of a persistent kernel
    exactly ONE tile (printed per family, pytest -s).  A case with several rounds that is added to one of the older tables belongs
    beside the multi-round cases, with its pin; this test then says so."""
    most = {}
    for test, op in PC.kernel_case_records():
        label = _planned_label(L.planner_handle(256), op)
        family = label.split("<")[0]
        if family in PERSISTENT and test not in NEW_SOURCES:
            grid, tiles = PC.rounds(op)
            most[family] = max(most.get(family, 0.0), tiles / grid)
    print("tiles per workgroup of the earlier cases:", {f: round(r, 2) for f, r in sorted(most.items())})
    assert most == {f: 1.0 for f in PERSISTENT}, most


