"""CPU: the calibration record (RCV_OP_CLS_CALIB) on the planner -- constant, symbol, queries and plan-time refusals --, the edges
``metrics.CalibrationState`` refuses, ``metrics.calibration_report`` against values worked out by hand and against the numpy
restatement (tests/calib_restatement.py), and the restatement's own rules: the hand-made case of the GPU test tells every wrong
variant of the rules apart."""
import math

import numpy as np
import pytest
import torch

import calib_restatement as R
import robocupvision_amd.model as M
from plan_census import label_of
from robocupvision_amd import _lib as L
from robocupvision_amd import metrics as MT

BASE = dict(n=3, h=5, w=7, cin=8, cout=5, inmode=0, count=16)


def test_constant_symbol_and_signature():
    assert L.OP_CLS_CALIB == 68 and L.CALIB_MAX_EDGES == 32 and L.CALIB_Q_SCALE == R.Q_SCALE == 2 ** 26
    assert "rcv_cls_calib" in L.EXPORTS and hasattr(L.load(), "rcv_cls_calib")
    assert len(L.load().rcv_cls_calib.argtypes) == 14          # handle, x, w, bias, five sizes, targets, edges, K, state, stream


def test_record_is_planned_on_the_planner():
    h = L.planner_handle()
    for cin, fused, form in ((8, False, 0), (8, True, 0), (16, False, 0), (16, True, 0), (8, False, 1), (1, False, 2), (0, False, 2)):
        for k in (1, 7, 32):
            op = L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP if fused else 0, n=3, h=5, w=7, cin=cin, cout=5, inmode=form, count=k,
                           aux0=L.LOAD_AFFINE_RELU, aux1=8)
            assert label_of(h, op) == "cls_calib" and L.op_workspace(h, op) == 0


@pytest.mark.parametrize("kw,word", [(dict(inmode=3), "source form"), (dict(inmode=-1), "source form"), (dict(n=0), "every size"),
                                     (dict(h=0), "every size"), (dict(w=-2), "every size"), (dict(n=70000, h=200, w=200), "2\\^31"),
                                     (dict(cout=0), "classes"), (dict(cout=9), "classes"), (dict(cin=12), "input channels"),
                                     (dict(inmode=1, cin=4), "floats per pixel"), (dict(inmode=1, cin=6), "floats per pixel"),
                                     (dict(count=0), "edges"), (dict(count=33), "edges"), (dict(count=-1), "edges")])
def test_plan_time_refusals(kw, word):
    with pytest.raises(L.RcvError, match=word):
        L.op_workspace(L.planner_handle(), L.make_op(L.OP_CLS_CALIB, 0, **{**BASE, **kw}))


def test_fused_refusals():
    h = L.planner_handle()
    with pytest.raises(L.RcvError, match="skip channels"):
        L.op_workspace(h, L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP, **{**BASE, "aux1": 6}))
    with pytest.raises(L.RcvError, match="skip load mode"):
        L.op_workspace(h, L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP, **{**BASE, "aux0": L.LOAD_NCHW}))
    for form in (1, 2):
        with pytest.raises(L.RcvError, match="RCV_F_FUSED_UP"):
            L.op_workspace(h, L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP, **{**BASE, "inmode": form}))


@pytest.mark.parametrize("edges", [(0.9, 0.5), (0.5, 0.5), (0.5, 0.5 + 1e-9), (0.1, float("nan")), (0.5, 1.5), (-0.1, 0.5), (float("inf"),), (),
                                   tuple(i / 33 for i in range(33)), "high", (0.5, None)],
                         ids=["unsorted", "equal", "equal_in_fp32", "nan", "above_1", "below_0", "inf", "none", "33", "text", "not_a_number"])
def test_state_refuses_bad_edges(edges):
    with pytest.raises(ValueError):
        MT.CalibrationState(5, edges)


def test_state_refuses_bad_classes_and_host_devices():
    for c in (0, 9, 2.0):
        with pytest.raises(ValueError):
            MT.CalibrationState(c, (0.5,))
    with pytest.raises(L.RcvError, match="HIP device"):
        MT.CalibrationState(5, (0.5, 0.9), device="cpu")
    e = MT.calibration_edges(tuple((i + 1) / 32 for i in range(32)))
    assert e.dtype == torch.float32 and e.numel() == 32
    assert MT.calibration_edges(MT.DEFAULT_CALIB_EDGES).numel() == len(MT.DEFAULT_CALIB_EDGES) <= 32
    assert MT.calibration_edges((0.0,)).tolist() == [0.0] and MT.calibration_edges((1.0,)).tolist() == [1.0]


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_report_by_hand():
    """C = 2, one edge at 0.5.  Class 1 is predicted for unlabelled pixels only.  Confidence sums: bin 0 holds 4 labelled pixels of
    confidence 0.25, bin 1 holds 8 of 0.875."""
    S = 2 ** 26
    tab = [[[3, 1, 2, 4 * S // 4, 2 * S // 8], [0, 0, 0, 0, 0]],
           [[6, 2, 1, 7 * S, 1 * S], [0, 0, 4, 0, 3 * S]]]
    r = MT.calibration_report(tab, (0.5,), 2)
    assert r["edges"] == [0.5] and r["labelled"] == 12 and r["unlabelled"] == 7
    assert r["kept"] == [[8, 0]] and r["correct"] == [[6, 0]] and r["kept_unlabelled"] == [[1, 4]]
    assert r["precision"][0][0] == 0.75 and math.isnan(r["precision"][0][1])
    assert r["coverage"][0][0] == 8 / 12 and math.isnan(r["coverage"][0][1])
    assert r["all"] == {"kept": [8], "correct": [6], "kept_unlabelled": [5], "precision": [0.75], "coverage": [8 / 12]}
    assert r["kept_confusion"].dtype == torch.int64 and r["kept_confusion"].tolist() == [[[6, 2], [0, 0]]]
    b = r["bins"]
    assert b["count"] == [4, 8] and b["accuracy"] == [0.75, 0.75] and b["mean_confidence"] == [0.25, 0.875]
    assert b["lo"] == [float("-inf"), 0.5] and b["hi"] == [0.5, float("inf")]
    assert b["per_class"]["count"] == [[4, 0], [8, 0]] and b["per_class"]["accuracy"][1][0] == 0.75
    assert math.isnan(b["per_class"]["accuracy"][0][1]) and math.isnan(b["per_class"]["mean_confidence"][1][1])
    assert b["per_class"]["mean_confidence"][0][0] == 0.25
    # ECE on the two bins: 4/12 * |0.75 - 0.25| + 8/12 * |0.75 - 0.875| = 1/6 + 1/12
    assert r["ece"] == 4 / 12 * 0.5 + 8 / 12 * 0.125 and abs(r["ece"] - 0.25) < 1e-15
    assert r.threshold(0.75) == 0.5 and r.threshold(0.75, cls=0) == 0.5
    assert r.threshold(0.8) is None and r.threshold(0.1, cls=1) is None


def test_report_thresholds_and_empty_bins():
    """C = 1, three edges: precision is 1 wherever something is kept; an empty top bin keeps nothing (0 / 0) and adds nothing to ECE."""
    S = 2 ** 26
    tab = [[[5, 0, S, 0]], [[0, 3, 0, S]], [[2, 0, S, 0]], [[0, 0, 0, 0]]]
    r = MT.calibration_report(tab, (0.25, 0.5, 0.75), 1)
    assert r["kept"] == [[2], [2], [0]] and r["all"]["coverage"] == [2 / 7, 2 / 7, 0.0] and r["kept_unlabelled"] == [[3], [0], [0]]
    assert r["precision"][0] == [1.0] and math.isnan(r["precision"][2][0]) and r.threshold(1.0) == 0.25 and r.threshold(1.0, 0) == 0.25
    assert r["bins"]["count"] == [5, 0, 2, 0] and math.isnan(r["bins"]["accuracy"][1]) and math.isnan(r["bins"]["mean_confidence"][3])
    assert r["ece"] == 5 / 7 * abs(1.0 - 0.2) + 2 / 7 * abs(1.0 - 0.5)
    empty = MT.calibration_report([[[0] * 4], [[0] * 4]], (0.5,), 1)
    assert math.isnan(empty["ece"]) and empty.threshold(0.0) is None and empty["labelled"] == 0
    with pytest.raises(ValueError):
        MT.calibration_report(tab, (0.5,), 1)


def test_report_is_the_restatement():
    cls, conf, t = R.handmade_maps((3, 5, 7), 5)
    for edges in (R.HAND_EDGES, np.array([0.5], np.float32), np.linspace(0.03, 0.99, 32).astype(np.float32)):
        tab = R.table(cls, conf, t, edges, 5)
        want, got = R.report(tab, edges), MT.calibration_report(tab.tolist(), edges.tolist(), 5)
        for key in ("kept", "correct", "kept_unlabelled", "precision", "coverage"):
            assert _same(got[key], want[key]) and _same(got["all"][key], want["all_" + key]), key
        assert np.array_equal(got["kept_confusion"].numpy(), want["kept_confusion"])
        for key in ("count", "accuracy", "mean_confidence"):
            assert _same(got["bins"][key], want["bin_" + key]) and _same(got["bins"]["per_class"][key], want["class_bin_" + key]), key
        assert abs(got["ece"] - want["ece"]) <= 8 * 2.0 ** -53 and (got["labelled"], got["unlabelled"]) == (want["labelled"], want["unlabelled"])
        for target in (0.0, 0.5, 0.66, 0.9, 1.0):
            for c in (None, 0, 4):
                assert got.threshold(target, c) == R.threshold(want, edges, target, c)


def test_table_by_hand():
    """Six pixels, C = 2, one edge at 0.5: on the edge, one ulp below it, unlabelled at 1, a NaN, a class byte >= C, and 2^32 + 1."""
    below = np.nextafter(np.float32(0.5), np.float32(0))
    cls = np.array([0, 0, 1, 1, 2, 1], np.uint8)
    conf = np.array([0.5, below, 1.0, np.nan, 0.9, 0.1], np.float32)
    t = np.array([0, 1, -100, 1, 0, 2 ** 32 + 1], np.int64)
    want = np.zeros((2, 2, 5), np.int64)
    want[1, 0, 0] += 1; want[1, 0, 3] += 2 ** 25                    # 0.5 >= 0.5
    want[0, 0, 1] += 1; want[0, 0, 3] += 2 ** 25 - 2                # (0.5 - 2^-25) * 2^26
    want[1, 1, 2] += 1; want[1, 1, 4] += 2 ** 26
    want[0, 1, 2] += 1; want[0, 1, 4] += 6710886                    # fp32(0.1) * 2^26 = 6710886.5, truncated
    assert np.array_equal(R.table(cls, conf, t, np.array([0.5], np.float32), 2), want)
    none = R.table(cls, conf, None, np.array([0.5], np.float32), 2)
    assert none[:, :, :2].sum() == 0 and none[:, :, 3].sum() == 0 and none[:, :, 2].sum() == 4
    assert none[:, :, 4].sum() == want[:, :, 3:].sum()


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_handmade_case_tells_wrong_rules_apart(variant):
    """The maps the GPU test runs (small plane, C = 5, HAND_EDGES): each wrong rule gives another table."""
    cls, conf, t = R.handmade_maps((3, 5, 7), 5)
    right = R.table(cls, conf, t, R.HAND_EDGES, 5)
    assert right.sum() > 0 and not np.array_equal(R.table(cls, conf, t, R.HAND_EDGES, 5, variant), right)


def test_handmade_case_holds_what_it_promises():
    cls, conf, t = R.handmade_maps((3, 5, 7), 5)
    flat = conf.reshape(-1)
    for e in R.HAND_EDGES:
        assert (flat == e).any() and (e == 0 or (flat == np.nextafter(e, np.float32(-1))).any())
    assert np.isnan(flat).any() and (cls >= 5).any() and all((t == v).any() for v in (-100, 5, 2 ** 32, 2 ** 32 + 4))
    assert flat[~np.isnan(flat)].min() >= 0.0 and flat[~np.isnan(flat)].max() <= 1.0
    assert set(R.bin_index(flat, R.HAND_EDGES).tolist()) == set(range(6))


def test_calibrate_refusals_without_a_device():
    x = torch.zeros(1, 3, 48, 64)
    net = M.ROBO_UNet()
    for cls in (M.ROBO_UNet, M.PB_FCN, M.PB_FCN_2, M.LabelProp, M.FCN):
        assert callable(getattr(cls, "calibrate"))
    with pytest.raises(L.RcvError, match=r"call `\.eval\(\)` first"):
        net.calibrate(x, None)
    with pytest.raises(L.RcvError, match="HIP device only"):
        net.eval().calibrate(x, None)
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN_2(True).eval().calibrate(x, None)
    with pytest.raises(L.RcvError, match="no per-pixel classifier"):
        M.Conv(8, 8, 3).eval().calibrate(torch.zeros(1, 8, 8, 8), None)
    with pytest.raises(TypeError):
        net.calibrate(None, None)


def test_calib_plan_ends_in_the_record():
    from robocupvision_amd.engine import Engine
    for net in (M.ROBO_UNet(), M.PB_FCN(32, 5, 5, False, 0)):
        eng = Engine(net._graph(), list(net.parameters()), M._bn_modules(net), dry_run=True)
        x = [torch.zeros(1, 3, 48, 64)]
        plan = eng._plan_for(x, False, labels="calib")
        assert plan.fwd.labels(eng.handle)[-1] == "cls_calib" and plan.label_op == plan.fwd.n - 1 and plan.label_classes == 5
        assert plan is eng._plan_for(x, False, labels="calib") and plan is not eng._plan_for(x, False, labels="proba")
        assert plan is not eng._plan_for(x, False) and plan is not eng._plan_for(x, False, labels=True)
    net = M.PB_FCN_2(True)
    eng = Engine(net._graph(), list(net.parameters()), M._bn_modules(net), dry_run=True)
    with pytest.raises(L.RcvError, match="pool_cls"):
        eng._plan_for([torch.zeros(1, 3, 48, 64)], False, labels="calib")
