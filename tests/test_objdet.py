"""CPU: the object-detection contract of RCV_OP_OBJECT_MATCH (test.py:28-89) -- two independent restatements agree, hand-computed
known answers, the host float64 arithmetic of DetectionMetrics, and the C ABI's plan-time refusals on a planning-only handle."""
import ctypes
import math

import numpy as np
import pytest
import torch

import objdet_restatement as R
from robocupvision_amd import _lib as L
from robocupvision_amd import metrics as M


def _plane(H, W, pixels, value=1):
    a = np.zeros((H, W), dtype=np.int64)
    for y, x in pixels:
        a[y, x] = value
    return a


def _box(H, W, y0, y1, x0, x1, value=1):
    a = np.zeros((H, W), dtype=np.int64)
    a[y0:y1 + 1, x0:x1 + 1] = value
    return a


# (name, pred [N,H,W], target [N,H,W], C, iou thresholds, distance thresholds, expected counts [N][C-1][2+2K])
KNOWN_ANSWERS = [
    # A at (y=1,x=0) is in block 0, B at (0,4) in block 2: block order A, B; raster order B, A.  T1 (0,2) is within 2.5 of both
    # (A: sqrt(5), B: 2), T2 (3,0) only of A (2).  Block order: A takes T1, B finds nothing -> 1.  Raster order would give 2.
    ("block_order", _plane(4, 6, [(1, 0), (0, 4)])[None], _plane(4, 6, [(0, 2), (3, 0)])[None], 2, [0.5], [2.5],
     [[[2, 2, 0, 1]]]),
    # IoU exactly 0.5 (inter 1, union 2) does not pass t=0.5, passes 0.25
    ("iou_half", _plane(3, 4, [(1, 1), (1, 2)])[None], _plane(3, 4, [(1, 1)])[None], 2, [0.5, 0.25], [0.0, 0.0],
     [[[1, 1, 0, 1, 0, 0]]]),
    # 1/10 == 0.1 in fp64: does not pass t=0.1, passes 0.0999
    ("iou_tenth", _plane(2, 12, [(0, 3)])[None], _box(2, 12, 0, 0, 1, 10)[None], 2, [0.1, 0.0999], [0.0, 0.0],
     [[[1, 1, 0, 1, 0, 0]]]),
    # centre offset (3, 4): distance exactly 5 does not pass d=5, passes 5.000001; t=1 matches nothing
    ("dist_345", _plane(6, 6, [(0, 0)])[None], _plane(6, 6, [(4, 3)])[None], 2, [1.0, 1.0], [5.0, 5.000001],
     [[[1, 1, 0, 0, 0, 1]]]),
    # a diagonal chain is one 8-connected component; the target is its bounding box (IoU 5/25)
    ("diagonal", _plane(5, 5, [(i, i) for i in range(5)])[None], _box(5, 5, 0, 4, 0, 4)[None], 2, [0.19, 0.2], [0.5, 0.5],
     [[[1, 1, 1, 0, 1, 1]]]),
    # empty pred / empty target / both empty (per image)
    ("empty", np.stack([np.zeros((3, 3), np.int64), _plane(3, 3, [(1, 1)]), np.zeros((3, 3), np.int64)]),
     np.stack([_plane(3, 3, [(0, 0)]), np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)]), 2, [0.5], [9.0],
     [[[0, 1, 0, 0]], [[1, 0, 0, 0]], [[0, 0, 0, 0]]]),
    # P1 (block 0) overlaps only T1 and claims it; P2 overlaps T1 and T2, T1 is used: P2 takes T2
    ("claimed", (_box(4, 12, 0, 1, 0, 1) + _box(4, 12, 0, 1, 4, 9))[None],
     (_box(4, 12, 0, 1, 0, 5) + _box(4, 12, 0, 1, 8, 11))[None], 2, [0.05], [0.0],
     [[[2, 2, 2, 0]]]),
    # target values >= C and < 0 are in no class; pred values >= C too
    ("out_of_range", np.array([[[1, 0, 3, 0], [0, 0, 0, 0], [2, 0, 7, 0]]]), np.array([[[1, 0, -3, 0], [0, 0, 0, 0], [9, 0, 2, 0]]]), 3,
     [0.5], [100.0], [[[1, 1, 1, 1], [1, 1, 0, 1]]]),
]


@pytest.mark.parametrize("case", KNOWN_ANSWERS, ids=[c[0] for c in KNOWN_ANSWERS])
def test_known_answers_both_restatements(case):
    _, pred, target, C, it, dt, expected = case
    expected = np.array(expected)
    assert np.array_equal(R.literal(pred, target, C, it, dt), expected)
    assert np.array_equal(R.fast(pred, target, C, it, dt), expected)


def test_block_order_differs_from_raster_order():
    """The order convention matters: with the preds taken in pixel-raster order the greedy distance count of 'block_order' is 2."""
    _, pred, target, C, it, dt, expected = KNOWN_ANSWERS[0]
    assert R.fast(pred, target, C, it, dt)[0, 0, 3] == 1
    swapped = np.zeros_like(pred)          # mirror left-right: B's block now precedes A's, as raster order would have them
    swapped[0] = pred[0][:, ::-1]
    assert R.fast(swapped, target[:, :, ::-1], C, it, dt)[0, 0, 3] == 2


def test_restatements_agree_on_random_planes():
    rng = np.random.default_rng(1234)
    sizes = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (4, 4), (5, 9), (8, 8), (9, 11), (13, 17), (12, 16), (11, 2)]
    n = 0
    for rep in range(25):
        for H, W in sizes:
            C = int(rng.integers(2, 6))
            K = int(rng.integers(1, 4))
            it = [float(v) for v in rng.choice([0.0, 0.05, 0.1, 0.25, 1 / 3, 0.5, 0.75, 1.0], size=K)]
            dt = [float(v) for v in rng.choice([0.0, 0.5, 1.0, 1.25, 2.5, 5.0, math.sqrt(2)], size=K)]
            dens = rng.choice([0.1, 0.3, 0.6, 0.9])
            pred = np.where(rng.random((2, H, W)) < dens, rng.integers(1, C, (2, H, W)), 0)
            target = np.where(rng.random((2, H, W)) < dens, rng.integers(1, C, (2, H, W)), 0)
            if rep % 3 == 0:
                target = np.where(rng.random((2, H, W)) < 0.8, pred, target)
            a, b = R.literal(pred, target, C, it, dt), R.fast(pred, target, C, it, dt)
            assert np.array_equal(a, b), (H, W, C, it, dt)
            assert R.scores([a], C, K) == M.detection_scores([b], C, K)
            n += 1
    assert n == 300


def test_batch_grouping_matches_the_formula():
    """update(B=3) then update(B=2): one batch value per update, summed in float64 (test.py:258-262), against a hand-written sum."""
    rng = np.random.default_rng(5)
    C, K = 4, 2
    it, dt = [0.5, 0.1], [2.5, 10.0]
    b1 = R.fast(R.blob_masks(rng, 3, 20, 24, C, 5), R.blob_masks(rng, 3, 20, 24, C, 5), C, it, dt)
    b2 = R.fast(R.blob_masks(rng, 2, 20, 24, C, 5), R.blob_masks(rng, 2, 20, 24, C, 5), C, it, dt)
    got = M.detection_scores([b1, b2], C, K)
    for crit in (0, 1):
        for k in range(K):
            total = 0.0
            for cnt in (b1, b2):
                p = r = 0.0
                for c in range(C - 1):
                    for b in range(cnt.shape[0]):
                        nP, nT, nc = int(cnt[b, c, 0]), int(cnt[b, c, 1]), int(cnt[b, c, 2 + crit * K + k])
                        p += nc / nP if nP else 1.0
                        r += nc / nT if nT else 1.0
                total += (p / (C - 1) + r / (C - 1)) / 2
            assert got[crit][k] == total
    assert got != M.detection_scores([np.concatenate([b1, b2])], C, K)     # grouping changes the numbers: it is part of the contract


def test_empty_planes_contribute_one():
    cnt = np.zeros((2, 3, 4), dtype=np.int64)        # no blobs anywhere: every prec and recall term is 1, summed over 2 images
    assert M.detection_scores([cnt], 4, 1) == [[2.0], [2.0]]     # (compute() divides by the image count: 1.0)


def _record(N=2, H=30, W=40, C=5, it=(0.5,), dt=(2.5,), pb=1, tb=8):
    return M.ObjectMatchRecord(N, H, W, C, it, dt, pb, tb)


def test_workspace_query_on_planner_handle():
    h = L.planner_handle(256)
    small, big = _record(2, 30, 40).workspace_bytes(h), _record(4, 60, 80).workspace_bytes(h)
    assert 0 < small < big
    assert _record(2, 31, 41).workspace_bytes(h) >= small
    assert _record(1, 480, 640).workspace_bytes(h) > 0
    rec = _record()
    rec.workspace_bytes(h)
    assert rec.op.i[L.RCV_I_NPART] * 256 == rec.workspace_bytes(h)
    assert L.OpList([rec.op]).labels(h)[0] == "object_match<u8,i64>"
    with pytest.raises(L.RcvError, match="planning-only"):
        L.OpList([rec.op]).run(h, 0)
    it, dt = ctypes.c_double(0.5), ctypes.c_double(2.5)
    lib = L.load()
    rc = lib.rcv_object_match(h, None, 1, None, 8, 1, 5, 4, 4, ctypes.byref(it), ctypes.byref(dt), 1, None, None, 1 << 20, None)
    assert rc != 0 and b"planning-only" in lib.rcv_last_error()


@pytest.mark.parametrize("kw", [dict(C=1), dict(C=9), dict(it=(), dt=()), dict(it=(0.5,) * 9, dt=(1.0,) * 9), dict(it=(-0.01,)),
                                dict(it=(float("nan"),)), dict(it=(float("inf"),)), dict(dt=(float("nan"),)),
                                dict(dt=(float("inf"),)), dict(dt=(-float("inf"),)), dict(pb=4), dict(tb=2), dict(N=0), dict(W=0)],
                         ids=["C1", "C9", "K0", "K9", "t_neg", "t_nan", "t_inf", "d_nan", "d_inf", "d_minf", "pred_i32", "target_i16",
                              "N0", "W0"])
def test_refusals(kw):
    with pytest.raises(L.RcvError):
        _record(**kw).workspace_bytes(L.planner_handle(256))


def test_edge_thresholds_are_accepted():
    h = L.planner_handle(256)
    assert _record(it=(1.0,), dt=(0.0,)).workspace_bytes(h) > 0
    assert _record(it=(0.0, 7.5), dt=(-3.0, 1e300)).workspace_bytes(h) > 0
    assert _record(C=2).workspace_bytes(h) > 0 and _record(C=8, it=(0.5,) * 8, dt=(1.0,) * 8).workspace_bytes(h) > 0


def test_detection_metrics_refuses_cpu_tensors_and_bad_arguments():
    m = M.DetectionMetrics(5)
    with pytest.raises(L.RcvError):
        m.update(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.int64))
    with pytest.raises(L.RcvError):
        M.object_match_counts(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.int64), 5)
    with pytest.raises(L.RcvError):
        M.DetectionMetrics(1)
    with pytest.raises(L.RcvError):
        M.DetectionMetrics(5, iou_thresholds=(0.5, -1.0), dist_thresholds=(1.0, 2.0))
    with pytest.raises(L.RcvError):
        M.DetectionMetrics(5, iou_thresholds=(0.5,), dist_thresholds=(1.0, 2.0))
