"""CPU: the contract of RCV_OP_OBJECTS (rcv_find_objects) -- the numpy restatement against scipy's labelling, hand-written
known answers (imported by test_gpu_objects.py), the C ABI's workspace query, labels and refusals on a planning-only handle, and the
Python surface's refusals."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import objdet_restatement as R
import objects_restatement as OR
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import metrics as M


def _plane(H, W, pixels=(), boxes=(), value=1):
    a = np.zeros((H, W), dtype=np.int64)
    for y, x in pixels:
        a[y, x] = value
    for y0, y1, x0, x1 in boxes:
        a[y0:y1 + 1, x0:x1 + 1] = value
    return a


# ------------------------------------------------------------------------------------------------------- (a) restatement vs scipy
def _scipy_components(plane, c):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(plane == c, structure=np.ones((3, 3)))
    out = []
    for k, sl in enumerate(ndi.find_objects(lab)):
        ys, xs = sl
        out.append((xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start, int((lab[sl] == k + 1).sum())))
    return out


BLOB_SHAPES = [(3, 37, 53), (2, 120, 160), (1, 5, 7)]


@pytest.mark.parametrize("shape", BLOB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_scipy_label(shape):
    pytest.importorskip("scipy")
    N, H, W = shape
    C = 5
    rng = np.random.default_rng(100 + H)
    blobs = R.blob_masks(rng, N, H, W, C)
    for maps, cap in ((blobs, 2), (blobs, 1), (R.jitter(rng, blobs, C, p=0.02), 6)):
        rows, counts = OR.find_objects(maps, C, 0, 0.0, cap)
        for n in range(N):
            for c in range(1, C):
                ref = _scipy_components(maps[n], c)
                mine = OR.components(maps[n], c)
                assert collections.Counter(mine) == collections.Counter(ref)          # multisets of (box, area)
                for k, comp in enumerate(mine):                                       # _rect itself, where the plane is small
                    if H * W <= 2000:
                        lab, _ = R._label(maps[n] == c)
                        assert comp[:4] == R._rect(lab == k) and comp[4] == int((lab == k).sum())
                emitted = int(counts[n, c - 1, 3])
                assert counts[n, c - 1].tolist() == [len(ref), len(ref), len(ref), min(len(ref), cap)]
                areas = sorted((r[4] for r in ref), reverse=True)
                assert rows[n, c - 1, :emitted, 4].tolist() == areas[:cap]            # the cap keeps the largest
                assert (rows[n, c - 1, emitted:] == 0).all()
                for r in rows[n, c - 1, :emitted].tolist():
                    assert tuple(r[:5]) in ref and r[6:] == [2 * r[0] + r[2], 2 * r[1] + r[3]]
                    assert mine[r[5]] == tuple(r[:5])                                 # rank indexes the component list


def test_jittered_maps_exceed_the_cap():
    """The cap is exercised: a jittered 120x160 map has more components of a class than 6."""
    rng = np.random.default_rng(7)
    maps = R.jitter(rng, R.blob_masks(rng, 1, 120, 160, 5), 5, p=0.02)
    _, counts = OR.find_objects(maps, 5, 0, 0.0, 6)
    assert (counts[0, :, 0] > 6).all() and (counts[0, :, 3] == 6).all()


# ------------------------------------------------------------------------------------------------------------ (b) known answers
_THREE = _plane(4, 8, [(0, 0), (0, 4), (3, 2)])            # blocks 0, 2, 5 (Wb = 4): ranks 0, 1, 2, all of area 1
_FOUR = _plane(4, 8, [(0, 0), (0, 4), (3, 2), (3, 6)])     # and block 7: rank 3
_R0, _R1, _R2 = [0, 0, 1, 1, 1, 0, 1, 1], [4, 0, 1, 1, 1, 1, 9, 1], [2, 3, 1, 1, 1, 2, 5, 7]
_Z = [0] * 8
_RATIO = _plane(5, 12, [(4, 11)], [(0, 1, 0, 9)])          # a 2x10 box (area 20, rank 0) and one pixel (rank 1)
_SORT = _plane(4, 8, [(0, 0)], [(0, 1, 4, 5), (3, 3, 0, 1)])      # areas 1, 4, 2 at ranks 0, 1, 2

# (name, maps [N,H,W], C, min_area, min_ratio, max_objects, expected rows [N][C-1][M][8], expected counts [N][C-1][4])
KNOWN_ANSWERS = [
    # equal areas: the order of emission is the rank; the cap keeps the lowest ranks
    ("ties_by_rank", _THREE[None], 2, 0, 0.0, 2, [[[_R0, _R1]]], [[[3, 3, 3, 2]]]),
    # exactly cap, cap + 1 and 0 components
    ("cap_exact_plus_one_none", np.stack([_THREE, _FOUR, _plane(4, 8)]), 2, 0, 0.0, 3,
     [[[_R0, _R1, _R2]], [[_R0, _R1, _R2]], [[_Z, _Z, _Z]]], [[[3, 3, 3, 3]], [[4, 4, 4, 3]], [[0, 0, 0, 0]]]),
    # area descending first, rank second; the strict min_area drops the area-1 pixel in the second entry
    ("sorted_by_area", _SORT[None], 2, 0, 0.0, 3,
     [[[[4, 0, 2, 2, 4, 1, 10, 2], [0, 3, 2, 1, 2, 2, 2, 7], [0, 0, 1, 1, 1, 0, 1, 1]]]], [[[3, 3, 3, 3]]]),
    ("min_area_is_strict", _SORT[None], 2, 1, 0.0, 3,
     [[[[4, 0, 2, 2, 4, 1, 10, 2], [0, 3, 2, 1, 2, 2, 2, 7], _Z]]], [[[3, 2, 2, 2]]]),
    # amax is taken over A: the only candidate for it (area 4 = min_area) is dropped by the strict compare, so amax = 0, A and Q are
    # empty; with min_area 2 the area-2 blob sets nothing either: amax = 4 over A = {4}, and 2 is not in A whatever the ratio
    ("amax_over_A", np.stack([_SORT, _SORT]), 2, 4, 1.0, 3, [[[_Z, _Z, _Z]], [[_Z, _Z, _Z]]], [[[3, 0, 0, 0]], [[3, 0, 0, 0]]]),
    ("amax_over_A_2", _SORT[None], 2, 2, 0.5, 3, [[[[4, 0, 2, 2, 4, 1, 10, 2], _Z, _Z]]], [[[3, 1, 1, 1]]]),
    # min_ratio exactly met: 20 * 0.05 == 1.0 in fp64, and 1.0 >= 1.0
    ("ratio_exactly_met", _RATIO[None], 2, 0, 0.05, 2, [[[[0, 0, 10, 2, 20, 0, 10, 2], [11, 4, 1, 1, 1, 1, 23, 9]]]], [[[2, 2, 2, 2]]]),
    ("ratio_just_missed", _RATIO[None], 2, 0, 0.05000001, 2, [[[[0, 0, 10, 2, 20, 0, 10, 2], _Z]]], [[[2, 2, 1, 1]]]),
    # cap = 0 for class 1 (M is the maximum of the caps, 1): counted, not emitted
    ("cap_zero", (_plane(3, 6, [(0, 0)]) + _plane(3, 6, [(2, 4)], value=2))[None], 3, 0, 0.0, (0, 1),
     [[[_Z], [[4, 2, 1, 1, 1, 0, 9, 5]]]], [[[1, 1, 1, 0], [1, 1, 1, 1]]]),
    # 0, C and 255 are background: the 3 between the two 1s does not join them
    ("background_values", np.array([[[1, 3, 1, 255, 2]]]), 3, 0, 0.0, 2,
     [[[[0, 0, 1, 1, 1, 0, 1, 1], [2, 0, 1, 1, 1, 1, 5, 1]], [[4, 0, 1, 1, 1, 0, 9, 1], _Z]]], [[[2, 2, 2, 2], [1, 1, 1, 1]]]),
    # test_objdet.py's block-order plane: A (y=1, x=0) is in block 0, B (0, 4) in block 2 -> ranks A = 0, B = 1 (raster order: B first)
    ("block_order", _plane(4, 6, [(1, 0), (0, 4)])[None], 2, 0, 0.0, 2,
     [[[[0, 1, 1, 1, 1, 0, 1, 3], [4, 0, 1, 1, 1, 1, 9, 1]]]], [[[2, 2, 2, 2]]]),
]


@pytest.mark.parametrize("case", KNOWN_ANSWERS, ids=[c[0] for c in KNOWN_ANSWERS])
def test_known_answers_restatement(case):
    _, maps, C, min_area, min_ratio, cap, rows, counts = case
    got_rows, got_counts = OR.find_objects(maps, C, min_area, min_ratio, cap)
    assert got_rows.tolist() == rows
    assert got_counts.tolist() == counts


def test_block_order_is_not_raster_order():
    """The block-order plane mirrored left-right: B's block now precedes A's, so the ranks swap with the emission order."""
    _, maps, C, *_ = KNOWN_ANSWERS[-1]
    rows, _ = OR.find_objects(maps[:, :, ::-1], C, 0, 0.0, 2)
    assert rows[0, 0, :, :2].tolist() == [[1, 0], [5, 1]] and rows[0, 0, :, 5].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------ (c) the C ABI, planner handle
ROUTE_LDS_MIN_N = 64         # batches from this size on take the single-launch kernel when the plane fits

def _record(N=2, H=30, W=40, C=5, min_area=0, min_ratio=0.0, max_objects=8, eb=1, form=0):
    return I.ObjectsRecord(N, H, W, C, min_area, min_ratio, max_objects, eb, form)


def test_workspace_query_on_planner_handle():
    h = L.planner_handle(256)
    small, big = _record(2, 30, 40).workspace_bytes(h), _record(4, 60, 80).workspace_bytes(h)
    assert 0 < small < big
    assert _record(2, 31, 41).workspace_bytes(h) >= small
    assert _record(1, 480, 640).workspace_bytes(h) > 0
    for N, H, W in ((2, 30, 40), (64, 120, 160), (1, 480, 640)):      # one set of planes, no pair hash, no candidate lists
        assert _record(N, H, W).workspace_bytes(h) < M.ObjectMatchRecord(N, H, W, 5, (0.5,), (2.5,)).workspace_bytes(h)
    rec = _record()
    rec.workspace_bytes(h)
    assert rec.op.i[L.RCV_I_NPART] * 256 == rec.workspace_bytes(h)
    assert rec.workspace_bytes(h) == _record(form=1).workspace_bytes(h) == _record(form=2).workspace_bytes(h)
    with pytest.raises(L.RcvError, match="planning-only"):
        L.OpList([rec.op]).run(h, 0)


def test_kernel_labels_show_the_route():
    h = L.planner_handle(256)

    def label(**kw):
        return L.OpList([_record(**kw).op]).labels(h)[0]
    assert label(form=1) == "objects<u8>" and label(form=2) == "objects<u8,lds>"
    assert label(form=1, eb=8) == "objects<i64>" and label(form=2, eb=8) == "objects<i64,lds>"
    # the route depends on the shape alone: planes up to 7680 2x2 blocks in batches of ROUTE_LDS_MIN_N or more take the LDS kernel
    assert label(N=ROUTE_LDS_MIN_N, H=120, W=160) == "objects<u8,lds>" and label(N=4 * ROUTE_LDS_MIN_N, H=120, W=160, eb=8) == "objects<i64,lds>"
    assert label(N=ROUTE_LDS_MIN_N - 1, H=120, W=160) == "objects<u8>" and label(N=1, H=120, W=160) == "objects<u8>"
    assert label(N=ROUTE_LDS_MIN_N, H=120, W=256) == "objects<u8,lds>" and label(N=ROUTE_LDS_MIN_N, H=122, W=256) == "objects<u8>"
    assert label(N=ROUTE_LDS_MIN_N, H=480, W=640) == "objects<u8>"


REFUSALS = {
    "C1": dict(C=1), "C9": dict(C=9), "M0": dict(max_objects=0), "M17": dict(max_objects=17),
    "cap_above_M": dict(max_objects=(2, 3, 4, 17)), "cap_negative": dict(max_objects=(2, -1, 2, 2)),
    "min_area_negative": dict(min_area=(0, 0, -1, 0)), "ratio_nan": dict(min_ratio=float("nan")), "ratio_inf": dict(min_ratio=float("inf")),
    "ratio_negative": dict(min_ratio=(0.0, -0.01, 0.0, 0.0)), "ratio_above_one": dict(min_ratio=1.0000001),
    "elem_i32": dict(eb=4), "elem_i16": dict(eb=2), "N0": dict(N=0), "H0": dict(H=0), "W0": dict(W=0), "N_negative": dict(N=-1),
    "plane_too_large": dict(N=1, H=1024, W=1026), "plane_too_tall": dict(N=1, H=8193, W=2), "batch_too_large": dict(N=32768, H=2, W=2),
    "ids_overflow": dict(N=8192, H=512, W=1024), "lds_form_does_not_fit": dict(N=1, H=122, W=256, form=2), "form_unknown": dict(form=3),
}


@pytest.mark.parametrize("kw", list(REFUSALS.values()), ids=list(REFUSALS))
def test_refusals_at_query_and_at_launch(kw):
    h = L.planner_handle(256)
    rec = _record(**kw)
    with pytest.raises(L.RcvError) as at_query:
        rec.workspace_bytes(h)
    assert "planning-only" not in str(at_query.value)
    buf = ctypes.create_string_buffer(64)
    assert L.load().rcv_op_kernel_label(h, ctypes.byref(rec.op), buf, 64) != 0


def test_cap_above_M_is_refused_at_the_record():
    """ObjectsRecord makes M the maximum of the caps, so a cap above M only reaches the library through a hand-made record."""
    h = L.planner_handle(256)
    rec = _record(max_objects=(1, 2, 3, 4))
    assert rec.M == 4 and rec.workspace_bytes(h) > 0
    rec.op.i[L.RCV_I_COUNT] = 3
    with pytest.raises(L.RcvError, match="cap of class 4"):
        rec.workspace_bytes(h)
    rec.op.i[L.RCV_I_COUNT] = 4
    rec.op.p[L.RCV_P_X1] = None
    with pytest.raises(L.RcvError, match="per-class rules"):
        rec.workspace_bytes(h)


def test_edge_rules_are_accepted():
    h = L.planner_handle(256)
    assert _record(min_ratio=1.0, max_objects=16).workspace_bytes(h) > 0
    assert _record(min_ratio=0.0, max_objects=1, min_area=(1 << 31) - 1).workspace_bytes(h) > 0
    assert _record(C=2).workspace_bytes(h) > 0 and _record(C=8, max_objects=(0,) * 7).workspace_bytes(h) > 0
    assert _record(N=1, H=512, W=1024).workspace_bytes(h) > 0 and _record(N=32767, H=1, W=1).workspace_bytes(h) > 0
    assert I.ObjectsRecord(1, 8, 8, **I.DBCONVERT).M == 6


# ---------------------------------------------------------------------------------------------------------- (d) the Python surface
def test_find_objects_refuses_cpu_tensors_and_bad_arguments():
    cpu = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(L.RcvError, match="HIP device"):
        I.find_objects(cpu)
    with pytest.raises(L.RcvError, match="HIP device"):
        robocupvision_amd.find_objects(cpu.long(), **robocupvision_amd.DBCONVERT)
    for bad in (dict(num_class=1), dict(num_class=9), dict(max_objects=17), dict(max_objects=0), dict(min_area=-1),
                dict(min_ratio=1.5), dict(min_ratio=float("nan")), dict(max_objects=(1, 2, 3, 17))):
        with pytest.raises(L.RcvError) as e:
            I.find_objects(cpu, **bad)
        assert "HIP device" not in str(e.value), bad                 # refused for the argument, with the library's message
    for bad in (dict(min_area=(1, 2, 3)), dict(min_ratio=(0.1,) * 5), dict(max_objects=(1, 2)), dict(min_area=1.5),
                dict(max_objects="many"), dict(num_class=5.5), dict(min_ratio=("a", 0, 0, 0))):
        with pytest.raises(L.RcvError) as e:
            I.find_objects(cpu, **bad)
        assert "HIP device" not in str(e.value), bad
    with pytest.raises(L.RcvError, match="dtype"):
        I.find_objects(cpu.to(torch.int32))
    with pytest.raises(L.RcvError, match=r"\[N,H,W\]"):
        I.find_objects(cpu[0])


def test_segmenter_objects_argument():
    import robocupvision_amd.model as Mo
    net = Mo.ROBO_UNet()
    seg = robocupvision_amd.Segmenter(net, objects=I.DBCONVERT)
    assert seg._objects == dict(I.DBCONVERT) and robocupvision_amd.Segmenter(net)._objects is None
    for bad in (dict(min_area=-1), dict(max_objects=17), dict(min_ratio=2.0), dict(min_area=(1, 2)), dict(colour=True), [("min_area", 1)]):
        with pytest.raises(L.RcvError):
            robocupvision_amd.Segmenter(net, objects=bad)
    frames = torch.zeros(1, 24, 32, 3, dtype=torch.uint8)
    for s in (seg, robocupvision_amd.Segmenter(net)):                 # CPU frames are refused as before, with or without objects
        with pytest.raises((L.RcvError, ValueError, TypeError)):
            s(frames)


def test_segmenter_without_objects_keeps_its_two_tuple(monkeypatch):
    """No GPU here: the model's predict is replaced by a stand-in; what __call__ returns is the point."""
    import robocupvision_amd.model as Mo
    net = Mo.ROBO_UNet()
    lab, col = torch.zeros(1, 24, 32, dtype=torch.uint8), torch.zeros(1, 24, 32, 3, dtype=torch.uint8)
    monkeypatch.setattr(I, "prepare_frames", lambda frames, size, finetune: frames)
    monkeypatch.setattr(net, "predict", lambda imgs, colour, palette: (lab, col))
    out = robocupvision_amd.Segmenter(net)(torch.zeros(1, 24, 32, 3, dtype=torch.uint8))
    assert isinstance(out, tuple) and len(out) == 2 and out[0] is lab and out[1] is col
    with pytest.raises(L.RcvError, match="HIP device"):                # with objects the labels go to find_objects: CPU here
        robocupvision_amd.Segmenter(net, objects=I.DBCONVERT)(torch.zeros(1, 24, 32, 3, dtype=torch.uint8))


def test_dbconvert_rules_and_docstring():
    assert dict(I.DBCONVERT) == dict(num_class=5, min_area=(25, 200, 30, 0), min_ratio=(0.05, 0.05, 0.2, 0.0), max_objects=(6, 5, 2, 0))
    assert "contourArea" in I.DBCONVERT.__doc__ and "LARGEST" in I.DBCONVERT.__doc__


def test_objects_views_and_to_list():
    rows, counts = OR.find_objects(KNOWN_ANSWERS[9][1], 3, 0, 0.0, 2)           # background_values
    o = I.Objects(torch.from_numpy(rows).to(torch.int32), torch.from_numpy(counts).to(torch.int32))
    assert o.boxes.shape == (1, 2, 2, 4) and o.area.tolist() == [[[1, 1], [1, 0]]] and o.rank.tolist() == [[[0, 1], [0, 0]]]
    assert o.count.tolist() == [[2, 1]]
    assert o.centres.dtype == torch.float64 and o.centres[0, 0].tolist() == [[0.5, 0.5], [2.5, 0.5]]
    assert o.to_list() == [[(1, 0, 0, 1, 1, 1), (1, 2, 0, 1, 1, 1), (2, 4, 0, 1, 1, 1)]]
