"""CPU: the class-map cleaning record (RCV_OP_MAP_FILTER, csrc/map_filter.hip) -- its numpy restatement (tests/map_filter_restatement.py)
against scipy's binary morphology, against a second, vectorised statement of the majority vote, against the reference's loops and
against known answers worked out by hand; the properties the public functions promise; what the vote does to the component count
of a jittered map; and the plumbing: constant, symbol, query, every plan-time refusal, the Python refusals.  The kernel itself is
compared with the restatement bit for bit in tests/test_gpu_map_filter.py."""
import ctypes

import numpy as np
import pytest
import torch

import map_filter_restatement as R
import objdet_restatement as OD
import objects_restatement as OB
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import model as M

ODD = (3, 5, 15)


def _maps(seed, N=2, H=23, W=31, C=5, dtype=np.uint8):
    return R.blobby_map(np.random.default_rng(seed), N, H, W, C, dtype)


# ------------------------------------------------------------------------------------------------------- restatement vs scipy
@pytest.mark.parametrize("k", ODD)
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_morphology_restatement_equals_scipy(k, dtype):
    """One class c at a time, ``over`` = everything: closing is binary_erosion(binary_dilation(m, border 0), border 1), opening is
    binary_dilation(binary_erosion(m, border 1), border 0), erosion is one binary_erosion(border 1), with a k x k square."""
    ndi = pytest.importorskip("scipy.ndimage")
    C = 5
    m = _maps(100 + k, dtype=dtype)
    st = np.ones((k, k), bool)
    void = 255 if dtype == np.uint8 else -100
    for c in range(C):
        closed = R.close_map(m, C, classes=[c], window=k, over=range(C), over_void=True)
        opened = R.open_map(m, C, classes=[c], window=k, fill=void)
        eroded = R.erode_map(m, C, classes=[c], window=k, fill=void)
        for n in range(len(m)):
            b = m[n] == c
            want = ndi.binary_erosion(ndi.binary_dilation(b, st, border_value=0), st, border_value=1)
            assert np.array_equal(closed[n] == c, want), (k, c, n)
            assert np.array_equal(closed[n][~want], m[n][~want])                # ... and nothing else moved
            want = ndi.binary_dilation(ndi.binary_erosion(b, st, border_value=1), st, border_value=0)
            assert np.array_equal(opened[n] == c, want), (k, c, n)
            assert np.array_equal(opened[n][~b], m[n][~b]) and np.all(opened[n][b & ~want].astype(np.int64) == void)
            want = ndi.binary_erosion(b, st, border_value=1)
            assert np.array_equal(eroded[n] == c, want), (k, c, n)
            assert np.array_equal(eroded[n][~b], m[n][~b]) and np.all(eroded[n][b & ~want].astype(np.int64) == void)


# --------------------------------------------------------------------------------------------------------------- the majority vote
def _majority_by_integral(m, C, k, min_major, min_own, fill_void):
    """The second statement: one-hot planes, zero padding, a summed-area table, four corner reads per window."""
    m = np.asarray(m)
    N, H, W = m.shape
    r0, r1 = k // 2, k - 1 - k // 2
    wide = m.astype(np.int64)
    hot = (wide[:, None] == np.arange(C)[None, :, None, None]).astype(np.int64)                        # [N, C, H, W]
    sat = np.zeros((N, C, H + k, W + k), dtype=np.int64)
    sat[:, :, 1 + r0:1 + r0 + H, 1 + r0:1 + r0 + W] = hot
    sat = sat.cumsum(2).cumsum(3)
    h = sat[:, :, k:k + H, k:k + W] - sat[:, :, 0:H, k:k + W] - sat[:, :, k:k + H, 0:W] + sat[:, :, 0:H, 0:W]
    assert r0 + r1 == k - 1
    isc = (wide >= 0) & (wide < C)
    own = np.take_along_axis(h, np.where(isc, wide, 0)[:, None], 1)[:, 0]
    take = (isc | fill_void) & ((h.max(1) >= min_major) | (isc & (own < min_own)))
    return np.where(take, h.argmax(1), m).astype(m.dtype)


@pytest.mark.parametrize("k,min_major,min_own", [(4, 15, 7), (3, 6, 3), (1, 1, 0), (2, 4, 2), (5, 20, 9), (15, 120, 60)])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_majority_restatement_equals_the_vectorised_statement(k, min_major, min_own, dtype):
    for C in (1, 2, 5, 8):
        m = _maps(7 * k + C, C=C, dtype=dtype)
        for fill_void in (False, True):
            got = R.majority_filter(m, C, k, min_major, min_own, fill_void)
            assert got.dtype == m.dtype and np.array_equal(got, _majority_by_integral(m, C, k, min_major, min_own, fill_void))


def test_majority_restatement_equals_the_reference_loops():
    rng = np.random.default_rng(3)
    m = OD.jitter(rng, OD.blob_masks(rng, 2, 13, 17, 5, n_blobs=5), 5, p=0.1).astype(np.uint8)
    for k, a, b in ((4, 15, 7), (3, 6, 3), (5, 13, 4)):
        got = R.majority_filter(m, 5, k, a, b)
        for n in range(2):
            assert np.array_equal(got[n], R.majority_literal(m[n], 5, k, a, b))


def test_majority_known_answers():
    """k = 4 (offsets -2 ... +1), min_major 15, min_own 7, worked out by hand."""
    # a speckle in a uniform plane: the window of (2, 2) is rows 0..3 x columns 0..3, 15 of its 16 pixels are class 1 -> 1
    a = np.ones((1, 6, 6), np.uint8)
    a[0, 2, 2] = 3
    assert np.array_equal(R.majority_filter(a), np.ones((1, 6, 6), np.uint8))
    # one pixel of class 2 in each corner of a class-0 plane.  Windows: (0,0) rows 0..1 x cols 0..1, 4 pixels; (0,5) rows 0..1 x cols
    # 3..5, 6; (5,0) rows 3..5 x cols 0..1, 6; (5,5) rows 3..5 x cols 3..5, 9: one of class 2 each, own = 1 < 7 -> the majority, 0
    b = np.zeros((1, 6, 6), np.uint8)
    for y, x in ((0, 0), (0, 5), (5, 0), (5, 5)):
        b[0, y, x] = 2
    assert np.array_equal(R.majority_filter(b), np.zeros((1, 6, 6), np.uint8))
    # ... with min_own = 1 the corners stay: no window holds 15 pixels of one class but those of rows / cols 2..4 (16 pixels, all 0)
    assert np.array_equal(R.majority_filter(b, min_own=1), b)
    # a minority that is kept: class 2 on rows 0..3 x cols 2..3 without (0, 3), class 1 elsewhere
    c = np.ones((1, 6, 6), np.uint8)
    c[0, 0:4, 2:4] = 2
    c[0, 0, 3] = 1
    out = R.majority_filter(c)
    assert out[0, 2, 2] == 2      # window rows 0..3 x cols 0..3: 7 of class 2 (own = 7, not < 7), 9 of class 1 (< 15): kept
    assert out[0, 2, 3] == 2      # window rows 0..3 x cols 1..4: the same 7
    assert out[0, 0, 2] == 1      # window rows 0..1 x cols 0..3, 8 pixels: (0,2), (1,2), (1,3) of class 2, own = 3 < 7 -> majority 1
    assert out[0, 0, 3] == 1      # window rows 0..1 x cols 1..4: 5 of class 1, own = 5 < 7 -> the majority, itself
    assert out[0, 5, 5] == 1 and out[0, 0, 0] == 1 and out[0, 5, 0] == 1 and out[0, 0, 5] == 1
    # a tie goes to the lowest class: the window of (2, 2) of a 4 x 4 plane is the plane: six 1s, six 3s, four 4s; own = 4 < 7
    d = np.array([[[1, 1, 1, 1], [1, 1, 3, 3], [3, 3, 4, 4], [3, 3, 4, 4]]], np.int64)
    assert R.majority_filter(d)[0, 2, 2] == 1
    # void: counted in no class, kept unless fill_void; (1, 1) of a 3 x 3 plane sees rows 0..2 x cols 0..2 = nine pixels, eight of class 2
    e = np.full((1, 3, 3), 2, np.int64)
    e[0, 1, 1] = -100
    assert R.majority_filter(e, min_major=8)[0, 1, 1] == -100 and R.majority_filter(e, min_major=8, fill_void=True)[0, 1, 1] == 2
    assert R.majority_filter(e, min_major=9, fill_void=True)[0, 1, 1] == -100
    for plane in (a, b, c):
        assert np.array_equal(R.majority_filter(plane)[0], R.majority_literal(plane[0]))


# ---------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("k", ODD)
def test_open_and_close_are_idempotent(k):
    for dtype, void in ((np.uint8, 255), (np.int64, -100)):
        m = _maps(40 + k, H=37, W=41, dtype=dtype)
        for fill in (0, void):
            once = R.open_map(m, 5, window=k, fill=fill)
            assert np.array_equal(R.open_map(once, 5, window=k, fill=fill), once)
        for kw in (dict(), dict(classes=[2, 4], over=(0, 1)), dict(over=(), over_void=True), dict(over_void=False)):
            once = R.close_map(m, 5, window=k, **kw)
            assert np.array_equal(R.close_map(once, 5, window=k, **kw), once)
        assert not np.array_equal(R.close_map(m, 5, window=3), m) and not np.array_equal(R.open_map(m, 5, window=3), m)


@pytest.mark.parametrize("k", ODD)
def test_close_leaves_the_classes_outside_over_alone(k):
    m = _maps(60 + k, H=37, W=41, dtype=np.int64)
    for over, over_void in (((0,), True), ((0,), False), ((0, 3), True), ((), True)):
        out = R.close_map(m, 5, window=k, over=over, over_void=over_void)
        may = np.isin(m, list(over)) | (~R.is_class(m, 5) & over_void)
        assert np.array_equal(out[~may], m[~may])
        assert R.is_class(out[out != m], 5).all() and (out[out != m] >= 1).all()


def test_window_one_is_the_identity():
    for dtype in (np.uint8, np.int64):
        m = _maps(5, dtype=dtype)
        S = 0b11111
        assert np.array_equal(R.majority_filter(m, 5, 1, 1, 0), m) and np.array_equal(R.majority_filter(m, 5, 1, 1, 9, True), m)
        assert np.array_equal(R.erode_map(m, 5, window=1, fill=7), m)
        assert np.array_equal(R.open_map(m, 5, window=1, fill=7), m)
        assert np.array_equal(R.close_map(m, 5, classes=range(5), window=1, over=range(5)), m)
        own = np.where(R.is_class(m, 5), 1 << np.where(R.is_class(m, 5), m, 0).astype(np.int64), 0)
        assert np.array_equal(R.erode_bits(m, 5, 1, S), own) and np.array_equal(R.dilate_bits(m, 5, 1, S), own)
        assert np.array_equal(R.open_finish(own, m, 5, 1, S, 7), m) and np.array_equal(R.close_finish(own, m, 5, 1, S, 0x11f), m)


def test_trim_of_a_constant_map_is_the_identity():
    for k in (1, 2, 3, 4, 15):
        for c in (0, 4):
            m = np.full((2, 9, 11), c, np.int64)
            assert np.array_equal(R.trim_pseudo_labels(m, 5, k), m)
    m = np.full((1, 9, 11), 2, np.int64)
    m[0, 4, 5] = -100                        # ... and the rim of a hole goes: the 3 x 3 block around it
    out = R.trim_pseudo_labels(m, 5, 3)
    assert (out[0, 3:6, 4:7] == -100).all() and int((out == -100).sum()) == 9


# -------------------------------------------------------------------------------------------------------------------------- effect
def _component_total(maps, C):
    return sum(len(OB.components(plane, c)) for plane in maps for c in range(C))


def test_majority_vote_removes_speckle_components():
    """test.py counts every component as a predicted object: the vote must lower that count on a jittered blob map."""
    rng = np.random.default_rng(20)
    C = 5
    maps = OD.jitter(rng, OD.blob_masks(rng, 3, 60, 80, C), C, p=0.02)
    cleaned = R.majority_filter(maps, C, window=3, min_major=6, min_own=3)
    before, after = _component_total(maps, C), _component_total(cleaned, C)
    assert after < before, (before, after)
    assert after * 2 < before, (before, after)          # (speckles are most of the components of such a map)


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def _op(**kw):
    base = dict(n=2, h=9, w=11, cout=5, count=3, inmode=1, aux0=L.MF_ERODE, aux1=0b11110, stride=0, dil=0)
    base.update(kw)
    return L.make_op(L.OP_MAP_FILTER, 0, **base)


def test_constant_symbol_and_query():
    assert L.OP_MAP_FILTER == 69 and "rcv_map_filter" in L.EXPORTS and hasattr(L.load(), "rcv_map_filter")
    assert len(L.load().rcv_map_filter.argtypes) == 16
    assert (L.MF_MAJORITY, L.MF_ERODE, L.MF_ERODE_BITS, L.MF_DILATE_BITS, L.MF_OPEN_FINISH, L.MF_CLOSE_FINISH) == tuple(range(6))
    assert L.MAP_FILTER_TILE_H >= 8 and L.MAP_FILTER_TILE_W >= 8 and L.MAP_FILTER_MAX_WINDOW == 15
    src = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "rcv.h")).read()
    assert "#define RCV_MAP_FILTER_TILE_H %d\n" % L.MAP_FILTER_TILE_H in src and "#define RCV_MAP_FILTER_TILE_W %d\n" % L.MAP_FILTER_TILE_W in src
    assert "RCV_OP_MAP_FILTER = 69" in src
    h = L.planner_handle()
    for eb in (1, 8):
        for C in (1, 4, 5, 8):
            for k in range(1, 16):
                ops = [_op(inmode=eb, cout=C, count=k, aux0=L.MF_MAJORITY, aux1=0, stride=15, dil=7),
                       _op(inmode=eb, cout=C, count=k, aux0=L.MF_ERODE, aux1=(1 << C) - 1, stride=-100 if eb == 8 else 255)]
                if k & 1:
                    ops += [_op(inmode=eb, cout=C, count=k, aux0=L.MF_ERODE_BITS, aux1=1), _op(inmode=eb, cout=C, count=k, aux0=L.MF_DILATE_BITS, aux1=1),
                            _op(inmode=eb, cout=C, count=k, aux0=L.MF_OPEN_FINISH, aux1=1, inmode2=1),
                            _op(inmode=eb, cout=C, count=k, aux0=L.MF_CLOSE_FINISH, aux1=1, inmode2=1, dil=L.MF_OVER_VOID | 1)]
                for op in ops:
                    assert L.op_workspace(h, op) == 0 and op.i[L.RCV_I_NPART] == 0
    assert L.OpList([_op(cout=5), _op(cout=3, aux1=0b110, inmode=8, count=15)]).labels(h) == ["map_filter<erode,u8,k3,c8>", "map_filter<erode,i64,k15,c4>"]
    with pytest.raises(L.RcvError, match="planning-only"):
        L.OpList([_op()]).run(h, 0)


def test_plan_time_refusals():
    h = L.planner_handle()
    slot = (ctypes.c_int64 * 2)()
    a, b = ctypes.addressof(slot), ctypes.addressof(slot) + 8
    for kw, msg in ((dict(count=0), r"window 0 unsupported \(1\.\.15\)"),
                    (dict(count=16), r"window 16 unsupported \(1\.\.15\)"),
                    (dict(count=4, aux0=L.MF_ERODE_BITS), "rule erode_bits takes odd windows only"),
                    (dict(count=2, aux0=L.MF_DILATE_BITS), "rule dilate_bits takes odd windows only"),
                    (dict(count=4, aux0=L.MF_OPEN_FINISH, inmode2=1), "rule open_finish takes odd windows only"),
                    (dict(count=14, aux0=L.MF_CLOSE_FINISH, inmode2=1), "rule close_finish takes odd windows only"),
                    (dict(cout=0), r"0 classes unsupported \(1\.\.8\)"),
                    (dict(cout=9), r"9 classes unsupported \(1\.\.8\)"),
                    (dict(aux1=1 << 5), "class set 0x20 names a class >= 5"),
                    (dict(aux0=L.MF_DILATE_BITS, aux1=0x100), "class set 0x100 names a class >= 5"),
                    (dict(aux0=L.MF_CLOSE_FINISH, inmode2=1, dil=1 << 5), "over set 0x20 names a class >= 5"),
                    (dict(aux0=L.MF_CLOSE_FINISH, inmode2=1, dil=1 << 9), "over set 0x200 names a class >= 5"),
                    (dict(stride=256), r"fill 256 does not fit a uint8 map \(0\.\.255\)"),
                    (dict(stride=-100), r"fill -100 does not fit a uint8 map"),
                    (dict(aux0=L.MF_OPEN_FINISH, inmode2=1, stride=-1), r"fill -1 does not fit a uint8 map"),
                    (dict(inmode=4), "class map element size 4 unsupported"),
                    (dict(inmode=0), "class map element size 0 unsupported"),
                    (dict(aux0=6), "rule 6 unknown"),
                    (dict(aux0=-1), "rule -1 unknown"),
                    (dict(aux0=L.MF_MAJORITY, aux1=0, stride=0, dil=0), "min_major 0 must be >= 1"),
                    (dict(aux0=L.MF_MAJORITY, aux1=0, stride=1, dil=-1), "min_own -1 must be >= 0"),
                    (dict(aux0=L.MF_MAJORITY, aux1=2, stride=1, dil=0), "fill_void 2 must be 0 or 1"),
                    (dict(aux0=L.MF_OPEN_FINISH), "rule open_finish reads a bit map beside the original map"),
                    (dict(aux0=L.MF_ERODE, inmode2=1), "rule erode reads the class map alone"),
                    (dict(aux0=L.MF_OPEN_FINISH, inmode2=1, p_in=a, p_out=b), "rule open_finish needs the original map"),
                    (dict(aux0=L.MF_CLOSE_FINISH, inmode2=1, p_in=a, p_out=b), "rule close_finish needs the original map"),
                    (dict(aux0=L.MF_CLOSE_FINISH, inmode2=1, p_in=a, p_in2=b, p_out=b), "cannot overwrite the original map"),
                    (dict(p_in=a, p_out=a), "cannot run in place"),
                    (dict(aux0=L.MF_MAJORITY, aux1=0, stride=15, dil=7, p_in=a, p_out=a), "cannot run in place"),
                    (dict(n=0), "batch 0 of 9x11 planes out of range"),
                    (dict(h=0), "out of range")):
        with pytest.raises(L.RcvError, match=msg):
            L.op_workspace(h, _op(**kw))
    assert L.op_workspace(h, _op(inmode=8, stride=-100)) == 0 and L.op_workspace(h, _op(p_in=a, p_out=b)) == 0
    assert L.op_workspace(h, _op(aux0=L.MF_OPEN_FINISH, inmode2=1, p_in=a, p_in2=a, p_out=b)) == 0


def test_python_refusals():
    u8 = torch.zeros(2, 9, 11, dtype=torch.uint8)
    i64 = torch.zeros(2, 9, 11, dtype=torch.int64)
    for fn, args in ((I.majority_filter, ()), (I.erode_map, (5,)), (I.open_map, (5,)), (I.close_map, (5,)), (I.trim_pseudo_labels, (5,))):
        name = fn.__name__
        with pytest.raises(L.RcvError, match=name + r": class_map must be a \[N,H,W\] tensor"):
            fn(np.zeros((2, 9, 11), np.int64), *args)
        with pytest.raises(L.RcvError, match=name + r": class_map must be a \[N,H,W\] tensor"):
            fn(i64[0], *args)
        with pytest.raises(L.RcvError, match="int64 pseudo-labels expected|dtype torch.int32 unsupported"):
            fn(i64.int(), *args)
        good = i64 if fn is I.trim_pseudo_labels else u8
        with pytest.raises(L.RcvError, match=name + " needs the class map on the HIP device"):
            fn(good, *args)
        with pytest.raises(L.RcvError, match=name + " needs the class map on the HIP device"):
            fn(good, *args, return_changed=True)
        with pytest.raises(L.RcvError, match=r"window 16 unsupported \(1\.\.15\)"):          # the library's message comes first
            fn(good, *args, window=16)
        with pytest.raises(L.RcvError, match=name + ": window: 2.5 is not an integer"):
            fn(good, *args, window=2.5)
        assert fn(good, *args, _plan_only=True) is None
    with pytest.raises(L.RcvError, match="int64 pseudo-labels expected"):
        I.trim_pseudo_labels(u8, 5)
    with pytest.raises(L.RcvError, match="9 classes unsupported"):
        I.majority_filter(u8, 9)
    with pytest.raises(L.RcvError, match="min_major 0 must be >= 1"):
        I.majority_filter(u8, min_major=0)
    with pytest.raises(L.RcvError, match="majority_filter: min_own: 'x' is not an integer|majority_filter: min_own: invalid literal"):
        I.majority_filter(u8, min_own="x")
    with pytest.raises(L.RcvError, match="takes odd windows only"):
        I.open_map(u8, 5, window=4)
    with pytest.raises(L.RcvError, match="takes odd windows only"):
        I.close_map(u8, 5, window=2)
    assert I.erode_map(u8, 5, window=4, _plan_only=True) is None and I.majority_filter(u8, window=2, _plan_only=True) is None
    with pytest.raises(L.RcvError, match="class set 0x22 names a class >= 5"):
        I.erode_map(u8, 5, classes=[1, 5])
    with pytest.raises(L.RcvError, match="class set 0x20 names a class >= 5"):
        I.close_map(u8, 5, classes=(5,))
    with pytest.raises(L.RcvError, match="over set 0x140 names a class >= 5"):
        I.close_map(u8, 5, over=(6,))
    with pytest.raises(L.RcvError, match="open_map: classes: class -1 out of range"):
        I.open_map(u8, 5, classes=[-1])
    with pytest.raises(L.RcvError, match="fill 256 does not fit a uint8 map"):
        I.erode_map(u8, 5, fill=256)
    with pytest.raises(L.RcvError, match="fill -100 does not fit a uint8 map"):
        I.open_map(u8, 5, fill=-100)
    assert I.open_map(i64, 5, fill=-100, _plan_only=True) is None
    for name in ("majority_filter", "erode_map", "open_map", "close_map", "trim_pseudo_labels"):
        assert getattr(robocupvision_amd, name) is getattr(I, name) and name in I.__all__


def test_segmenter_clean_is_checked_at_construction():
    net = M.ROBO_UNet()
    seg = robocupvision_amd.Segmenter(net, clean=[("majority", {}), ("close", {"window": 5}), ("open", {"classes": [1]}), ("erode", {"fill": 0})])
    assert [fn.__name__ for fn, _ in seg._clean[0]] == ["majority_filter", "close_map", "open_map", "erode_map"] and seg._clean[1] == []
    assert all(kw["num_class"] == 5 for _, kw in seg._clean[0]) and robocupvision_amd.Segmenter(net)._clean is None
    seg = robocupvision_amd.Segmenter(net, pseudo_labels=0.9, clean=[("trim", {"window": 5}), ("majority", {"num_class": 4})])
    assert [fn.__name__ for fn, _ in seg._clean[1]] == ["trim_pseudo_labels"] and seg._clean[0][0][1]["num_class"] == 4
    for bad, msg in (("majority", "clean must be a list"),
                     ([("majority",)], "is not a \\(step, keywords\\) pair"),
                     (["majority"], "is not a \\(step, keywords\\) pair"),
                     ([("median", {})], "clean step 'median' unknown"),
                     ([("trim", {})], "clean step 'trim' unknown \\(majority, erode, open, close; trim with pseudo_labels\\)"),
                     ([("majority", {"classes": [1]})], "clean step 'majority' takes the keywords"),
                     ([("close", {"fill": 0})], "clean step 'close' takes the keywords"),
                     ([("majority", {"window": 16})], "window 16 unsupported"),
                     ([("close", {"window": 4})], "rule dilate_bits takes odd windows only"),
                     ([("open", {"classes": [7]})], "class set 0x80 names a class >= 5"),
                     ([("erode", {"fill": 300})], "fill 300 does not fit a uint8 map"),
                     ([("majority", {}), ("erode", {"num_class": 9})], "9 classes unsupported")):
        with pytest.raises(L.RcvError, match=msg):
            robocupvision_amd.Segmenter(net, clean=bad)
    with pytest.raises(L.RcvError, match="needs the frames on the HIP device|HIP device"):
        robocupvision_amd.Segmenter(net, clean=[("majority", {})])(torch.zeros(1, 24, 32, 3, dtype=torch.uint8))
