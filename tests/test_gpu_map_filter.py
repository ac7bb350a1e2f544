"""GPU: RCV_OP_MAP_FILTER (csrc/map_filter.hip; ``majority_filter`` / ``erode_map`` / ``open_map`` / ``close_map`` /
``trim_pseudo_labels`` / ``Segmenter(clean=...)``) against the numpy restatement (tests/map_filter_restatement.py, itself checked against
scipy and the reference's loops on the CPU in tests/test_map_filter.py) -- bit for bit, no tolerance: planes smaller than any window,
planes that cross every halo edge and corner between tiles, every window parity, 1..8 classes (the 32-bit and the 64-bit counts),
uint8 and int64 maps with their void values, the byte lanes at their largest count, the three branches of the vote, overlapping
closings, the changed counter."""
import ctypes

import numpy as np
import pytest
import torch

import batch_prep_restatement as BR
import map_filter_restatement as R
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import model as M
from robocupvision_amd import palette as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = L.MAP_FILTER_TILE_H, L.MAP_FILTER_TILE_W
PLANES = [(1, 1), (2, 3), (3, 2), (TH - 1, TW + 1), (2 * TH + 3, 2 * TW + 5)]
WINDOWS = (1, 2, 3, 4, 5, 15)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    """Bit for bit, dtype included; ``got``: a tensor or (tensor, changed)."""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d pixels differ, first at %s: %s, want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _both(fn, ref, m, *args, **kw):
    """The public function with and without the changed counter against the restatement."""
    want = ref(m, *args, **kw)
    what = "%s%s %s %s" % (fn.__name__, m.shape, args, kw)
    _same(fn(_dev(m), *args, **kw), want, what)
    out, changed = fn(_dev(m), *args, return_changed=True, **kw)
    _same(out, want, what)
    assert changed.dtype == torch.int32 and changed.cpu().tolist() == R.changed(m, want).tolist(), what


def _subsets(C):
    return [None, [C - 1], list(range(0, C, 2))]


@pytest.mark.parametrize("C", [1, 2, 5, 8])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("plane", PLANES)
def test_public_functions_equal_the_restatement(plane, dtype, C):
    H, W = plane
    rng = np.random.default_rng(1000 * C + 7 * H + W)
    m3 = R.blobby_map(rng, 3, H, W, C, dtype)
    void = 255 if dtype == np.uint8 else -100
    for k in WINDOWS:
        for m in ((m3, m3[:1]) if k in (4, 5) else (m3,)):          # batches of 3 and of 1
            n_win = min(k, H + k // 2) * min(k, W + k // 2)
            for fill_void in (False, True):
                _both(I.majority_filter, R.majority_filter, m, C, k, max(1, (3 * n_win) // 5), n_win // 4, fill_void)
            _both(I.majority_filter, R.majority_filter, m, C, k, 1, 0, True)          # every looked-at pixel takes the majority
            for classes, fill in zip(_subsets(C), (void, 0, 200 if dtype == np.uint8 else (1 << 31) - 1)):
                _both(I.erode_map, R.erode_map, m, C, classes, k, fill)
                if k & 1:
                    _both(I.open_map, R.open_map, m, C, classes, k, fill)
            if k & 1:
                _both(I.close_map, R.close_map, m, C, None, k)
                _both(I.close_map, R.close_map, m, C, list(range(C)), k, tuple(range(C)), True)
                _both(I.close_map, R.close_map, m, C, [C - 1], k, (0, C - 1), False)
            if dtype == np.int64:
                _both(I.trim_pseudo_labels, R.trim_pseudo_labels, m, C, k)


def _run(op):
    L.OpList([op]).run(L.handle(0), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_bit_map_records_and_the_named_entry(dtype):
    """The two halves of opening and closing as records: the bit maps themselves, then the finish rules on them."""
    N, H, W, C, k = 2, TH + 5, TW + 7, 5, 3
    S, O = 0b10110, 0b00001 | L.MF_OVER_VOID
    eb = np.dtype(dtype).itemsize
    m = R.blobby_map(np.random.default_rng(77), N, H, W, C, dtype)
    src = _dev(m)
    base = dict(n=N, h=H, w=W, cout=C, count=k, inmode=eb, aux1=S)
    for rule, ref in ((L.MF_ERODE_BITS, R.erode_bits), (L.MF_DILATE_BITS, R.dilate_bits)):
        bits = torch.full((N, H, W), 0xee, dtype=torch.uint8, device=DEV)
        _run(L.make_op(L.OP_MAP_FILTER, 0, aux0=rule, p_in=src.data_ptr(), p_out=bits.data_ptr(), **base))
        want = ref(m, C, k, S)
        _same(bits, want, "bits rule %d" % rule)
        out = torch.empty_like(src)
        changed = torch.full((N,), 5, dtype=torch.int32, device=DEV)          # the counter is added to
        if rule == L.MF_ERODE_BITS:
            fin, want2, a0, a1 = L.MF_OPEN_FINISH, R.open_finish(want, m, C, k, S, 9), 9, 0
        else:
            fin, want2, a0, a1 = L.MF_CLOSE_FINISH, R.close_finish(want, m, C, k, S, O), 0, O
        _run(L.make_op(L.OP_MAP_FILTER, 0, aux0=fin, inmode2=1, stride=a0, dil=a1, p_in=bits.data_ptr(), p_in2=src.data_ptr(), p_out=out.data_ptr(),
                       p_x0=changed.data_ptr(), **base))
        _same(out, want2, "finish rule %d" % fin)
        assert changed.cpu().tolist() == (R.changed(m, want2) + 5).tolist()
        # bits outside S in a caller's bit map are not counted
        noisy = bits | 0b01001
        out2 = torch.empty_like(src)
        _run(L.make_op(L.OP_MAP_FILTER, 0, aux0=fin, inmode2=1, stride=a0, dil=a1, p_in=noisy.data_ptr(), p_in2=src.data_ptr(), p_out=out2.data_ptr(),
                       **base))
        _same(out2, want2, "finish rule %d, foreign bits" % fin)
    out = torch.empty_like(src)
    changed = torch.zeros(N, dtype=torch.int32, device=DEV)
    L.check(L.load().rcv_map_filter(L.handle(0), src.data_ptr(), None, eb, N, H, W, C, 4, L.MF_MAJORITY, 0, 15, 7, out.data_ptr(), changed.data_ptr(),
                                    torch.cuda.current_stream(DEV).cuda_stream), "rcv_map_filter")
    torch.cuda.synchronize()
    want = R.majority_filter(m)
    _same(out, want, "rcv_map_filter")
    assert changed.cpu().tolist() == R.changed(m, want).tolist()
    with pytest.raises(L.RcvError, match="cannot run in place"):
        _run(L.make_op(L.OP_MAP_FILTER, 0, aux0=L.MF_ERODE, p_in=src.data_ptr(), p_out=src.data_ptr(), **base))
    with pytest.raises(L.RcvError, match="null operand"):
        _run(L.make_op(L.OP_MAP_FILTER, 0, aux0=L.MF_ERODE, p_in=src.data_ptr(), **base))


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_byte_lanes_do_not_carry(dtype):
    """k = 15: a plane of one class puts 225 into one byte lane, its neighbours must read 0 (classes 0 and 7: the two ends of the
    packed word); a checkerboard of classes 3 and 4 puts 113 and 112 on either side of the boundary between the two halves."""
    H, W, C, k = TH + 9, TW + 9, 8, 15
    yy, xx = np.mgrid[0:H, 0:W]
    planes = [np.full((H, W), 0), np.full((H, W), 7), np.where((yy + xx) & 1, 3, 4)]
    m = np.stack(planes).astype(dtype)
    h, n = R.window_counts(m, C, k)
    assert h[0, 0].max() == 225 and h[7, 1].max() == 225 and h[1:, 0].max() == 0 and h[:7, 1].max() == 0 and n.max() == 225
    assert {int(h[3, 2, 20, 20]), int(h[4, 2, 20, 20])} == {112, 113}
    for min_major, min_own in ((225, 225), (113, 113), (1, 0), (226, 113)):
        _both(I.majority_filter, R.majority_filter, m, C, k, min_major, min_own)
    _both(I.erode_map, R.erode_map, m, C, None, k, 5)
    _both(I.open_map, R.open_map, m, C, None, k, 5)
    _both(I.close_map, R.close_map, m, C, list(range(C)), k, tuple(range(C)), True)
    for c, plane in ((0, 0), (7, 1)):          # ... and what the answers are, without the restatement
        one = _dev(m[plane:plane + 1])
        for out in (I.majority_filter(one, C, k, 225, 225), I.erode_map(one, C, None, k, 5), I.open_map(one, C, None, k, 5),
                    I.close_map(one, C, list(range(C)), k, tuple(range(C)))):
            assert torch.equal(out, one)
        bits = torch.empty(1, H, W, dtype=torch.uint8, device=DEV)
        for rule in (L.MF_ERODE_BITS, L.MF_DILATE_BITS):
            _run(L.make_op(L.OP_MAP_FILTER, 0, n=1, h=H, w=W, cout=C, count=k, inmode=np.dtype(dtype).itemsize, aux0=rule, aux1=0xff,
                           p_in=one.data_ptr(), p_out=bits.data_ptr()))
            assert bool((bits == (1 << c)).all())
    board = _dev(m[2:3])
    vote = I.majority_filter(board, C, k, 113, 0).cpu().numpy()[0]          # interior windows hold 113 of the centre's colour
    assert np.array_equal(vote[7:H - 7, 7:W - 7], m[2, 7:H - 7, 7:W - 7])
    dil = torch.empty(1, H, W, dtype=torch.uint8, device=DEV)
    _run(L.make_op(L.OP_MAP_FILTER, 0, n=1, h=H, w=W, cout=C, count=3, inmode=np.dtype(dtype).itemsize, aux0=L.MF_DILATE_BITS, aux1=0xff,
                   p_in=board.data_ptr(), p_out=dil.data_ptr()))
    assert bool((dil == 0b11000).all())


def test_all_three_branches_of_the_vote_are_taken():
    rng = np.random.default_rng(5)
    H, W, C = 2 * TH + 3, 2 * TW + 5, 5
    for dtype in (np.uint8, np.int64):
        m = R.blobby_map(rng, 3, H, W, C, dtype)
        for k, a, b in ((4, 15, 7), (3, 6, 3), (5, 20, 8)):
            major, few, kept = R.majority_branches(m, C, k, a, b)
            want = R.majority_filter(m, C, k, a, b)
            assert major.any() and few.any() and kept.any()
            assert (want != m)[major].any() and (want != m)[few].any() and not (want != m)[kept].any()
            assert (~R.is_class(m, C)).any() and np.array_equal(want[~R.is_class(m, C)], m[~R.is_class(m, C)])
            _both(I.majority_filter, R.majority_filter, m, C, k, a, b)


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_overlapping_closings_and_foreign_neighbours(dtype):
    """(a) A checkerboard of classes 1 and 2 with single background and void pixels: every such hole lies in the closing of both
    classes, the lowest wins.  (b) A ring of class 1 around background and one pixel of class 3: the closing fills the background,
    class 3 is outside ``over`` and stays; with over=(0, 3) it goes too."""
    H, W, C = TH + 3, TW + 3, 5
    void = 255 if dtype == np.uint8 else -100
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.where((yy + xx) & 1, 1, 2)
    holes = (yy % 5 == 2) & (xx % 7 == 3)
    a[holes] = np.where((yy[holes] // 5) & 1, 0, void)
    a = a[None].astype(dtype)
    want = R.close_map(a, C, window=3)
    assert (want[0][holes] == 1).all() and np.array_equal(want[0][~holes], a[0][~holes])
    _both(I.close_map, R.close_map, a, C, None, 3)
    want = R.close_map(a, C, window=3, over_void=False)
    assert (want[0][holes & (a[0] == 0)] == 1).all() and np.array_equal(want[0][a[0] != 0], a[0][a[0] != 0])
    _both(I.close_map, R.close_map, a, C, None, 3, (0,), False)
    _both(I.close_map, R.close_map, a, C, [2], 3)          # class 2 alone claims them
    assert (R.close_map(a, C, [2], 3)[0][holes] == 2).all()

    b = np.zeros((1, H, W), dtype)
    b[0, 10:17, 20:27] = 1
    b[0, 12:15, 22:25] = 0
    b[0, 13, 23] = 3
    want = R.close_map(b, C, window=5)
    assert want[0, 13, 23] == 3 and (want[0, 12:15, 22:25] == np.array([[1, 1, 1], [1, 3, 1], [1, 1, 1]])).all()
    _both(I.close_map, R.close_map, b, C, None, 5)
    want = R.close_map(b, C, window=5, over=(0, 3))
    assert (want[0, 10:17, 20:27] == 1).all()          # (class 3's own closing is the one pixel; class 1, the lower, takes it)
    _both(I.close_map, R.close_map, b, C, None, 5, (0, 3))


def _net(seed=5):
    torch.manual_seed(seed)
    net = M.ROBO_UNet()
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    return net.to(DEV).eval()


def test_segmenter_clean_equals_the_functions_on_its_labels():
    net = _net()
    frames = _dev(BR.synthetic_frames(2, 48, 64, 9)[0])
    size = (48, 64)
    lab0, col0 = robocupvision_amd.Segmenter(net, img_size=size)(frames)
    steps = [("majority", {"window": 3, "min_major": 6, "min_own": 3}), ("close", {"window": 3}), ("open", {"classes": [1, 2], "window": 3}),
             ("erode", {"classes": [4], "window": 2, "fill": 0})]
    lab, col = robocupvision_amd.Segmenter(net, img_size=size, clean=steps)(frames)
    want = I.erode_map(I.open_map(I.close_map(I.majority_filter(lab0, 5, 3, 6, 3), 5, window=3), 5, [1, 2], 3), 5, [4], 2, 0)
    assert lab.dtype == torch.uint8 and torch.equal(lab, want)
    assert torch.equal(col, P.colorize(want)) and torch.equal(col, P.device_palette(None, DEV)[want.long()])
    # objects see the cleaned map; pseudo-labels take the trim step, the class map the others
    lab2, col2, objs = robocupvision_amd.Segmenter(net, img_size=size, clean=steps, objects=I.DBCONVERT)(frames)
    assert torch.equal(lab2, want) and torch.equal(col2, col) and torch.equal(objs.rows, I.find_objects(want, **I.DBCONVERT).rows)
    plain = robocupvision_amd.Segmenter(net, img_size=size, pseudo_labels=0.5)(frames)
    lab3, pseudo3, col3 = robocupvision_amd.Segmenter(net, img_size=size, pseudo_labels=0.5, clean=[("trim", {"window": 3}), steps[0]])(frames)
    assert torch.equal(lab3, I.majority_filter(plain[0], 5, 3, 6, 3)) and torch.equal(col3, P.colorize(lab3))
    assert torch.equal(pseudo3, I.trim_pseudo_labels(plain[1], 5, 3)) and int((pseudo3 == -100).sum()) >= int((plain[1] == -100).sum())


def test_segmenter_without_clean_is_unchanged():
    net = _net()
    frames = _dev(BR.synthetic_frames(2, 48, 64, 9)[0])
    from robocupvision_amd import data as D
    imgs = D.prepare_frames(frames, (24, 32), False)
    lab, col = robocupvision_amd.Segmenter(net, img_size=(24, 32))(frames)
    want, want_col = net.predict(imgs, colour=True)
    assert torch.equal(lab, want) and torch.equal(col, want_col)
    lab, col = robocupvision_amd.Segmenter(net, img_size=(24, 32), clean=[])(frames)          # no steps: the same map, coloured apart
    assert torch.equal(lab, want) and torch.equal(col, want_col)
