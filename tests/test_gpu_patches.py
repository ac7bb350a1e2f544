"""GPU: RCV_OP_OBJECT_PATCHES (csrc/patches.hip; ``object_patches`` / ``classify_objects`` / ``Segmenter(patches=...)``) against the numpy
restatement of the contract (tests/patches_restatement.py, pinned to Pillow by tests/test_patches.py), bitwise: hand-built rows and
counts with every edge case, a non-integer frame / map ratio, a large frame whose boxes cross and end on the chunk boundaries of the
horizontal pass, the chain from a class map, two streams, the patch classifiers and the Segmenter."""
import numpy as np
import pytest
import torch

import objdet_restatement as R
import patches_restatement as PR
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import patches as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 64          # PT_CHUNK of csrc/patches.hip: source rows whose horizontal pass is held in LDS at a time


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_equal(got, ref, what):
    """(images, bytes, valid) of the device against the restatement, bitwise."""
    images, byts, valid = got
    assert np.array_equal(valid, ref[2]), "%s: valid differs" % what
    bad = np.argwhere(byts != ref[1])
    assert bad.size == 0, "%s: %d bytes differ, first (slot, y, x, c) %s: device %d vs %d" % (
        what, len(bad), bad[0].tolist(), byts[tuple(bad[0])], ref[1][tuple(bad[0])])
    bad = np.argwhere(images.view(np.uint32) != ref[0].view(np.uint32))
    assert bad.size == 0, "%s: %d image elements differ, first (slot, c, y, x) %s: device %r vs %r" % (
        what, len(bad), bad[0].tolist(), images[tuple(bad[0])], ref[0][tuple(bad[0])])


def _device(frames, rows, counts, **kw):
    p = P.object_patches(_dev(frames), (_dev(rows), _dev(counts)), return_bytes=True, **kw)
    torch.cuda.synchronize()
    return p.images.cpu().numpy(), p.bytes.cpu().numpy(), p.valid.cpu().numpy()


def _named_entry(frames, rows, counts, map_size, size, margin, with_bytes=True):
    """rcv_object_patches on buffers pre-filled with junk: every element must be written by the launch."""
    f, r, c = _dev(frames), _dev(rows), _dev(counts)
    N, Hs, Ws, _ = frames.shape
    _, Cm1, Mx, _ = rows.shape
    n = N * Cm1 * Mx
    images = torch.full((n, 3) + tuple(size), float("nan"), dtype=torch.float32, device=DEV)
    byts = torch.full((n,) + tuple(size) + (3,), 0xA5, dtype=torch.uint8, device=DEV)
    h = L.handle(0)
    L.check(L.load().rcv_object_patches(h, f.data_ptr(), N, Hs, Ws, r.data_ptr(), c.data_ptr(), Cm1 + 1, Mx, map_size[0], map_size[1],
                                        size[0], size[1], margin, images.data_ptr(), byts.data_ptr() if with_bytes else None,
                                        torch.cuda.current_stream().cuda_stream), "rcv_object_patches")
    torch.cuda.synchronize()
    return images.cpu().numpy(), byts.cpu().numpy()


@pytest.mark.parametrize("size,margin", [((32, 32), 0), ((16, 24), 2), ((1, 1), 0), ((33, 31), 1), ((64, 64), 0)],
                         ids=["32x32", "16x24_m2", "1x1", "33x31_m1", "64x64"])
def test_hand_built_rows_bitwise(size, margin):
    """N = 2, C-1 = 4, M = 3 on 96 x 128 frames with a 24 x 32 map: the edge boxes of the restatement, counts partly below M (one above
    it), other in-range boxes past the counts.  Through ``object_patches`` (a record in an OpList) and through the named entry."""
    Hs, Ws, H, W = 96, 128, 24, 32
    frames = PR.seeded_frames(3, 2, Hs, Ws)
    rows, counts = PR.hand_built(H, W)
    ref = PR.object_patches(frames, rows, counts, (H, W), size, margin)
    assert ref[2].sum() == 15 and not ref[1][~ref[2].reshape(-1)].any()
    _assert_equal(_device(frames, rows, counts, map_size=(H, W), size=size, margin=margin), ref, "object_patches")
    images, byts = _named_entry(frames, rows, counts, (H, W), size, margin)
    _assert_equal((images, byts, ref[2]), ref, "rcv_object_patches")
    if size == (32, 32):
        images, byts = _named_entry(frames, rows, counts, (H, W), size, margin, with_bytes=False)      # no bytes: images alone
        assert np.array_equal(images.view(np.uint32), ref[0].view(np.uint32)) and (byts == 0xA5).all()
        p = P.object_patches(_dev(frames), I.Objects(_dev(rows), _dev(counts)), map_size=(H, W))
        assert p.bytes is None and p.shape_nkm == (2, 4, 3) and torch.equal(p.images.cpu(), torch.from_numpy(ref[0]))


def test_default_map_is_the_frame():
    frames = PR.seeded_frames(4, 2, 40, 56)
    rows, counts = PR.hand_built(40, 56)
    _assert_equal(_device(frames, rows, counts), PR.object_patches(frames, rows, counts), "map = frame")


def test_frames_at_an_odd_address():
    """The kernel stages source rows with 16-byte aligned loads; a frame buffer that starts 5 bytes into such a word (a view into a
    larger allocation) takes the guarded path at its first and last bytes -- the whole-frame box reads both."""
    frames = PR.seeded_frames(14, 2, 40, 57)
    rows, counts = PR.hand_built(40, 57)
    buf = torch.zeros(frames.size + 5, dtype=torch.uint8, device=DEV)
    view = buf[5:].view(frames.shape)
    view.copy_(_dev(frames))
    assert view.data_ptr() % 16 == 5 and view.is_contiguous()
    p = P.object_patches(view, (_dev(rows), _dev(counts)), return_bytes=True)
    torch.cuda.synchronize()
    _assert_equal((p.images.cpu().numpy(), p.bytes.cpu().numpy(), p.valid.cpu().numpy()), PR.object_patches(frames, rows, counts), "odd address")


def test_non_integer_ratio():
    """90 x 130 frames over a 24 x 32 map: box corners at multiples of 3.75 / 4.0625."""
    frames = PR.seeded_frames(5, 2, 90, 130)
    rows, counts = PR.hand_built(24, 32, seed=6)
    for size, margin in (((32, 32), 0), ((16, 24), 1)):
        ref = PR.object_patches(frames, rows, counts, (24, 32), size, margin)
        _assert_equal(_device(frames, rows, counts, map_size=(24, 32), size=size, margin=margin), ref, "90x130 %s" % (size,))


def test_large_frame_crosses_every_chunk_boundary():
    """One 480 x 640 frame: the full-frame box (30 / 40 taps per row / column, the widest coefficient rows; its 480 source rows are
    seven and a half chunks of CHUNK rows and an output row straddles every boundary), a 5 x 5 box, and two boxes whose source rows
    are exactly two chunks (one starting at row 0, one not)."""
    Hs, Ws = 480, 640
    frames = PR.seeded_frames(7, 1, Hs, Ws)
    boxes = [(0, 0, Ws, Hs), (317, 211, 5, 5), (100, 0, 200, 126), (100, 30, 200, 124)]
    rows = np.zeros((1, 1, 4, 8), np.int32)
    rows[0, 0, :, 0:4] = boxes
    counts = np.array([[[9, 9, 9, 4]]], np.int32)
    yf, yn, _ = PR.box_coeffs(Hs, 0.0, float(Hs), 32)
    assert max(yn) == 30 and all(any(yf[y] < b < yf[y] + yn[y] for y in range(32)) for b in range(CHUNK, Hs, CHUNK))
    for (x, y, w, h), first in ((boxes[2], 0), (boxes[3], 28)):
        yf, yn, _ = PR.box_coeffs(Hs, float(y), float(y + h), 32)
        assert yf[0] == first and yf[-1] + yn[-1] - yf[0] == 2 * CHUNK
    ref = PR.object_patches(frames, rows, counts)
    _assert_equal(_device(frames, rows, counts), ref, "480x640")


def test_chain_from_class_maps():
    """blob maps -> find_objects(**DBCONVERT) -> object_patches: the restatement applied to the device's own rows and counts."""
    rng = np.random.default_rng(9)
    maps = R.blob_masks(rng, 3, 24, 32, 5, n_blobs=14, r_max=7)
    frames = PR.seeded_frames(8, 3, 96, 128)
    objs = I.find_objects(_dev(maps).to(torch.uint8), **I.DBCONVERT)
    p = robocupvision_amd.object_patches(_dev(frames), objs, map_size=(24, 32), return_bytes=True)
    torch.cuda.synchronize()
    rows, counts = objs.rows.cpu().numpy(), objs.counts.cpu().numpy()
    ref = PR.object_patches(frames, rows, counts, (24, 32))
    assert ref[2].sum() >= 3 and p.shape_nkm == (3, 4, 6)
    _assert_equal((p.images.cpu().numpy(), p.bytes.cpu().numpy(), p.valid.cpu().numpy()), ref, "chain")


def test_reproducible_on_two_streams():
    frames, (rows, counts) = _dev(PR.seeded_frames(3, 2, 96, 128)), (_dev(a) for a in PR.hand_built(24, 32))
    kw = dict(map_size=(24, 32), margin=1, return_bytes=True)
    a = P.object_patches(frames, (rows, counts), **kw)
    b = P.object_patches(frames, (rows, counts), **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        c = P.object_patches(frames, (rows, counts), **kw)
    side.synchronize()
    for other in (b, c):
        assert torch.equal(a.images.view(torch.int32), other.images.view(torch.int32)) and torch.equal(a.bytes, other.bytes)
    assert a.bytes.any()


def _patches_for_classifiers():
    frames = _dev(PR.seeded_frames(12, 2, 96, 128))
    rows, counts = (_dev(a) for a in PR.hand_built(24, 32))
    return frames, (rows, counts), P.object_patches(frames, (rows, counts), map_size=(24, 32))


@pytest.mark.parametrize("name", ["BNNMC", "BNNL"])
def test_classify_objects_with_the_bnn_classifiers(name):
    from robocupvision_amd import bnn
    torch.manual_seed(77)
    model = getattr(bnn, name)().to(DEV).eval()
    frames, objects, p = _patches_for_classifiers()
    cls = robocupvision_amd.classify_objects(frames, objects, model, map_size=(24, 32))
    want = model.predict(p.images).reshape(p.shape_nkm)
    torch.cuda.synchronize()
    valid = p.valid
    assert cls.dtype == torch.uint8 and tuple(cls.shape) == (2, 4, 3) and int(valid.sum()) == 15
    assert torch.equal(cls[valid], want[valid]) and (cls[~valid] == 255).all() and (cls[valid] < 4).all()
    assert torch.equal(cls, P.classify_patches(p, model))


def test_classify_objects_through_the_logits_route():
    import robocupvision_amd.model as Mo
    torch.manual_seed(78)
    model = Mo.PB_FCN(32, 4, 1, False, 1).to(DEV).train()
    frames, objects, p = _patches_for_classifiers()
    cls = robocupvision_amd.classify_objects(frames, objects, model, map_size=(24, 32))
    assert model.training                                  # called in eval mode, left as it was
    with torch.no_grad():
        logits = model.eval()(p.images)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (24, 4, 1, 1)
    want = torch.max(logits, 1)[1].reshape(p.shape_nkm).to(torch.uint8)
    valid = p.valid
    assert torch.equal(cls[valid], want[valid]) and (cls[~valid] == 255).all()


def test_segmenter_with_patches_and_classifier():
    import robocupvision_amd.model as Mo
    from robocupvision_amd.bnn import BNNMC
    torch.manual_seed(2025)
    net = Mo.ROBO_UNet().to(DEV)
    clf = BNNMC().to(DEV)
    frames = _dev(PR.seeded_frames(13, 2, 96, 128))
    labels, colour, objs, cut, classes = robocupvision_amd.Segmenter(net, img_size=(24, 32), objects=I.DBCONVERT, patches={},
                                                                     classifier=clf)(frames)
    plain = robocupvision_amd.Segmenter(net, img_size=(24, 32), objects=I.DBCONVERT)(frames)
    torch.cuda.synchronize()
    assert len(plain) == 3 and torch.equal(plain[0], labels) and torch.equal(plain[1], colour)
    assert torch.equal(plain[2].rows, objs.rows) and torch.equal(plain[2].counts, objs.counts)
    by_hand = P.object_patches(frames, objs, map_size=(24, 32))
    assert cut.bytes is None and cut.shape_nkm == (2, 4, 6)
    assert torch.equal(cut.images.view(torch.int32), by_hand.images.view(torch.int32)) and torch.equal(cut.valid, by_hand.valid)
    assert torch.equal(classes, P.classify_patches(by_hand, clf)) and tuple(classes.shape) == (2, 4, 6)
    ref = PR.object_patches(frames.cpu().numpy(), objs.rows.cpu().numpy(), objs.counts.cpu().numpy(), (24, 32))
    assert np.array_equal(cut.images.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
    four = robocupvision_amd.Segmenter(net, img_size=(24, 32), objects=I.DBCONVERT, patches=dict(return_bytes=True, margin=1))(frames)
    assert len(four) == 4 and four[3].bytes is not None and tuple(four[3].bytes.shape) == (48, 32, 32, 3)
