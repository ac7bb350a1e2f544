"""CPU: the object-patch contract (tests/patches_restatement.py) against live Pillow ``Image.resize((Sw, Sh), BILINEAR, box=...)``, byte
for byte; its YUV step against tests/rgb_prep_restatement.py's step 4; validity, clamping, margin and zero fill; the refusals of the
RCV_OP_OBJECT_PATCHES record through a planner handle, of ``object_patches`` / ``classify_objects`` and of ``Segmenter``."""
import ctypes

import numpy as np
import pytest
import torch

import patches_restatement as PR
import rgb_prep_restatement as RP
import robocupvision_amd
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import patches as P

# (frame Hs x Ws, map H x W or None = the frame's own size).  96 x 128 over 24 x 32: integer corners; 90 x 130 over 24 x 32: corners at
# multiples of 3.75 / 4.0625 -- not integers, and exact in fp32, the type Pillow parses ``box`` into
CONFIGS = {"96x128": ((96, 128), None), "96x128_map24x32": ((96, 128), (24, 32)), "90x130_map24x32": ((90, 130), (24, 32))}
SIZES = [(32, 32), (16, 24), (1, 1)]
FRAMES = {}


def _frame(Hs, Ws):
    if (Hs, Ws) not in FRAMES:
        FRAMES[(Hs, Ws)] = PR.seeded_frames(11, 1, Hs, Ws)[0]
    return FRAMES[(Hs, Ws)]


def _cases(H, W):
    """(x, y, w, h, margin): the edge boxes, a margin that clips on both sides of both axes, one that clips on one side, 40 seeded
    boxes (every fourth with a margin)."""
    rng = np.random.default_rng(H * 1000 + W)
    cases = [b + (0,) for b in PR.edge_boxes(H, W)]
    cases += [(1, 1, W - 2, H - 2, 3), (2, H - 6, 5, 4, 4), (6, 6, 4, 4, 2)]
    cases += [b + ((k % 4 == 0) * (1 + k % 3),) for k, b in enumerate(PR.random_boxes(rng, 40, H, W))]
    return cases


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
def test_restatement_equals_pillow_resize_box(cfg, size):
    (Hs, Ws), ms = CONFIGS[cfg]
    H, W = ms or (Hs, Ws)
    frame = _frame(Hs, Ws)
    shrink = 0.0
    for (x, y, w, h, margin) in _cases(H, W):
        mb = PR.map_box(x, y, w, h, margin, H, W)
        fb = PR.frame_box(mb, H, W, Hs, Ws)
        assert 0 <= fb[0] < fb[2] <= Ws and 0 <= fb[1] < fb[3] <= Hs
        ours, theirs = PR.resize_box(frame, fb, size), PR.pillow_resize_box(frame, fb, size)
        bad = np.argwhere(ours != theirs)
        assert bad.size == 0, "box %s margin %d -> %s: %d bytes differ, first %s: %d vs Pillow %d" % (
            (x, y, w, h), margin, fb, len(bad), bad[0].tolist(), ours[tuple(bad[0])], theirs[tuple(bad[0])])
        shrink = max(shrink, (fb[2] - fb[0]) / size[1], (fb[3] - fb[1]) / size[0])
    if size == (1, 1):
        assert shrink > 8            # the whole frame into one pixel: far beyond what the table-driven resize kernels admit
    if ms is None and size == (32, 32):
        assert PR.frame_box(PR.map_box(8, 9, 3, 5, 0, H, W), H, W, Hs, Ws) == (8.0, 9.0, 11.0, 14.0)      # 3 x 5 -> 32 x 32: an up-scale


def test_shrink_by_15_and_20_at_32x32():
    """The boxes of tests/test_gpu_patches.py's large-frame case: a 480 x 640 frame whole (a shrink by 15 / 20: 30 / 40 taps), a 5 x 5
    box and the two boxes whose source rows are exactly two 64-row chunks of the kernel."""
    frame = PR.seeded_frames(7, 1, 480, 640)[0]
    for box in ((0, 0, 640, 480), (317, 211, 5, 5), (100, 0, 200, 126), (100, 30, 200, 124)):
        fb = PR.frame_box(PR.map_box(*box, 0, 480, 640), 480, 640, 480, 640)
        assert np.array_equal(PR.resize_box(frame, fb, (32, 32)), PR.pillow_resize_box(frame, fb, (32, 32))), box
    _, xn, _ = PR.box_coeffs(640, 0.0, 640.0, 32)
    _, yn, _ = PR.box_coeffs(480, 0.0, 480.0, 32)
    assert (max(xn), max(yn)) == (40, 30)


def test_non_integer_corners_are_exercised():
    (Hs, Ws), (H, W) = CONFIGS["90x130_map24x32"]
    corners = [v for c in _cases(H, W) for v in PR.frame_box(PR.map_box(*c, H, W), H, W, Hs, Ws)]
    assert sum(1 for v in corners if v != int(v)) > 50
    assert all(float(np.float32(v)) == v for v in corners)


def test_box_coefficients_match_the_whole_axis_tables():
    """A box that is the whole axis gives the rows of ``data.bilinear_table`` (in0 = 0 adds nothing)."""
    from robocupvision_amd.data import bilinear_table
    for in_size, out_size in ((128, 32), (96, 16), (130, 24), (5, 32), (640, 32)):
        tab = bilinear_table(in_size, out_size)
        first, count, coef = PR.box_coeffs(in_size, 0.0, float(in_size), out_size)
        for xx in range(out_size):
            assert (first[xx], count[xx]) == (tab[xx, 0], tab[xx, 1]) and coef[xx] == tab[xx, 2:2 + count[xx]].tolist()
            assert count[xx] <= tab.shape[1] - 2


def test_map_box_clamps_whatever_the_row_holds():
    H, W = 24, 32
    assert PR.map_box(3, 4, 5, 6, 0, H, W) == (3, 4, 8, 10)
    assert PR.map_box(3, 4, 5, 6, 2, H, W) == (1, 2, 10, 12)
    assert PR.map_box(1, 1, 30, 22, 3, H, W) == (0, 0, 32, 24)                  # the margin clips on both sides
    assert PR.map_box(-7, -9, 3, 2, 0, H, W) == (0, 0, 1, 1)                    # left of the map: the first pixel
    assert PR.map_box(500, 600, 3, 2, 0, H, W) == (31, 23, 32, 24)              # right of it: the last pixel
    assert PR.map_box(5, 5, 0, -4, 0, H, W) == (5, 5, 6, 6)                     # empty / negative extent: one pixel
    assert PR.map_box(5, 5, 1 << 30, 1 << 30, 1 << 30, H, W) == (0, 0, 32, 24)
    assert PR.map_box(-(1 << 31), (1 << 31) - 1, (1 << 31) - 1, -(1 << 31), 0, H, W) == (0, 23, 1, 24)


def test_validity_zero_fill_margin_and_yuv_step():
    Hs, Ws, H, W = 96, 128, 24, 32
    frames = PR.seeded_frames(3, 2, Hs, Ws)
    rows, counts = PR.hand_built(H, W)
    N, Cm1, Mx, _ = rows.shape
    valid = PR.valid_slots(counts, Mx)
    assert valid.sum() == 15 and (~valid).sum() == 9 and valid[N - 1, Cm1 - 1].all() and counts[N - 1, Cm1 - 1, 3] > Mx
    for margin in (0, 2):
        images, byts, v = PR.object_patches(frames, rows, counts, (H, W), (32, 32), margin)
        pil = PR.object_patches(frames, rows, counts, (H, W), (32, 32), margin, resize=PR.pillow_resize_box)
        assert np.array_equal(v, valid) and np.array_equal(byts, pil[1]) and np.array_equal(images.view(np.uint32), pil[0].view(np.uint32))
        flat = valid.reshape(-1)
        assert not images[~flat].any() and not byts[~flat].any()
        assert all(byts[p].any() for p in np.flatnonzero(flat))
        for p in np.flatnonzero(flat)[:4]:
            n, c, k = np.unravel_index(p, valid.shape)
            fb = PR.frame_box(PR.map_box(*rows[n, c, k, 0:4], margin, H, W), H, W, Hs, Ws)
            assert np.array_equal(byts[p], PR.pillow_resize_box(frames[n], fb, (32, 32)))
            # step 4 of the RGB loader on the resized bytes: an image of the patch's own size takes no resize there
            img, _ = RP.prepare_image(byts[p], None, (32, 32))
            assert np.array_equal(images[p].view(np.uint32), img.view(np.uint32))
            assert np.array_equal(images[p].view(np.uint32), RP.to_yuv(byts[p]).view(np.uint32))
    with_margin = PR.object_patches(frames, rows, counts, (H, W), (32, 32), 2)[1]
    assert not np.array_equal(with_margin, PR.object_patches(frames, rows, counts, (H, W), (32, 32), 0)[1])
    # the default map is the frame itself
    a = PR.object_patches(frames, rows, counts, None, (16, 24))
    b = PR.object_patches(frames, rows, counts, (Hs, Ws), (16, 24))
    assert a[0].shape == (24, 3, 16, 24) and a[1].shape == (24, 16, 24, 3) and np.array_equal(a[1], b[1])


# ---- the record ----
def _record(N=2, Hs=96, Ws=128, Cm1=4, Mx=3, map_size=(24, 32), size=(32, 32), margin=0):
    return P.PatchesRecord(N, Hs, Ws, Cm1, Mx, map_size, size, margin)


def test_record_plans_without_workspace():
    h = L.planner_handle(256)
    rec = _record()
    assert L.op_workspace(h, rec.op) == 0 and rec.op.i[L.RCV_I_NPART] == 0
    assert L.OpList([rec.op]).labels(h)[0] == "object_patches<4>"
    assert L.OpList([_record(size=(64, 64)).op]).labels(h)[0] == "object_patches<16>"
    assert L.OpList([_record(size=(32, 33)).op]).labels(h)[0] == "object_patches<16>"
    for kw in (dict(Hs=1080, Ws=1920, map_size=(270, 480)), dict(Hs=1080, Ws=1920, map_size=None, size=(1, 1)), dict(size=(64, 64)),
               dict(size=(1, 64)), dict(map_size=None), dict(map_size=(96, 128)), dict(map_size=(1, 1)), dict(N=1, Cm1=1, Mx=1),
               dict(margin=(1 << 31) - 1), dict(Hs=2160, Ws=3840, map_size=(2160, 3840), size=(64, 64))):
        _record(**kw).check(h)
    with pytest.raises(L.RcvError, match="planning-only"):
        L.OpList([rec.op]).run(h, 0)


REFUSALS = {
    "no_frames": (dict(N=0), "every count"), "no_rows": (dict(Mx=0), "every count"), "no_classes": (dict(Cm1=0), "every count"),
    "size_0": (dict(size=(0, 32)), "patch size"), "size_65": (dict(size=(32, 65)), "patch size"), "size_neg": (dict(size=(-1, 32)), "patch size"),
    "margin_neg": (dict(margin=-1), "margin"),
    "map_taller": (dict(map_size=(97, 32)), "does not fit"), "map_wider": (dict(map_size=(24, 129)), "does not fit"),
    "map_0": (dict(map_size=(0, 32)), "does not fit"), "map_neg": (dict(map_size=(24, -3)), "does not fit"),
    "frame_0": (dict(Hs=0, map_size=(1, 1)), "every size"),
    "products": (dict(Hs=96, Ws=46341, map_size=(24, 46341)), "32 bits"), "products_y": (dict(Hs=65536, Ws=128, map_size=(32768, 32)), "32 bits"),
    "slots": (dict(N=1 << 20, Cm1=1 << 6, Mx=1 << 5), "2\\^31"),
    "tables_x": (dict(Hs=96, Ws=1 << 20, size=(32, 64)), "LDS"), "tables_y": (dict(Hs=1 << 22, Ws=128, size=(1, 1), map_size=(24, 32)), "LDS"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_record_refusals_at_query_and_at_launch(name):
    kw, text = REFUSALS[name]
    h = L.planner_handle(256)
    rec = _record(**kw)
    with pytest.raises(L.RcvError, match=text) as at_query:
        rec.check(h)
    assert "planning-only" not in str(at_query.value)
    buf = ctypes.create_string_buffer(64)
    assert L.load().rcv_op_kernel_label(h, ctypes.byref(rec.op), buf, 64) != 0


def test_named_entry_refuses_like_the_record():
    lib, h = L.load(), L.planner_handle(256)
    assert "rcv_object_patches" in L.EXPORTS and L.OP_OBJECT_PATCHES == 50
    rc = lib.rcv_object_patches(h, None, 2, 96, 128, None, None, 5, 3, 24, 32, 32, 65, 0, None, None, None)
    assert rc != 0 and b"patch size" in lib.rcv_last_error()
    rc = lib.rcv_object_patches(h, None, 2, 96, 128, None, None, 1, 3, 24, 32, 32, 32, 0, None, None, None)      # C = 1: no class has boxes
    assert rc != 0 and b"every count" in lib.rcv_last_error()
    rc = lib.rcv_object_patches(h, None, 2, 96, 128, None, None, 5, 3, 24, 32, 32, 32, 0, None, None, None)
    assert rc != 0 and b"planning-only" in lib.rcv_last_error()


# ---- the Python surface ----
def _cpu_inputs(N=2, Hs=96, Ws=128, Cm1=4, Mx=3):
    return (torch.zeros(N, Hs, Ws, 3, dtype=torch.uint8), torch.zeros(N, Cm1, Mx, 8, dtype=torch.int32), torch.zeros(N, Cm1, 4, dtype=torch.int32))


def test_object_patches_refuses_cpu_tensors_and_bad_arguments():
    frames, rows, counts = _cpu_inputs()
    with pytest.raises(L.RcvError, match="HIP device"):
        P.object_patches(frames, (rows, counts), map_size=(24, 32))
    with pytest.raises(L.RcvError, match="HIP device"):
        robocupvision_amd.object_patches(frames, I.Objects(rows, counts))
    with pytest.raises(L.RcvError, match="HIP device"):
        robocupvision_amd.classify_objects(frames, (rows, counts), torch.nn.Identity(), map_size=(24, 32))
    for bad, text in ((dict(size=(0, 32)), "patch size"), (dict(size=(32, 65)), "patch size"), (dict(margin=-1), "margin"),
                      (dict(map_size=(97, 128)), "does not fit"), (dict(map_size=(0, 0)), "does not fit"), (dict(size=32), "pair"),
                      (dict(size=(32, 32, 3)), "pair"), (dict(size=(32.5, 32)), "integer"), (dict(margin=1.5), "integer"),
                      (dict(margin="wide"), "integer"), (dict(map_size=(24,)), "pair"), (dict(margin=1 << 31), "32 bits"),
                      (dict(size=(True, 32)), "integer")):
        with pytest.raises(L.RcvError, match=text) as e:
            P.object_patches(frames, (rows, counts), **bad)
        assert "HIP device" not in str(e.value), bad              # refused for the argument, with the library's message
    with pytest.raises(TypeError, match="tensors"):
        P.object_patches(frames.numpy(), (rows, counts))
    with pytest.raises(TypeError, match="Objects"):
        P.object_patches(frames, rows)
    with pytest.raises(TypeError, match="uint8"):
        P.object_patches(frames.float(), (rows, counts))
    with pytest.raises(TypeError, match="int32"):
        P.object_patches(frames, (rows.long(), counts))
    with pytest.raises(TypeError, match="int32"):
        P.object_patches(frames, (rows, counts.long()))
    for f, r, c in ((frames[0], rows, counts), (frames[..., :2], rows, counts), (frames, rows[..., :7], counts), (frames, rows, counts[..., :3]),
                    (frames, rows[0], counts), (frames[:1], rows, counts), (frames, rows, counts[:, :3]), (frames, rows[:, :3], counts)):
        with pytest.raises(ValueError):
            P.object_patches(f, (r, c))
    with pytest.raises(TypeError):
        P.object_patches(frames, (rows, counts), colour=True)


def test_valid_is_device_arithmetic_on_counts():
    rows, counts = PR.hand_built(24, 32)
    p = P.Patches(None, None, torch.from_numpy(counts), rows.shape[:3])
    assert p.valid.dtype == torch.bool and np.array_equal(p.valid.numpy(), PR.valid_slots(counts, 3)) and p.shape_nkm == (2, 4, 3)


def test_package_exports():
    for name in ("object_patches", "classify_objects", "classify_patches", "Patches"):
        assert getattr(robocupvision_amd, name) is getattr(P, name)
    assert robocupvision_amd.patches is P and P.NO_OBJECT == 255


def test_segmenter_refuses_wrong_patch_keywords_at_construction():
    from robocupvision_amd.bnn import BNNMC
    net = M.ROBO_UNet()
    seg = robocupvision_amd.Segmenter(net, img_size=(24, 32), objects=I.DBCONVERT, patches={}, classifier=BNNMC().train())
    assert seg._patches == {} and seg._classifier.training is False
    assert robocupvision_amd.Segmenter(net, objects=I.DBCONVERT, patches=dict(size=(16, 24), margin=2, return_bytes=True))._patches["margin"] == 2
    plain = robocupvision_amd.Segmenter(net, objects=I.DBCONVERT)
    assert plain._patches is None and plain._classifier is None
    with pytest.raises(L.RcvError, match="needs objects"):
        robocupvision_amd.Segmenter(net, patches={})
    with pytest.raises(L.RcvError, match="needs patches"):
        robocupvision_amd.Segmenter(net, objects=I.DBCONVERT, classifier=BNNMC())
    with pytest.raises(TypeError, match="module"):
        robocupvision_amd.Segmenter(net, objects=I.DBCONVERT, patches={}, classifier="bnn")
    for bad in (dict(size=(0, 32)), dict(size=(65, 32)), dict(margin=-1), dict(margin=0.5), dict(size=32), dict(map_size=(24, 32)),
                dict(colour=True), [("size", (32, 32))], "size"):
        with pytest.raises(L.RcvError):
            robocupvision_amd.Segmenter(net, img_size=(24, 32), objects=I.DBCONVERT, patches=bad)
    for s in (seg, plain):                       # CPU frames are refused as before
        with pytest.raises(L.RcvError, match="HIP device"):
            s(torch.zeros(1, 96, 128, 3, dtype=torch.uint8))
