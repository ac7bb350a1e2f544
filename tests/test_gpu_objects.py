"""GPU: RCV_OP_OBJECTS (csrc/objects.hip) against the numpy restatement of the contract (tests/objects_restatement.py), bitwise: the
hand-written known answers, seeded blob and jittered maps at every shape class, adversarial planes for the union-find and for select,
both kernel forms (general / single-launch LDS) byte for byte, the routing boundary, the zero fill, the named entry point, the
component counts of RCV_OP_OBJECT_MATCH, and Segmenter(objects=...)."""
import ctypes

import numpy as np
import pytest
import torch

import objdet_restatement as R
import objects_restatement as OR
import robocupvision_amd
from test_gpu_objdet import _grid, _serpentine, _spiral
from test_objects import KNOWN_ANSWERS
from robocupvision_amd import _lib as L
from robocupvision_amd import infer as I
from robocupvision_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_MAX_BLOCKS = 7680        # 2x2 blocks per plane the single-launch form takes (a 120 x 256 plane)


def _device(maps, C, min_area=0, min_ratio=0.0, max_objects=8, dtype=torch.uint8, form=0):
    t = torch.from_numpy(np.ascontiguousarray(maps)).to(dtype).to(DEV)
    o = I.find_objects(t, C, min_area, min_ratio, max_objects, _form=form)
    torch.cuda.synchronize()
    return o.rows.cpu().numpy().astype(np.int64), o.counts.cpu().numpy().astype(np.int64)


def _check(maps, C, min_area=0, min_ratio=0.0, max_objects=8, dtype=torch.uint8, ref=None):
    """Every form the plane admits (the library's route, general, LDS) against the restatement, bitwise; returns the reference."""
    maps = np.asarray(maps)
    ref = ref or OR.find_objects(maps, C, min_area, min_ratio, max_objects)
    fits = ((maps.shape[1] + 1) // 2) * ((maps.shape[2] + 1) // 2) <= LDS_MAX_BLOCKS
    for form in (0, 1, 2) if fits else (0, 1):
        rows, counts = _device(maps, C, min_area, min_ratio, max_objects, dtype, form)
        assert rows.shape == ref[0].shape and counts.shape == ref[1].shape
        bad = np.argwhere(counts != ref[1])
        assert bad.size == 0, "form %d counts, first mismatches (n, c-1, slot): %s; device %s vs %s" % (
            form, bad[:4].tolist(), [int(counts[tuple(b)]) for b in bad[:4]], [int(ref[1][tuple(b)]) for b in bad[:4]])
        bad = np.argwhere(rows != ref[0])
        assert bad.size == 0, "form %d rows, first mismatches (n, c-1, row, col): %s; device %s vs %s" % (
            form, bad[:4].tolist(), [int(rows[tuple(b)]) for b in bad[:4]], [int(ref[0][tuple(b)]) for b in bad[:4]])
    return ref


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("case", KNOWN_ANSWERS, ids=[c[0] for c in KNOWN_ANSWERS])
def test_known_answers(case, dtype):
    _, maps, C, min_area, min_ratio, cap, rows, counts = case
    _check(maps, C, min_area, min_ratio, cap, dtype, ref=(np.array(rows), np.array(counts)))


@pytest.mark.parametrize("N,H,W,seed", [(8, 120, 160, 1), (3, 37, 53, 2), (1, 5, 7, 3), (1, 1, 1, 4), (2, 2, 3, 5), (1, 240, 320, 6),
                                        (1, 480, 640, 7), (64, 24, 32, 8)])      # 64 images: the library's own route is the LDS form
def test_blob_maps(N, H, W, seed):
    rng = np.random.default_rng(seed)
    maps = R.blob_masks(rng, N, H, W, 5, n_blobs=20)
    if H * W == 1:
        maps[:] = 3
    ref = _check(maps, 5, max_objects=8)
    if H * W > 30:
        assert ref[1][:, :, 3].sum() > 0
    _check(maps, 5, **{k: v for k, v in I.DBCONVERT.items() if k != "num_class"})


@pytest.mark.parametrize("M_", [16, 1])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_jittered_maps(M_, dtype):
    rng = np.random.default_rng(20 + M_)
    maps = R.jitter(rng, R.blob_masks(rng, 3, 120, 160, 5), 5, p=0.02)
    if dtype == torch.int64:
        maps[0, 0, :7] = [9, -1, -200, 5, 255, 300, 1 << 40]       # background: values >= C, negative, above 8 bits
    ref = _check(maps, 5, max_objects=M_, dtype=dtype)
    assert (ref[1][:, :, 0] > 16).all() and (ref[1][:, :, 3] == M_).all()       # more components than rows: the cap decides
    _check(maps, 5, min_area=(1, 2, 0, 3), min_ratio=(0.01, 0.5, 1.0, 0.0), max_objects=(M_, 1, M_, 0) if M_ > 1 else 1, dtype=dtype)


@pytest.mark.parametrize("C", [2, 8])
def test_class_counts(C):
    rng = np.random.default_rng(30 + C)
    maps = R.jitter(rng, R.blob_masks(rng, 2, 40, 56, C, n_blobs=25), C, p=0.03)
    maps[1, 3, :4] = [C, 255, 0, C - 1]
    _check(maps, C, min_area=1, min_ratio=0.1, max_objects=5)


def test_adversarial_planes():
    """Long find chains (serpentine, spiral), and thousands of equal-area components through select (the stride-2 grid: 4 800)."""
    H, W = 120, 160
    spiral = np.zeros((H, W), dtype=np.int64)
    spiral[:, :H] = _spiral(H)
    checker = ((np.add.outer(np.arange(H), np.arange(W)) % 2) + 1).astype(np.int64)
    big = _grid(H, W)
    big[100:, 100:] = 1                                         # one blob larger than the 4 000-odd pixels around it
    maps = np.stack([_serpentine(H, W), spiral, checker, np.ones((H, W), dtype=np.int64), _grid(H, W), _grid(H, W, 1) * 2, big])
    ref = _check(maps, 3, max_objects=16)
    assert ref[1][0, 0].tolist() == [1, 1, 1, 1] and ref[1][4, 0].tolist() == [4800, 4800, 4800, 16]
    assert ref[0][4, 0, :, 5].tolist() == list(range(16))                      # equal areas: the first sixteen ranks
    assert ref[1][5, 1, 0] == 4800 and ref[0][6, 0, 0, 4] > 1
    ref = _check(maps, 3, min_area=1, min_ratio=0.5, max_objects=(16, 3))
    assert ref[1][4, 0].tolist() == [4800, 0, 0, 0] and ref[1][6, 0, 1:].tolist() == [1, 1, 1]


def test_routing_boundary():
    """The largest plane the single-launch form takes (120 x 256: 7680 2x2 blocks, 30 tiles) and one row of blocks more."""
    rng = np.random.default_rng(41)
    h = L.handle(0)
    for H, lds in ((120, True), (122, False)):
        maps = R.jitter(rng, R.blob_masks(rng, 1, H, 256, 5, n_blobs=20), 5, p=0.01)
        maps[0, H - 1, 250:] = 4                                # something in the last tile
        ref = _check(maps, 5, max_objects=16)
        assert ref[1][0, :, 0].min() > 0
        rec = I.ObjectsRecord(64, H, 256, 5)                    # the route of a batch of 64 such planes
        assert L.OpList([rec.op]).labels(h)[0] == ("objects<u8,lds>" if lds else "objects<u8>")
    with pytest.raises(L.RcvError, match="does not fit the lds form"):
        I.find_objects(torch.zeros(1, 122, 256, dtype=torch.uint8, device=DEV), _form=2)


def test_op_list_and_named_entry_point_agree_and_zero_fill():
    rng = np.random.default_rng(51)
    N, H, W, C, Mx = 4, 64, 96, 5, 8
    maps = torch.from_numpy(R.blob_masks(rng, N, H, W, C, n_blobs=20)).to(torch.uint8).to(DEV)
    a = I.find_objects(maps, C, 2, 0.05, Mx)
    b = I.find_objects(maps, C, 2, 0.05, Mx)
    h = L.handle(0)
    lib = L.load()
    area, ratio, cap = (ctypes.c_int32 * 4)(*[2] * 4), (ctypes.c_double * 4)(*[0.05] * 4), (ctypes.c_int32 * 4)(*[Mx] * 4)
    stream = torch.cuda.current_stream().cuda_stream
    for form in (1, 2):
        rec = I.ObjectsRecord(N, H, W, C, 2, 0.05, Mx, 1, form)
        ws = torch.empty(rec.workspace_bytes(h), dtype=torch.uint8, device=DEV)
        rows = torch.full_like(a.rows, -1)                      # 0xFF in every byte
        counts = torch.full_like(a.counts, -1)
        op = rec.op
        op.p[L.RCV_P_IN], op.p[L.RCV_P_OUT], op.p[L.RCV_P_X0], op.p[L.RCV_P_PART] = maps.data_ptr(), rows.data_ptr(), counts.data_ptr(), ws.data_ptr()
        L.OpList([op]).run(h, stream)
        torch.cuda.synchronize()
        assert torch.equal(rows, a.rows) and torch.equal(counts, a.counts)
    assert (a.counts[..., 3] < Mx).any()                        # some rows are fill
    ws = torch.empty(I.ObjectsRecord(N, H, W, C).workspace_bytes(h), dtype=torch.uint8, device=DEV)
    rows, counts = torch.full_like(a.rows, -1), torch.full_like(a.counts, -1)
    L.check(lib.rcv_find_objects(h, maps.data_ptr(), 1, N, C, H, W, area, ratio, cap, Mx, rows.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                 ws.numel(), stream), "rcv_find_objects")
    torch.cuda.synchronize()
    assert torch.equal(a.rows, b.rows) and torch.equal(a.counts, b.counts)
    assert torch.equal(a.rows, rows) and torch.equal(a.counts, counts)
    with pytest.raises(L.RcvError, match="workspace"):
        L.check(lib.rcv_find_objects(h, maps.data_ptr(), 1, N, C, H, W, area, ratio, cap, Mx, rows.data_ptr(), counts.data_ptr(),
                                     ws.data_ptr(), 1024, stream), "rcv_find_objects")
    with pytest.raises(L.RcvError, match="cap of class"):      # a refusal of the query is a refusal of the launch
        cap[2] = Mx + 1
        L.check(lib.rcv_find_objects(h, maps.data_ptr(), 1, N, C, H, W, area, ratio, cap, Mx, rows.data_ptr(), counts.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream), "rcv_find_objects")


def test_component_counts_equal_object_match():
    rng = np.random.default_rng(61)
    C = 5
    maps = R.jitter(rng, R.blob_masks(rng, 4, 60, 80, C, n_blobs=15), C, p=0.02)
    t = torch.from_numpy(maps).to(torch.uint8).to(DEV)
    n_pred = M.object_match_counts(t, t, C)[:, :, 0]
    assert torch.equal(I.find_objects(t, C).counts[:, :, 0], n_pred) and int(n_pred.sum()) > 0


def test_views_and_to_list_on_the_device():
    _, maps, C, min_area, min_ratio, cap, rows, counts = KNOWN_ANSWERS[9]          # background_values
    o = robocupvision_amd.find_objects(torch.from_numpy(maps).to(DEV), C, min_area, min_ratio, cap)
    assert o.to_list() == [[(1, 0, 0, 1, 1, 1), (1, 2, 0, 1, 1, 1), (2, 4, 0, 1, 1, 1)]]
    assert o.count.tolist() == [[2, 1]] and o.centres[0, 0].tolist() == [[0.5, 0.5], [2.5, 0.5]]
    assert o.boxes.data_ptr() == o.rows.data_ptr()


def test_segmenter_objects_on_a_seeded_unet():
    import robocupvision_amd.model as Mo
    torch.manual_seed(2024)
    net = Mo.ROBO_UNet().to(DEV)
    rng = np.random.default_rng(71)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8)).to(DEV)
    labels, colour, objs = robocupvision_amd.Segmenter(net, objects=I.DBCONVERT)(frames)
    two = robocupvision_amd.Segmenter(net)(frames)
    assert len(two) == 2 and torch.equal(two[0], labels) and torch.equal(two[1], colour)
    again = I.find_objects(labels, **I.DBCONVERT)
    torch.cuda.synchronize()
    assert torch.equal(objs.rows, again.rows) and torch.equal(objs.counts, again.counts)
    rules = {k: v for k, v in I.DBCONVERT.items() if k != "num_class"}
    ref = OR.find_objects(labels.cpu().numpy(), 5, rules["min_area"], rules["min_ratio"], rules["max_objects"])
    assert np.array_equal(objs.rows.cpu().numpy(), ref[0]) and np.array_equal(objs.counts.cpu().numpy(), ref[1])
    assert objs.rows.shape == (2, 4, 6, 8) and (objs.counts[:, 3, 3] == 0).all()
