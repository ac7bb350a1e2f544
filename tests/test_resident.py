"""CPU: the device-resident dataset (RCV_OP_RESIZE_U8, RCV_OP_BATCH_PREP_IDX, ``ResidentDataset`` / ``EpochLoader`` of
robocupvision_amd/data.py) -- the restatement of the two records (tests/resident_restatement.py) against live Pillow and against the
batch restatement, the plan-time refusals on the planner handle, ``draw_jitter_rows`` against ``draw_jitter`` bit for bit, and the
epoch bookkeeping (``EpochLoader.plan``), none of which needs a device."""
import ctypes
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT
import batch_prep_restatement as R
import resident_restatement as RR
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("src,size", RR.SHAPES)
def test_resize_u8_restatement_equals_pillow(src, size):
    frames, labels = R.synthetic_frames(2, src[0], src[1], 11, full_range_labels=True, cover_size=size)
    got, got_l = RR.resize_u8(frames, labels, size)
    assert got.dtype == np.uint8 and got.shape == (2,) + size + (3,) and got_l.shape == (2,) + size
    for b in range(2):
        want = np.asarray(Image.fromarray(frames[b]).resize((size[1], size[0]), Image.BILINEAR))
        want_l = np.asarray(Image.fromarray(labels[b].astype(np.uint8)).convert("I").resize((size[1], size[0]), Image.NEAREST))
        assert int((got[b] != want).sum()) == 0 and int((got_l[b] != want_l).sum()) == 0
        assert len(np.unique(got_l[b])) == min(256, size[0] * size[1])          # every label value 0..255 reaches an output that has room
    # ... and it is the resize stage of the batch restatement: the batch made from the bytes is the batch made from the frames
    a = R.prepare_batch(frames, labels, size, train=False)
    b = R.prepare_batch(got, got_l, size, train=False)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    assert RR.resize_u8(frames, None, size)[1] is None and RR.resize_u8(frames, labels, size, np.uint8)[1].dtype == np.uint8


@pytest.mark.parametrize("src,size", [RR.SHAPES[0], RR.SHAPES[3]])
@pytest.mark.parametrize("train", [False, True])
def test_indexed_restatement_equals_batch_restatement_on_the_gathered_store(src, size, train):
    frames, labels = R.synthetic_frames(5, src[0], src[1], 21)
    flags = (True, False, True, False)
    for index in ([4, 3, 2, 1, 0], [1, 1, 4, 1], [0, 4, 2, 2, 3, 1, 0, 4, 4], [3]):
        random.seed(len(index))
        torch.manual_seed(len(index))
        rows = D.draw_jitter(len(index)).numpy() if train else None
        gi, gt, bad = RR.prepare_batch_indexed(frames, labels, index, size, train=train, params=rows, flags=flags)
        wi, wt = R.prepare_batch(frames[index], labels[index], size, train=train, params=rows, flags=flags)
        assert bad == 0 and np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gt, wt)
    gi, gt, bad = RR.prepare_batch_indexed(frames, labels, [0, 5, -1, 2], size, flags=flags)
    wi, wt = R.prepare_batch(frames[[0, 2]], labels[[0, 2]], size, flags=flags)
    assert bad == 2 and not gi[1:3].any() and not gt[1:3].any()
    assert np.array_equal(_bits(gi[[0, 3]]), _bits(wi)) and np.array_equal(gt[[0, 3]], wt)


def _taps(n_in, n_out):
    return D.bilinear_table(n_in, n_out).shape[1] - 2


def _rec_resize(B=64, Hs=480, Ws=640, H=120, W=160, lab=4, out=1, tables=True, kx=None, ky=None):
    t = 64 if tables else 0          # (a planner handle never reads through a pointer)
    return L.make_op(L.OP_RESIZE_U8, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, inmode2=lab, inmode=out, p_x1=t, p_x2=t, p_x3=t if lab else 0,
                     p_x4=t if lab else 0)


def _rec_indexed(B=64, N=4096, Hs=120, Ws=160, H=120, W=160, lab=1, train=1, mask=0, tables=True, kx=None, ky=None, idx=8, index=64,
                 counter=64):
    t = 64 if tables else 0
    return L.make_op(L.OP_BATCH_PREP_IDX, n=B, count=N, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, inmode2=lab, inmode=idx, aux0=train, aux1=mask, p_x1=t, p_x2=t, p_x3=t, p_x4=t,
                     p_x5=t, p_in_aux=index, p_epi_aux=counter)


def test_plan_on_the_planner_handle():
    h = L.planner_handle(256)
    for lab in (0, 1, 4):
        for out in (1, 4):
            for H, W in ((120, 160), (480, 640)):
                op = L.OpList([_rec_resize(H=H, W=W, lab=lab, out=out)])
                assert L.op_workspace(h, op.arr[0]) == 0 and op.labels(h) == ["resize_u8"]
    for lab in (1, 4):
        for idx in (4, 8):
            for Hs, Ws in ((120, 160), (480, 640)):
                for train in (0, 1):
                    op = L.OpList([_rec_indexed(Hs=Hs, Ws=Ws, lab=lab, idx=idx, train=train, mask=5)])
                    assert L.op_workspace(h, op.arr[0]) == 0 and op.labels(h) == ["batch_prep_idx"]
    assert L.op_workspace(h, _rec_indexed(B=9, N=5)) == 0          # more rows than the store has images
    for rec in (_rec_resize(), _rec_indexed()):
        with pytest.raises(L.RcvError, match="planning-only handle"):
            L.OpList([rec]).run(h, 0)


@pytest.mark.parametrize("rec,kw,msg", [
    # what rcv_batch_prep refuses, on both records
    (_rec_resize, dict(B=0), "every size must be >= 1"), (_rec_resize, dict(H=0, ky=3), "every size must be >= 1"),
    (_rec_resize, dict(H=59, ky=19), "shrinks an axis by more than 8"), (_rec_resize, dict(lab=2), "label element size 2 unsupported"),
    (_rec_resize, dict(tables=False), "null table"), (_rec_resize, dict(kx=7), "taps per column / row"),
    (_rec_resize, dict(B=1 << 14, Hs=480, Ws=640), "more than 2\\^31 pixels"),
    (_rec_indexed, dict(B=0), "every size must be >= 1"), (_rec_indexed, dict(Ws=0, kx=3), "every size must be >= 1"),
    (_rec_indexed, dict(Hs=480, Ws=640, W=79, kx=19), "shrinks an axis by more than 8"), (_rec_indexed, dict(lab=8), "label element size 8 unsupported"),
    (_rec_indexed, dict(tables=False), "null table"), (_rec_indexed, dict(ky=5), "taps per column / row"),
    (_rec_indexed, dict(mask=16), "maskLabel flags 16 out of range"), (_rec_indexed, dict(N=1 << 17), "more than 2\\^31 pixels"),
    # their own
    (_rec_indexed, dict(N=0), "a store of 0 images"), (_rec_indexed, dict(N=-3), "a store of -3 images"),
    (_rec_indexed, dict(idx=2), "index element size 2 unsupported"), (_rec_indexed, dict(idx=0), "index element size 0 unsupported"),
    (_rec_indexed, dict(index=0), "null index or null bad-index counter"), (_rec_indexed, dict(counter=0), "null index or null bad-index counter"),
    (_rec_resize, dict(out=2), "label element size out 2 cannot hold"), (_rec_resize, dict(lab=1, out=0), "label element size out 0 cannot hold"),
    (_rec_resize, dict(out=8), "label element size out 8 cannot hold"),
])
def test_plan_time_refusals(rec, kw, msg):
    h = L.planner_handle(256)
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(h, rec(**kw))
    assert L.op_workspace(h, rec()) == 0


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/rcv.h").read(), flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("rcv_resize_u8", "rcv_batch_prep_indexed"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTS and getattr(L.load(), name).argtypes
    assert re.search(r"RCV_OP_RESIZE_U8\s*=\s*%d\b" % L.OP_RESIZE_U8, src) and re.search(r"RCV_OP_BATCH_PREP_IDX\s*=\s*%d\b" % L.OP_BATCH_PREP_IDX, src)
    for name in ("resize_u8", "draw_jitter_rows", "ResidentDataset", "EpochLoader"):
        assert getattr(robocupvision_amd, name) is getattr(D, name) and name in D.__all__


@pytest.mark.parametrize("seeds", [(1, 1), (7, 12345), (20261020, 3)])
def test_draw_jitter_rows_equals_draw_jitter(seeds):
    def seeded(fn):
        random.seed(seeds[0])
        torch.manual_seed(seeds[1])
        rows = fn(257)
        return rows, fn(1), random.random(), torch.rand(1).item()          # the rows, and where both generators were left

    a, b = seeded(D.draw_jitter), seeded(D.draw_jitter_rows)
    assert b[0].dtype == torch.float32 and tuple(b[0].shape) == (257, 8) and b[0].device.type == "cpu"
    assert np.array_equal(_bits(a[0].numpy()), _bits(b[0].numpy())) and np.array_equal(_bits(a[1].numpy()), _bits(b[1].numpy()))
    assert a[2] == b[2] and a[3] == b[3]
    assert 0 < int(b[0][:, 0].sum()) < 257 and bool((b[0][:, 7] == 0).all())
    random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    off = D.draw_jitter_rows(5, h=0.0)
    random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    assert np.array_equal(_bits(off.numpy()), _bits(D.draw_jitter(5, h=0.0).numpy())) and bool((off[:, 7] == 1).all())
    assert tuple(D.draw_jitter_rows(0).shape) == (0, 8)


class _Store:          # what EpochLoader's bookkeeping asks of a store: its length
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_epoch_loader_plan():
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(4))
    ld = D.EpochLoader(_Store(10), 4)
    assert ld.plan(perm) == [(0, 4), (4, 8), (8, 10)] and len(ld) == 3 and torch.equal(ld.share(perm), perm)
    visited = torch.cat([ld.share(perm)[a:b] for a, b in ld.plan(perm)])
    assert torch.equal(visited, perm)                                   # the permutation once, in order
    ld = D.EpochLoader(_Store(10), 4, drop_last=True)
    assert ld.plan(perm) == [(0, 4), (4, 8)] and len(ld) == 2
    parts = []
    for rank in (0, 1):
        ld = D.EpochLoader(_Store(10), 4, rank=rank, world=2)
        assert ld.plan(perm) == [(0, 4), (4, 5)] and len(ld) == 2
        assert torch.equal(ld.share(perm), perm[rank::2])
        parts.append(torch.cat([ld.share(perm)[a:b] for a, b in ld.plan(perm)]))
        assert D.EpochLoader(_Store(10), 4, rank=rank, world=2, drop_last=True).plan(perm) == [(0, 4)]
    assert sorted(torch.cat(parts).tolist()) == list(range(10)) and len(set(parts[0].tolist()) & set(parts[1].tolist())) == 0
    # uneven shares, an exact multiple, fewer samples than ranks
    assert [len(D.EpochLoader(_Store(10), 4, rank=r, world=3)) for r in range(3)] == [1, 1, 1]
    assert [D.EpochLoader(_Store(10), 2, rank=r, world=3).plan(perm) for r in range(3)] == [[(0, 2), (2, 4)], [(0, 2), (2, 3)], [(0, 2), (2, 3)]]
    assert D.EpochLoader(_Store(8), 4).plan(perm[:8]) == [(0, 4), (4, 8)] and len(D.EpochLoader(_Store(8), 4, drop_last=True)) == 2
    assert D.EpochLoader(_Store(1), 4, rank=1, world=2).plan(perm[:1]) == [] and len(D.EpochLoader(_Store(1), 4, rank=1, world=2)) == 0
    for kw in (dict(batch_size=0), dict(batch_size=4, rank=2, world=2), dict(batch_size=4, world=0)):
        with pytest.raises(ValueError):
            D.EpochLoader(_Store(10), **kw)


def test_python_refusals():
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    lab = torch.zeros(2, 24, 32, dtype=torch.int32)
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.resize_u8(f, lab, (12, 16))                                   # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.resize_u8(f, lab, (24, 16))                                   # exactly one axis kept
    with pytest.raises(TypeError):
        D.resize_u8(f, lab.long(), (12, 16))
    with pytest.raises(TypeError):
        D.resize_u8(f, lab, (12, 16), label_dtype=torch.int64)
    with pytest.raises(ValueError):
        D.resize_u8(f, lab[:1], (12, 16))
    with pytest.raises(ValueError):
        D.ResidentDataset.from_tensors(f, lab[:1], (12, 16))
