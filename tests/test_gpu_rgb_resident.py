"""GPU: the RGB loader and LabelProp frame pairs from the device-resident store -- ``prepare_rgb_batch(index=)`` (RCV_OP_RGB_PREP_IDX)
against ``prepare_rgb_batch`` of the gathered store and ``prepare_lp_pairs`` (RCV_OP_LP_PAIR_PREP) against ``labelprop_batch`` of
``prepare_rgb_batch`` of the gathered frames with every row repeated, ``torch.equal`` on every output; the defined result of an index
outside the store; one configuration per record against the NumPy restatement, every element; ``ResidentDataset`` + ``RGBEpochLoader``
against ``prepare_rgb_batch`` of the FULL-SIZE frames; ``LPEpochLoader`` against ``prepare_lp_pairs``; and one batch of each through a
training step.  The shapes cross the 8-row x 64-column tile on both sides of the tap count from which the kernel stages its source
rows in LDS, and the 2048-pixel workgroup of the no-resize form with a ragged second workgroup.  Every bar is equality."""
import functools
import random

import numpy as np
import pytest
import torch

import rgb_prep_restatement as R
import rgb_resident_restatement as RG
import robocupvision_amd.model as M
from robocupvision_amd import data as D
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAG_SETS = [(False, False, False, False), (True, False, True, False)]          # (no_ball, no_robot, no_goal, no_line)
# store (Hs, Ws) -> (H, W): staged, across a column tile and a row tile; through the cache; no resize, 2590 pixels = 2048 + 542
STORES = {"staged": ((44, 280), (11, 70)), "cache": ((22, 140), (11, 70)), "ident": ((37, 70), (37, 70))}
INDEX_VARIANTS = [("reversed", [4, 3, 2, 1, 0]), ("repeats", [1, 1, 4, 1]), ("B > N", [0, 4, 2, 2, 3, 1, 0, 4, 4]), ("B = 1", [3]), ("slice", None)]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(a, b):
    return torch.equal(a, b) and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _store(kind, wide_labels):
    """N = 5 images on the device (uint8 or int32 labels); made once, never written."""
    src = STORES[kind][0]
    frames, labels = R.synthetic_frames(5, src[0], src[1], 21)
    return torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(torch.int32 if wide_labels else torch.uint8).to(DEV)


def _rows(B, seed, contrast=True):
    """Rows that hold all four operations in drawn orders and factors, both flips mixed over the rows; with ``contrast`` at least one
    row WITHOUT a contrast next to one with (B >= 2); without it no row holds one."""
    random.seed(seed)
    np.random.seed(seed)
    rows = D.draw_color_jitter_rows(B).numpy() if contrast else D.draw_color_jitter_rows(B, contrast=0.0).numpy()
    rows[:, 0] = np.arange(B) % 2
    rows[:, 1] = (np.arange(B) // 2) % 2
    if contrast and B >= 2:
        rows[1] = R.make_row([R.OP_HUE, R.OP_BRIGHTNESS, R.OP_SATURATION], fb=rows[1, 7], fs=rows[1, 9], shift=int(rows[1, 10]), hflip=True)
        assert (rows[0, 3:7] == R.OP_CONTRAST).any() and not (rows[1, 3:3 + int(rows[1, 2])] == R.OP_CONTRAST).any()
    return torch.from_numpy(rows)


def _index(index, dtype):
    if index is None:          # a non-zero-offset slice of a longer index tensor
        longer = torch.tensor([9, 9, 2, 0, 4, 9], dtype=dtype, device=DEV)
        idx = longer[2:5]
        assert idx.data_ptr() != longer.data_ptr()
        return idx
    return torch.tensor(index, dtype=dtype, device=DEV)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("kind", list(STORES))
def test_indexed_prep_equals_prep_of_the_gathered_store(kind, train):
    size = STORES[kind][1]
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    k = 0
    for name, index in INDEX_VARIANTS:
        for flags in FLAG_SETS:
            dtype = (torch.int32, torch.int64)[k % 2]          # (two flag sets per variant: every variant runs with both widths)
            frames, labels = _store(kind, wide_labels=bool((k // 2) % 2))
            k += 1
            idx = _index(index, dtype)
            B = int(idx.shape[0])
            rows = _rows(B, 30 + k) if train else None
            kw = dict(img_size=size, train=train, params=rows, no_ball=flags[0], no_robot=flags[1], no_goal=flags[2], no_line=flags[3])
            gi, gt = D.prepare_rgb_batch(frames, labels, index=idx, bad_index=bad, **kw)
            wi, wt = D.prepare_rgb_batch(frames[idx.long()].contiguous(), labels[idx.long()].contiguous(), **kw)
            assert tuple(gi.shape) == (B, 3) + size and tuple(gt.shape) == (B,) + size and gt.dtype == torch.int64
            assert _same(gi, wi) and torch.equal(gt, wt), (name, flags, dtype)
            if train:          # the same rows from the device, with and without the caller's word on the contrast
                gi2, gt2 = D.prepare_rgb_batch(frames, labels, index=idx, bad_index=bad, **dict(kw, params=rows.to(DEV)), contrast=True)
                assert _same(gi2, wi) and torch.equal(gt2, wt), (name, flags, dtype)
    gi, gt = D.prepare_rgb_batch(frames, None, img_size=size, train=False, index=idx, bad_index=bad)          # the patch chain: no labels
    assert gt is None and _same(gi, D.prepare_rgb_batch(frames[idx.long()].contiguous(), None, img_size=size, train=False)[0])
    assert int(bad.item()) == 0


@pytest.mark.parametrize("kind", list(STORES))
def test_no_contrast_hint_gives_the_same_bits(kind):
    """Rows that hold no contrast: the call that is told so (one launch) equals the call that runs the statistics launch."""
    size = STORES[kind][1]
    frames, labels = _store(kind, False)
    idx = torch.tensor([2, 0, 4, 4], device=DEV)
    rows = _rows(4, 91, contrast=False)
    assert not (rows[:, 3:7] == R.OP_CONTRAST).any() and bool((rows[:, 2] == 3).all())
    want = D.prepare_rgb_batch(frames[idx].contiguous(), labels[idx].contiguous(), img_size=size, params=rows)
    for hint in (False, True, None):
        got = D.prepare_rgb_batch(frames, labels, img_size=size, params=rows.to(DEV), index=idx, contrast=hint)
        assert _same(got[0], want[0]) and torch.equal(got[1], want[1]), hint


@pytest.mark.parametrize("kind", list(STORES))
def test_index_outside_the_store_is_zeros_and_counted(kind):
    src, size = STORES[kind]
    frames, labels = _store(kind, False)
    N = 5
    store = D.ResidentDataset.from_tensors(frames, labels, src)          # at its own size: a copy
    assert len(store) == N and torch.equal(store.frames, frames) and torch.equal(store.labels, labels)
    store.check()                                                       # nothing counted yet
    rows = _rows(4, 77)
    rows[2] = rows[0]                                                   # a refused row WITH a contrast: the statistics launch meets it too
    idx = torch.tensor([0, N, -1, 2], device=DEV)
    gi, gt = D.prepare_rgb_batch(store.frames, store.labels, img_size=size, params=rows, index=idx, bad_index=store.bad_index)
    wi, wt = D.prepare_rgb_batch(frames[[0, 2]].contiguous(), labels[[0, 2]].contiguous(), img_size=size, params=rows[[0, 3]].contiguous())
    assert not gi[1:3].any() and not gt[1:3].any()
    assert _same(gi[[0, 3]], wi) and torch.equal(gt[[0, 3]], wt)
    assert int(store.bad_index.item()) == 2
    with pytest.raises(IndexError, match="2 images"):
        store.check()
    store.check()                                                       # cleared by the check that raised


# ------------------------------------------------------------------------------------------ pairs
@functools.lru_cache(maxsize=None)
def _pair_store(H, W, wide_labels):
    frames, labels = R.synthetic_frames(6, H, W, 41)
    labels = labels.copy()
    labels[2, H // 2, W // 3] = 7                                       # outside [0, 5): no class channel
    return torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(torch.int32 if wide_labels else torch.uint8).to(DEV)


def _composition(frames, labels, pairs, train, rows):
    """Item 2 of the contract by the existing ops: labelprop_batch of prepare_rgb_batch of the gathered frames, every row repeated."""
    B = int(pairs.shape[0])
    H, W = int(frames.shape[1]), int(frames.shape[2])
    flat = pairs.reshape(-1).long()
    imgs, tgts = D.prepare_rgb_batch(frames[flat].contiguous(), labels[flat].contiguous(), img_size=(H, W), train=train,
                                     params=None if rows is None else rows.repeat_interleave(2, 0))
    return M.labelprop_batch(imgs.view(B, 2, 3, H, W), tgts.view(B, 2, H, W))


PAIR_SETS = [("consecutive, reversed, same", [[0, 1], [1, 2], [4, 3], [2, 2], [5, 0]]), ("B = 1", [[3, 2]])]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("H,W", [(16, 16), (37, 70)])
def test_lp_pairs_equal_the_composition(H, W, train):
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    k = 0
    for name, plist in PAIR_SETS:
        for wide in (False, True):
            frames, labels = _pair_store(H, W, wide)
            dtype = (torch.int32, torch.int64)[k % 2]
            k += 1
            pairs = torch.tensor(plist, dtype=dtype, device=DEV)
            B = len(plist)
            rows = _rows(B, 50 + k) if train else None
            gx, gt = D.prepare_lp_pairs(frames, labels, pairs, train=train, params=rows, bad_index=bad)
            wx, wt = _composition(frames, labels, pairs, train, rows)
            assert tuple(gx.shape) == (2 * B, 8, H, W) and gx.permute(0, 2, 3, 1).is_contiguous() and gt.dtype == torch.int64
            assert _same(gx.permute(0, 2, 3, 1), wx.permute(0, 2, 3, 1)) and torch.equal(gt, wt), (name, wide, dtype)
            seven = gt == 7
            if B > 1:          # frame 2 is in three samples: all five class channels of the OTHER sample of its pair are -1 there
                other = seven[[s ^ 1 for s in range(2 * B)]]
                assert int(seven.sum()) == 3 and bool((gx.permute(0, 2, 3, 1)[other][:, 3:] == -1).all())
            again = D.prepare_lp_pairs(frames, labels, pairs, train=train, params=rows, bad_index=bad)
            assert _same(again[0].permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1)) and torch.equal(again[1], gt)
            if train:          # device rows, with the caller's word
                dx, dt = D.prepare_lp_pairs(frames, labels, pairs, params=rows.to(DEV), bad_index=bad, contrast=True)
                assert _same(dx.permute(0, 2, 3, 1), wx.permute(0, 2, 3, 1)) and torch.equal(dt, wt)
    assert int(bad.item()) == 0


def test_lp_pairs_no_contrast_hint_and_bad_pair():
    H, W = 37, 70
    frames, labels = _pair_store(H, W, False)
    pairs = torch.tensor([[0, 1], [4, 2]], device=DEV)
    rows = _rows(2, 93, contrast=False)
    want = _composition(frames, labels, pairs, True, rows)
    for hint in (False, True, None):
        got = D.prepare_lp_pairs(frames, labels, pairs, params=rows.to(DEV), contrast=hint)
        assert _same(got[0].permute(0, 2, 3, 1), want[0].permute(0, 2, 3, 1)) and torch.equal(got[1], want[1]), hint
    # a pair with ONE index outside the store: zeros in both samples, counted once; the pairs next to it are untouched
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows = _rows(4, 94)
    rows[1] = rows[0]                                                   # the refused pairs hold a contrast
    rows[3] = rows[0]
    pairs = torch.tensor([[0, 1], [2, 6], [3, 4], [-1, 0]], device=DEV)
    gx, gt = D.prepare_lp_pairs(frames, labels, pairs, params=rows, bad_index=bad)
    wx, wt = _composition(frames, labels, pairs[[0, 2]], True, rows[[0, 2]].contiguous())
    gx = gx.permute(0, 2, 3, 1)
    assert not gx[2:4].any() and not gt[2:4].any() and not gx[6:8].any() and not gt[6:8].any()
    assert _same(gx[[0, 1, 4, 5]], wx.permute(0, 2, 3, 1)) and torch.equal(gt[[0, 1, 4, 5]], wt)
    assert int(bad.item()) == 2


# ------------------------------------------------------------------------------------------ against the NumPy restatement
def test_indexed_prep_against_the_restatement():
    src, size = STORES["staged"]
    frames, labels = R.synthetic_frames(5, src[0], src[1], 21)
    rows = _rows(4, 61)
    index = [4, 7, 0, 4]
    flags = (True, False, True, False)
    wi, wt, wbad = RG.prepare_rgb_indexed(frames, labels, index, size, train=True, params=rows.numpy(), flags=flags)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    gi, gt = D.prepare_rgb_batch(torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(DEV), img_size=size, params=rows,
                                 index=torch.tensor(index, device=DEV), bad_index=bad, no_ball=True, no_goal=True)
    assert np.array_equal(_bits(gi), wi.view(np.uint32)) and np.array_equal(gt.cpu().numpy(), wt) and int(bad.item()) == wbad == 1


def test_lp_pairs_against_the_restatement():
    H, W = 37, 70
    frames, labels = R.synthetic_frames(6, H, W, 41)
    labels[2, 5, 5] = 7
    rows = _rows(3, 62)
    pairs = [[2, 3], [5, 5], [1, 6]]
    wx, wt, wbad = RG.prepare_lp_pairs(frames, labels, pairs, train=True, params=rows.numpy())
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    gx, gt = D.prepare_lp_pairs(torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(DEV), torch.tensor(pairs, device=DEV), params=rows,
                                bad_index=bad)
    assert np.array_equal(_bits(gx.contiguous()), wx.view(np.uint32)) and np.array_equal(gt.cpu().numpy(), wt) and int(bad.item()) == wbad == 1


# ------------------------------------------------------------------------------------------ loaders
def test_rgb_epoch_batches_equal_prep_of_the_full_size_frames():
    src, size = STORES["staged"]
    frames, labels = R.synthetic_frames(9, src[0], src[1], 61)
    frames, labels = torch.from_numpy(frames), torch.from_numpy(labels)
    store = D.ResidentDataset.from_tensors(frames, labels, size, device=DEV, chunk=4)
    assert tuple(store.frames.shape) == (9,) + size + (3,) and store.labels.dtype == torch.uint8
    fd, ld = frames.to(DEV), labels.to(DEV)
    epochs = []
    for prefetch in (False, True):
        random.seed(5)
        np.random.seed(5)
        loader = D.RGBEpochLoader(store, 4, generator=torch.Generator().manual_seed(9), no_robot=True, prefetch=prefetch)
        assert len(loader) == 3
        got = []
        for _ in range(2):
            batches = list(loader)
            assert (loader._next is not None) == prefetch
            got.append((loader.last_index, loader.last_rows, batches))
        epochs.append(got)
    index, rows, batches = epochs[0][0]
    assert torch.equal(index, torch.randperm(9, generator=torch.Generator().manual_seed(9))) and tuple(rows.shape) == (9, 12)
    assert [int(b[0].shape[0]) for b in batches] == [4, 4, 1]
    for k, (a, b) in enumerate(loader.plan(index)):
        wi, wt = D.prepare_rgb_batch(fd[index[a:b]].contiguous(), ld[index[a:b]].contiguous(), img_size=size, params=rows[a:b].contiguous(),
                                     no_robot=True)
        assert _same(batches[k][0], wi) and torch.equal(batches[k][1], wt), k
    for e in range(2):          # prefetch draws the same epochs, only earlier
        (ia, ra, ba), (ib, rb, bb) = epochs[0][e], epochs[1][e]
        assert torch.equal(ia, ib) and torch.equal(ra, rb) and len(ba) == len(bb) == 3
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ba, bb))
    assert not torch.equal(epochs[0][0][0], epochs[0][1][0])
    # rows without a contrast: every slice is told so and takes one launch; validation: arange, no draws
    random.seed(6)
    np.random.seed(6)
    loader = D.RGBEpochLoader(store, 4, jitter=(0.5, 0.0, 0.4, 0.3), shuffle=False, drop_last=True)
    batches = list(loader)
    assert len(batches) == 2 and not (loader.last_rows[:, 3:7] == R.OP_CONTRAST).any()
    wi, wt = D.prepare_rgb_batch(fd[4:8].contiguous(), ld[4:8].contiguous(), img_size=size, params=loader.last_rows[4:8].contiguous())
    assert _same(batches[1][0], wi) and torch.equal(batches[1][1], wt)
    val = list(D.RGBEpochLoader(store, 4, train=False, shuffle=False))
    wi, wt = D.prepare_rgb_batch(fd[8:9].contiguous(), ld[8:9].contiguous(), img_size=size, train=False)
    assert len(val) == 3 and _same(val[2][0], wi) and torch.equal(val[2][1], wt)
    store.check()


def test_lp_epoch_batches_equal_lp_pairs_and_train_labelprop():
    H, W = 16, 16
    frames, labels = R.synthetic_frames(7, H, W, 71)
    store = D.ResidentDataset.from_tensors(torch.from_numpy(frames), torch.from_numpy(labels), (H, W), device=DEV)
    windows = torch.tensor([[0, 1], [1, 2], [3, 4], [4, 5], [5, 6]])          # two sequences of 3 and 4 frames
    random.seed(7)
    np.random.seed(7)
    loader = D.LPEpochLoader(store, windows, 2, generator=torch.Generator().manual_seed(3))
    assert len(loader) == 3
    batches = list(loader)
    pairs, rows = loader.last_index, loader.last_rows
    assert torch.equal(pairs, windows[torch.randperm(5, generator=torch.Generator().manual_seed(3))]) and tuple(rows.shape) == (5, 12)
    assert [int(b[0].shape[0]) for b in batches] == [4, 4, 2]
    for k, (a, b) in enumerate(loader.plan(torch.arange(5))):
        wx, wt = D.prepare_lp_pairs(store.frames, store.labels, pairs[a:b].to(DEV), params=rows[a:b].contiguous())
        assert _same(batches[k][0].permute(0, 2, 3, 1), wx.permute(0, 2, 3, 1)) and torch.equal(batches[k][1], wt), k
    store.check()
    torch.manual_seed(12345678)
    model = M.LabelProp(5, 32, 0).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    tr = Trainer(model, class_weights=(1, 6, 1, 3, 2), optimizer=SGD(model, lr=2e-1, momentum=0.5, weight_decay=1e-3))
    tr.step(*batches[0])
    assert np.isfinite(tr.pop_metrics()["loss"])
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


def test_rgb_epoch_batch_trains_pb_fcn():
    size = (40, 72)
    frames, labels = R.synthetic_frames(6, 160, 288, 55)
    store = D.ResidentDataset.from_tensors(torch.from_numpy(frames), torch.from_numpy(labels), size, device=DEV)
    random.seed(8)
    np.random.seed(8)
    x, t = next(iter(D.RGBEpochLoader(store, 3, generator=torch.Generator().manual_seed(11))))
    torch.manual_seed(12345678)
    model = M.PB_FCN(32, 5, 1, False, 0).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))
    tr.step(x, t)
    assert np.isfinite(tr.pop_metrics()["loss"])
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    store.check()
