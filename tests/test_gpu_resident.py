"""GPU: the device-resident dataset -- ``resize_u8`` (RCV_OP_RESIZE_U8) against live Pillow, every byte; ``prepare_batch(index=)``
(RCV_OP_BATCH_PREP_IDX) against ``prepare_batch`` of the gathered store, ``torch.equal`` on images and targets (the same arithmetic in
the same order, U / V included); the defined result of an index outside the store; ``ResidentDataset`` + ``EpochLoader`` against
``prepare_batch`` of the FULL-SIZE frames, bit for bit; and an ``EpochLoader`` batch through ``Trainer.step``.  The shapes cross the
kernel's 8-row x 64-column tile in both directions on both sides of the tap count from which it stages its source rows in LDS
(tests/resident_restatement.py SHAPES).  Every bar is equality: nothing here has a tolerance."""
import functools
import random

import numpy as np
import pytest
import torch
from PIL import Image

import batch_prep_restatement as R
import resident_restatement as RR
import robocupvision_amd.model as M
from robocupvision_amd import data as D
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAG_SETS = [(False, False, False, False), (True, False, True, False)]          # (no_ball, no_robot, no_goal, no_line)


@functools.lru_cache(maxsize=None)
def _pillow_case(src, size):
    """Three frames with labels that hold every value 0..255 (where the output has room), and Pillow's resize of them; made once."""
    frames, labels = R.synthetic_frames(3, src[0], src[1], 11, full_range_labels=True, cover_size=size)
    want = np.stack([np.asarray(Image.fromarray(f).resize((size[1], size[0]), Image.BILINEAR)) for f in frames])
    want_l = np.stack([np.asarray(Image.fromarray(p.astype(np.uint8)).convert("I").resize((size[1], size[0]), Image.NEAREST)) for p in labels])
    assert all(len(np.unique(p)) == min(256, size[0] * size[1]) for p in want_l)
    for a in (frames, labels, want, want_l):
        a.setflags(write=False)
    return frames, labels, want, want_l


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,size", RR.SHAPES)
def test_resize_u8_vs_live_pillow(src, size, B):
    frames, labels, want, want_l = _pillow_case(src, size)
    f = torch.from_numpy(frames[:B].copy()).to(DEV)
    for lab_in in (torch.uint8, torch.int32):
        lab = torch.from_numpy(labels[:B].copy()).to(lab_in).to(DEV)
        for lab_out in (torch.uint8, torch.int32):
            out, out_l = D.resize_u8(f, lab, size, label_dtype=lab_out)
            assert out.dtype == torch.uint8 and tuple(out.shape) == (B,) + size + (3,) and out.is_contiguous()
            assert out_l.dtype == lab_out and tuple(out_l.shape) == (B,) + size and out_l.is_contiguous()
            assert int((out.cpu().numpy() != want[:B]).sum()) == 0, (lab_in, lab_out)
            assert int((out_l.cpu().numpy().astype(np.int64) != want_l[:B]).sum()) == 0, (lab_in, lab_out)
    out, none = D.resize_u8(f, None, size)
    assert none is None and int((out.cpu().numpy() != want[:B]).sum()) == 0


def test_resize_u8_unaligned_frame_buffer():
    """Rows of 111 bytes in a buffer that starts 1 byte into an allocation and ends at its last byte (the staged path: 9 taps)."""
    src, size = RR.SHAPES[2]
    frames, labels, want, want_l = _pillow_case(src, size)
    buf = torch.zeros(1 + frames.size, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(frames.copy()).reshape(-1).to(DEV)
    f = buf[1:].view(3, src[0], src[1], 3)
    assert f.data_ptr() % 16 == 1 and f.is_contiguous()
    out, out_l = D.resize_u8(f, torch.from_numpy(labels.copy()).to(DEV), size)
    assert int((out.cpu().numpy() != want).sum()) == 0 and int((out_l.cpu().numpy() != want_l).sum()) == 0


@functools.lru_cache(maxsize=None)
def _store(resizing):
    """N = 5 images on the device: 44 x 280 (-> 11 x 70, int32 labels) or 11 x 70 already (no resize, uint8 labels)."""
    src = RR.SHAPES[0][0] if resizing else RR.SHAPES[3][0]
    frames, labels = R.synthetic_frames(5, src[0], src[1], 21)
    return torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(torch.int32 if resizing else torch.uint8).to(DEV)


def _rows(B, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    rows = D.draw_jitter_rows(B)
    rows[:, 0] = torch.arange(B) % 2          # both flip states in every batch of two or more
    return rows


INDEX_VARIANTS = [("reversed", [4, 3, 2, 1, 0]), ("repeats", [1, 1, 4, 1]), ("B > N", [0, 4, 2, 2, 3, 1, 0, 4, 4]), ("B = 1", [3])]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("resizing", [True, False])
def test_indexed_prep_equals_prep_of_the_gathered_store(resizing, train):
    frames, labels = _store(resizing)
    size = (11, 70)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    k = 0
    for name, index in INDEX_VARIANTS + [("slice", None)]:
        for flags in FLAG_SETS:
            dtype = (torch.int32, torch.int64)[k % 2]          # (two flag sets per variant: every variant runs with both widths)
            k += 1
            if index is None:          # a non-zero-offset slice of a longer index tensor
                longer = torch.tensor([9, 9, 2, 0, 4, 9], dtype=dtype, device=DEV)
                idx = longer[2:5]
                assert idx.data_ptr() != longer.data_ptr()
            else:
                idx = torch.tensor(index, dtype=dtype, device=DEV)
            B = int(idx.shape[0])
            rows = _rows(B, 30 + k) if train else None
            kw = dict(train=train, params=rows, no_ball=flags[0], no_robot=flags[1], no_goal=flags[2], no_line=flags[3])
            gi, gt = D.prepare_batch(frames, labels, size, index=idx, bad_index=bad, **kw)
            wi, wt = D.prepare_batch(frames[idx.long()].contiguous(), labels[idx.long()].contiguous(), size, **kw)
            assert tuple(gi.shape) == (B, 3) + size and tuple(gt.shape) == (B,) + size and gt.dtype == torch.int64
            assert torch.equal(gi, wi) and torch.equal(gt, wt), (name, flags, dtype)
            assert np.array_equal(gi.cpu().numpy().view(np.uint32), wi.cpu().numpy().view(np.uint32)), (name, flags, dtype)
    assert int(bad.item()) == 0


def test_index_outside_the_store_is_zeros_and_counted():
    frames, labels = _store(False)
    size, N = (11, 70), 5
    store = D.ResidentDataset.from_tensors(frames, labels, size)
    assert len(store) == N and torch.equal(store.frames, frames) and torch.equal(store.labels, labels)
    store.check()                                                       # nothing counted yet
    rows = _rows(4, 77)
    gi, gt = D.prepare_batch(store.frames, store.labels, size, params=rows, index=torch.tensor([0, N, -1, 2], device=DEV), bad_index=store.bad_index)
    wi, wt = D.prepare_batch(frames[[0, 2]].contiguous(), labels[[0, 2]].contiguous(), size, params=rows[[0, 3]].contiguous())
    assert not gi[1:3].any() and not gt[1:3].any()
    assert torch.equal(gi[[0, 3]], wi) and torch.equal(gt[[0, 3]], wt)
    assert int(store.bad_index.item()) == 2
    with pytest.raises(IndexError, match="2 images"):
        store.check()
    store.check()                                                       # cleared by the check that raised


def _full_size(n, src, seed):
    frames, labels = R.synthetic_frames(n, src[0], src[1], seed)
    return torch.from_numpy(frames), torch.from_numpy(labels)


def test_epoch_batches_equal_prep_of_the_full_size_frames():
    size = (24, 32)
    frames, labels = _full_size(10, (48, 64), 61)
    store = D.ResidentDataset.from_tensors(frames, labels, size, device=DEV, chunk=4)
    assert tuple(store.frames.shape) == (10, 24, 32, 3) and store.labels.dtype == torch.uint8 and store.frames.device.type == "cuda"
    random.seed(5)
    torch.manual_seed(5)
    loader = D.EpochLoader(store, 4, train=True, generator=torch.Generator().manual_seed(9), no_robot=True)
    assert len(loader) == 3
    batches = list(loader)
    index, rows = loader.last_index, loader.last_rows
    assert sorted(index.tolist()) == list(range(10)) and index.tolist() != list(range(10)) and tuple(rows.shape) == (10, 8)
    assert torch.equal(index, torch.randperm(10, generator=torch.Generator().manual_seed(9)))
    assert [int(b[0].shape[0]) for b in batches] == [4, 4, 2]
    fd, ld = frames.to(DEV), labels.to(DEV)
    for k, (a, b) in enumerate(loader.plan(index)):
        wi, wt = D.prepare_batch(fd[index[a:b]].contiguous(), ld[index[a:b]].contiguous(), size, params=rows[a:b].contiguous(), no_robot=True)
        assert torch.equal(batches[k][0], wi) and torch.equal(batches[k][1], wt), k
    store.check()
    # validation order: arange, no draws
    val = list(D.EpochLoader(store, 4, train=False, shuffle=False, drop_last=True))
    assert len(val) == 2
    wi, wt = D.prepare_batch(fd[4:8].contiguous(), ld[4:8].contiguous(), size, train=False)
    assert torch.equal(val[1][0], wi) and torch.equal(val[1][1], wt)


def test_prefetch_draws_the_same_epochs_earlier():
    size = (24, 32)
    frames, labels = _full_size(10, (48, 64), 61)
    store = D.ResidentDataset.from_tensors(frames, labels, size, device=DEV)
    epochs = []
    for prefetch in (False, True):
        random.seed(15)
        torch.manual_seed(15)
        loader = D.EpochLoader(store, 4, train=True, generator=torch.Generator().manual_seed(16), prefetch=prefetch)
        got = []
        for _ in range(2):
            batches = list(loader)
            assert (loader._next is not None) == prefetch
            got.append((loader.last_index, loader.last_rows, batches))
        epochs.append(got)
    for e in range(2):
        (ia, ra, ba), (ib, rb, bb) = epochs[0][e], epochs[1][e]
        assert torch.equal(ia, ib) and torch.equal(ra, rb) and len(ba) == len(bb) == 3
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ba, bb))
    assert not torch.equal(epochs[0][0][0], epochs[0][1][0])          # the two epochs differ: the comparison above is not vacuous
    store.check()


def test_store_of_two_source_sizes_equals_stores_built_separately():
    size = (24, 32)
    fa, la = _full_size(5, (48, 64), 62)
    fb, lb = _full_size(5, (96, 128), 63)
    lb = lb.clone()
    lb[4, 2, 2] = 300                                                   # a value past uint8 under the output's corner (NEAREST reads row / column 2): int32 labels
    items = [(fa[i].numpy(), la[i].numpy()) for i in range(5)] + [(fb[i].numpy(), lb[i].numpy()) for i in range(5)]
    mixed = D.ResidentDataset(items, size, device=DEV, chunk=4)
    sa = D.ResidentDataset.from_tensors(fa, la, size, device=DEV)
    sb = D.ResidentDataset.from_tensors(fb, lb, size, device=DEV)
    assert sa.labels.dtype == torch.uint8 and sb.labels.dtype == torch.int32 and mixed.labels.dtype == torch.int32
    assert torch.equal(mixed.frames, torch.cat([sa.frames, sb.frames])) and torch.equal(mixed.labels, torch.cat([sa.labels.int(), sb.labels]))
    assert int(mixed.labels[9, 0, 0]) == 300
    random.seed(6)
    torch.manual_seed(6)
    loader = D.EpochLoader(mixed, 4, train=True, generator=torch.Generator().manual_seed(10))
    batches = list(loader)
    index, rows = loader.last_index, loader.last_rows
    for k, (a, b) in enumerate(loader.plan(index)):
        imgs, tgt = [], []
        for j in range(a, b):          # image by image from the store of its own source size
            s, i = (sa, int(index[j])) if index[j] < 5 else (sb, int(index[j]) - 5)
            x, t = D.prepare_batch(s.frames[i:i + 1], s.labels[i:i + 1], size, params=rows[j:j + 1].contiguous())
            imgs.append(x)
            tgt.append(t)
        assert torch.equal(batches[k][0], torch.cat(imgs)) and torch.equal(batches[k][1], torch.cat(tgt)), k
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.ResidentDataset.from_tensors(fa, la, (48, 32), device=DEV)     # exactly one axis kept


def test_epoch_loader_batch_trains_robo_unet():
    """EpochLoader -> Trainer.step gives the loss bits of the same tensors made by prepare_batch from the full-size frames."""
    size = (24, 32)
    frames, labels = _full_size(6, (96, 128), 55)
    store = D.ResidentDataset.from_tensors(frames, labels, size, device=DEV)
    losses = []
    for resident in (True, False):
        random.seed(8)
        torch.manual_seed(8)
        loader = D.EpochLoader(store, 3, train=True, generator=torch.Generator().manual_seed(11))
        x, t = next(iter(loader))
        if not resident:
            idx = loader.last_index[:3]
            x, t = D.prepare_batch(frames[idx].to(DEV), labels[idx].to(DEV), size, params=loader.last_rows[:3].contiguous())
        torch.manual_seed(12345678)
        tr = Trainer(M.ROBO_UNet().to(DEV))
        tr.step(x, t)
        tr.step(x, t)
        losses.append(tr.pop_metrics()["loss"])
    assert np.isfinite(losses[0]) and np.float64(losses[0]).tobytes() == np.float64(losses[1]).tobytes(), losses
