"""GPU: the batch preparation kernel (RCV_OP_BATCH_PREP, ``prepare_batch``) against the reference's goldens
(tests/golden/make_golden_batch_prep.py) and against the NumPy restatement (tests/batch_prep_restatement.py) computed live.  Needs
neither Pillow nor the reference.  Bars: targets exact; validation-mode images exact (bits); training mode Y exact, U / V within
2^-23 (|m0 U| + |m1 V|) of the products summed in float64 (one fused multiply-add over an fp32 product: each rounding is at most
2^-24 of a magnitude that |m0 U| + |m1 V| bounds).  Every element of every output is compared."""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import batch_prep_restatement as R
import robocupvision_amd.model as M
from robocupvision_amd import data as D
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

with open(os.path.join(GOLDEN, "batch_prep.json")) as _f:
    META = json.load(_f)
KATS = np.load(os.path.join(GOLDEN, "batch_prep.npz"))
NO_FLAGS = (False, False, False, False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def _run(frames, labels, size, finetune=False, train=False, rows=None, flags=NO_FLAGS, lab_dtype=torch.int32):
    f = torch.from_numpy(frames).to(DEV)
    lab = torch.from_numpy(labels).to(lab_dtype).to(DEV)
    imgs, tgt = D.prepare_batch(f, lab, size, finetune=finetune, train=train, params=None if rows is None else torch.from_numpy(rows),
                                no_ball=flags[0], no_robot=flags[1], no_goal=flags[2], no_line=flags[3])
    torch.cuda.synchronize()
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (len(frames), 3) + tuple(size) and imgs.is_contiguous()
    assert tgt.dtype == torch.int64 and tuple(tgt.shape) == (len(frames),) + tuple(size) and tgt.is_contiguous()
    return imgs.cpu().numpy(), tgt.cpu().numpy()


def _check_train(imgs, tgt, frames, labels, size, finetune, rows, flags):
    """The kernel's training-mode batch against the restatement, image by image, every element."""
    for b in range(len(frames)):
        want, lab, uv64 = R.prepare_image(frames[b], labels[b], size, finetune, True, rows[b], flags, exact_uv=True)
        assert np.array_equal(tgt[b], lab), "targets of image %d" % b
        assert np.array_equal(_bits(imgs[b, 0]), _bits(want[0])), "Y of image %d" % b
        if rows[b, 7] != 0:
            assert np.array_equal(_bits(imgs[b, 1:]), _bits(want[1:])), "U / V of image %d must be untouched" % b
            continue
        small = frames[b] if frames[b].shape[:2] == tuple(size) else R.resize_bilinear(frames[b], size)
        bound = 2.0 ** -23 * R.uv_bound(small, finetune, rows[b], rows[b, 0] != 0)
        err = np.abs(imgs[b, 1:].astype(np.float64) - uv64)
        assert bool((err <= bound).all()), ("U / V of image %d: worst error / bound" % b, float((err / np.maximum(bound, 1e-300)).max()))


def _rows(B, seed, uv_off=()):
    random.seed(seed)
    torch.manual_seed(seed)
    rows = D.draw_jitter(B).numpy()
    for b in range(B):
        rows[b, 0] = float((b + seed) % 2)          # both flip states in every batch of two or more
    for b in uv_off:
        rows[b, 7] = 1.0
    return rows


@pytest.mark.parametrize("tag", sorted(META["configs"]))
def test_kernel_vs_goldens(tag):
    c = META["configs"][tag]
    B, size, ft = c["B"], tuple(c["size"]), c["finetune"]
    frames, labels = R.synthetic_frames(B, c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"], cover_size=size)
    vi, vt = _run(frames, labels, size, finetune=ft, train=False)
    assert np.array_equal(vt, KATS[tag + "/val_labels"].astype(np.int64))
    assert np.array_equal(_bits(vi), _bits(KATS[tag + "/val_imgs"])) and _sha(vi, vt) == c["val_sha256"]
    rows = KATS[tag + "/params"]
    ti, tt = _run(frames, labels, size, finetune=ft, train=True, rows=rows)
    gi = KATS[tag + "/train_imgs"]
    assert np.array_equal(tt, KATS[tag + "/train_labels"].astype(np.int64))
    assert np.array_equal(_bits(ti[:, 0]), _bits(gi[:, 0]))
    _check_train(ti, tt, frames, labels, size, ft, rows, NO_FLAGS)


@pytest.mark.parametrize("tag", sorted(META["full"]))
def test_full_size_validation_sha(tag):
    c = META["full"][tag]
    frames, labels = R.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"])
    vi, vt = _run(frames, labels, tuple(c["size"]), train=False)
    assert _sha(vi, vt) == c["val_sha256"]


@pytest.mark.parametrize("tag", ["ident", "ragged"])
@pytest.mark.parametrize("lab_dtype", [torch.uint8, torch.int32])
def test_all_mask_flag_sets_on_every_label_value(tag, lab_dtype):
    c = META["configs"][tag]
    size = tuple(c["size"])
    frames, labels = R.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=True, cover_size=size)
    for b in range(c["B"]):
        assert len(np.unique(R.resize_nearest(labels[b], size))) == 256, "every label value 0..255 must reach the output"
    for k, flags in enumerate(R.FLAG_SETS):
        vi, vt = _run(frames, labels, size, train=False, flags=flags, lab_dtype=lab_dtype)
        assert np.array_equal(vt, KATS[tag + "/masked"][k].astype(np.int64)), flags
        assert np.array_equal(_bits(vi), _bits(KATS[tag + "/val_imgs"]))


# (B, (Hs, Ws), (H, W), finetune, label dtype): a row of Ws * 3 bytes that is no multiple of 16 (131, 70, 47, 301 pixels), an
# upscale, a shrink of exactly 8 and a fractional one, more than one tile in x (W > 64) and in y (H > 8) with ragged last tiles,
# B = 1 and B = 64, the no-resize path at a pixel count that is no multiple of its 2048-pixel blocks, and both sides of the row shrink
# from which the kernel stages its source rows in LDS (9 taps per column: a shrink above 3 -- 96 -> 32 reads through the cache, 97 -> 32
# stages; of the others 131 -> 33, 80 -> 10 and 640 -> 150 stage)
LIVE_CASES = [
    (2, (97, 131), (40, 33), False, torch.int32),
    (1, (50, 70), (75, 100), True, torch.uint8),
    (2, (33, 47), (32, 46), False, torch.uint8),
    (1, (41, 301), (19, 150), False, torch.int32),
    (2, (64, 80), (8, 10), True, torch.int32),
    (1, (480, 640), (100, 150), False, torch.uint8),
    (64, (20, 28), (10, 14), False, torch.int32),
    (3, (45, 67), (45, 67), False, torch.uint8),
    (1, (1, 1), (1, 1), False, torch.int32),
    (2, (30, 96), (10, 32), False, torch.int32),
    (2, (30, 97), (10, 32), False, torch.uint8),
]


@pytest.mark.parametrize("ci", range(len(LIVE_CASES)))
def test_kernel_vs_live_restatement(ci):
    B, src, size, ft, lab_dtype = LIVE_CASES[ci]
    frames, labels = R.synthetic_frames(B, src[0], src[1], 40 + ci, full_range_labels=True)
    flags = R.FLAG_SETS[(3 * ci + 5) % 16]
    wi, wt = R.prepare_batch(frames, labels, size, finetune=ft, train=False, flags=flags)
    vi, vt = _run(frames, labels, size, finetune=ft, train=False, flags=flags, lab_dtype=lab_dtype)
    assert np.array_equal(vt, wt) and np.array_equal(_bits(vi), _bits(wi))
    rows = _rows(B, 70 + ci, uv_off=(0,) if B > 1 else ())
    ti, tt = _run(frames, labels, size, finetune=ft, train=True, rows=rows, flags=flags, lab_dtype=lab_dtype)
    _check_train(ti, tt, frames, labels, size, ft, rows, flags)


def test_unaligned_frame_buffer():
    """Frames that start 1 byte into an allocation and end at its last byte: the 16-byte loads of the staging may not reach outside."""
    B, src, size = 2, (23, 69), (11, 17)          # (a shrink of 4.06: the staged path)
    frames, labels = R.synthetic_frames(B, src[0], src[1], 91)
    wi, wt = R.prepare_batch(frames, labels, size, train=False)
    buf = torch.zeros(1 + frames.size, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(frames).reshape(-1).to(DEV)
    f = buf[1:].view(B, src[0], src[1], 3)
    assert f.data_ptr() % 16 == 1 and f.is_contiguous()
    imgs, tgt = D.prepare_batch(f, torch.from_numpy(labels).to(DEV), size, train=False)
    assert np.array_equal(tgt.cpu().numpy(), wt) and np.array_equal(_bits(imgs.cpu().numpy()), _bits(wi))


def test_device_refusals():
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(2, 24, 32, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="params"):
        D.prepare_batch(f, lab, (12, 16))                                  # train=True without the rows
    with pytest.raises(ValueError, match="contiguous"):
        D.prepare_batch(f.transpose(1, 2), lab.transpose(1, 2), (12, 16), train=False)
    with pytest.raises(Exception, match="shrinks an axis by more than 8"):
        D.prepare_batch(f, lab, (2, 16), train=False)


def test_prepared_batch_trains_robo_unet():
    """prepare_batch -> Trainer.step gives the loss bits of the same tensors uploaded: the outputs are what the step takes."""
    B, src, size = 3, (96, 128), (24, 32)
    frames, labels = R.synthetic_frames(B, src[0], src[1], 55)
    rows = _rows(B, 56, uv_off=(0, 1, 2))          # (U / V left alone: the restatement's batch is then bit-identical to the kernel's)
    wi = np.stack([R.prepare_image(frames[b], labels[b], size, False, True, rows[b])[0] for b in range(B)])
    wt = np.stack([R.prepare_image(frames[b], labels[b], size, False, True, rows[b])[1] for b in range(B)])
    losses = []
    for use_kernel in (True, False):
        torch.manual_seed(12345678)
        model = M.ROBO_UNet().to(DEV)
        tr = Trainer(model)
        if use_kernel:
            x, t = D.prepare_batch(torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(DEV), size, params=torch.from_numpy(rows))
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(wi)) and np.array_equal(t.cpu().numpy(), wt)
        else:
            x, t = torch.from_numpy(wi).to(DEV), torch.from_numpy(wt).to(DEV)
        tr.step(x, t)
        tr.step(x, t)
        losses.append(tr.pop_metrics()["loss"])
    assert np.isfinite(losses[0]) and np.float64(losses[0]).tobytes() == np.float64(losses[1]).tobytes(), losses
