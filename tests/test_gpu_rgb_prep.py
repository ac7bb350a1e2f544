"""GPU: the RGB batch preparation kernel (RCV_OP_RGB_PREP, ``prepare_rgb_batch``, csrc/rgb_prep.hip) against the NumPy restatement
(tests/rgb_prep_restatement.py) computed live and against the goldens (tests/golden/make_golden_rgb_prep.py, made with Pillow's own
calls).  Needs neither Pillow nor the reference.  The bar is one: every element of every output, images as float32 BITS and targets
as integers, equals the restatement's."""
import hashlib
import itertools
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import rgb_prep_restatement as R
import robocupvision_amd.model as M
from robocupvision_amd import data as D
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

with open(os.path.join(GOLDEN, "rgb_prep.json")) as _f:
    META = json.load(_f)
KATS = np.load(os.path.join(GOLDEN, "rgb_prep.npz"))
NO_FLAGS = (False, False, False, False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def _run(frames, labels, size, train=False, rows=None, flags=NO_FLAGS, lab_dtype=torch.int32, scale=None, device_rows=False):
    f = torch.from_numpy(frames).to(DEV)
    lab = None if labels is None else torch.from_numpy(labels).to(lab_dtype).to(DEV)
    params = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.float32))
    if device_rows:
        params = params.to(DEV)
    kw = dict(scale=scale) if scale is not None else dict(img_size=size)
    imgs, tgt = D.prepare_rgb_batch(f, lab, train=train, params=params, no_ball=flags[0], no_robot=flags[1], no_goal=flags[2],
                                    no_line=flags[3], **kw)
    torch.cuda.synchronize()
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (len(frames), 3) + tuple(size) and imgs.is_contiguous()
    if labels is None:
        assert tgt is None
        return imgs.cpu().numpy(), None
    assert tgt.dtype == torch.int64 and tuple(tgt.shape) == (len(frames),) + tuple(size) and tgt.is_contiguous()
    return imgs.cpu().numpy(), tgt.cpu().numpy()


def _check(got, frames, labels, size, train, rows, flags=NO_FLAGS):
    """Every element of the kernel's batch against the restatement, image by image."""
    imgs, tgt = got
    for b in range(len(frames)):
        wi, wl = R.prepare_image(frames[b], None if labels is None else labels[b], size, train, None if rows is None else rows[b], flags)
        assert np.array_equal(_bits(imgs[b]), _bits(wi)), ("image %d: %d elements differ" % (b, int((_bits(imgs[b]) != _bits(wi)).sum())))
        if labels is not None:
            assert np.array_equal(tgt[b], wl), "targets of image %d" % b


def _drawn(B, seed):
    random.seed(seed)
    np.random.seed(seed)
    return D.draw_color_jitter(B).numpy()


def _perm_rows(seed):
    rows = _drawn(24, seed)
    for b, perm in enumerate(itertools.permutations(range(4))):
        rows[b, 3:7] = perm
        rows[b, 0], rows[b, 1] = float(b & 1), float((b >> 1) & 1)
    return rows


@pytest.fixture(scope="module")
def colours():
    """The 2^20 colours 17 k mod 2^24 as one 1024 x 1024 frame."""
    k = (17 * np.arange(1 << 20, dtype=np.int64)) % (1 << 24)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8).reshape(1, 1024, 1024, 3)


@pytest.mark.parametrize("tag", sorted(META["configs"]))
def test_kernel_vs_goldens(tag):
    c = META["configs"][tag]
    B, size, flags = c["B"], tuple(c["size"]), R.FLAG_SETS[c["flags"]]
    frames, labels = R.synthetic_frames(B, c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"], cover_size=size)
    rows = KATS[tag + "/params"]
    ti, tt = _run(frames, labels, size, train=True, rows=rows, flags=flags)
    assert np.array_equal(tt, KATS[tag + "/train_labels"].astype(np.int64))
    assert np.array_equal(_bits(ti), _bits(KATS[tag + "/train_imgs"])) and _sha(ti, tt) == c["train_sha256"]
    for b in range(B):          # the golden's bytes after step 3 give these bits through step 4
        assert np.array_equal(_bits(ti[b]), _bits(R.to_yuv(KATS[tag + "/train_bytes"][b])))
    vi, vt = _run(frames, labels, size, train=False, flags=flags)
    assert np.array_equal(vt, KATS[tag + "/val_labels"].astype(np.int64)) and _sha(vi, vt) == c["val_sha256"]


def test_all_24_orders_with_both_flips_mixed():
    """B = 24, one image per permutation of the four operations, (33, 47) -> (16, 23) through ``scale=2``."""
    frames, labels = R.synthetic_frames(24, 33, 47, 31)
    rows = _perm_rows(32)
    assert R.scaled_size(33, 47, 2) == (16, 23) and {(r[0], r[1]) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    _check(_run(frames, labels, (16, 23), train=True, rows=rows, scale=2), frames, labels, (16, 23), True, rows)
    # rows that already lie on the device are taken as they are (the statistics launch always runs)
    _check(_run(frames, labels, (16, 23), train=True, rows=rows, scale=2, device_rows=True), frames, labels, (16, 23), True, rows)


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_multi_tile_ragged_with_contrast(where):
    """(97, 131) -> (40, 33): five tiles in y, ragged in x and y; the partial sums of L cross tiles.  B = 2."""
    frames, labels = R.synthetic_frames(2, 97, 131, 33, full_range_labels=True)
    rows = _drawn(2, 34)
    order = {"first": [1, 3, 0, 2], "last": [2, 0, 3, 1], "absent": [3, 2, 0, -1]}[where]
    for b in range(2):
        rows[b, 3:7] = order
        rows[b, 2] = 3 if where == "absent" else 4
        rows[b, 0], rows[b, 1] = float(b), float(1 - b)
    _check(_run(frames, labels, (40, 33), train=True, rows=rows, flags=R.FLAG_SETS[6]), frames, labels, (40, 33), True, rows, R.FLAG_SETS[6])


def test_wide_output_more_than_one_tile_in_x():
    """(41, 301) -> (19, 150): three tiles in x, the last one ragged, three in y."""
    frames, labels = R.synthetic_frames(1, 41, 301, 35)
    rows = _drawn(1, 36)
    rows[0, 0], rows[0, 1] = 1.0, 1.0
    _check(_run(frames, labels, (19, 150), train=True, rows=rows), frames, labels, (19, 150), True, rows)


@pytest.mark.parametrize("src,size", [((30, 96), (10, 32)), ((30, 97), (10, 32)), ((64, 80), (8, 10)), ((50, 70), (75, 100))])
def test_both_sides_of_the_staging_threshold(src, size):
    """The kernel stages its source rows in LDS from 9 taps per column (a shrink above 3): 96 -> 32 reads through the cache, 97 -> 32
    stages; a shrink of exactly 8 (17 taps, the most the tables allow) and an upscale."""
    assert (D.bilinear_table(src[1], size[1]).shape[1] - 2 >= 9) == (src[1] > 3 * size[1])
    frames, labels = R.synthetic_frames(2, src[0], src[1], 57, full_range_labels=True)
    rows = _drawn(2, 58)
    rows[0, 0], rows[1, 1] = 1.0, 1.0
    _check(_run(frames, labels, size, train=True, rows=rows, lab_dtype=torch.uint8), frames, labels, size, True, rows)


@pytest.mark.parametrize("src", [(45, 67), (1, 1)])
def test_identity_resize(src):
    B = 3
    frames, labels = R.synthetic_frames(B, src[0], src[1], 37, full_range_labels=True)
    rows = _drawn(B, 38)
    rows[:, 0], rows[:, 1] = [0, 1, 1], [1, 0, 1]
    _check(_run(frames, labels, src, train=True, rows=rows, scale=1, lab_dtype=torch.uint8), frames, labels, src, True, rows)
    _check(_run(frames, labels, src, train=False, scale=1), frames, labels, src, False, None)


def test_patches_without_labels():
    """The chain of classTrainer.py / objDetEval.py: 32 x 32 patches, B = 64, no label plane."""
    frames, _ = R.synthetic_frames(64, 32, 32, 39)
    rows = _drawn(64, 40)
    _check(_run(frames, None, (32, 32), train=True, rows=rows, scale=1), frames, None, (32, 32), True, rows)
    _check(_run(frames, None, (32, 32), train=False, scale=1), frames, None, (32, 32), False, None)
    small, _ = R.synthetic_frames(4, 64, 64, 41)          # ... and patches that are scaled
    _check(_run(small, None, (32, 32), train=True, rows=rows[:4], scale=2), small, None, (32, 32), True, rows[:4])


def test_full_size_frames_scaled_by_4():
    frames, labels = R.synthetic_frames(2, 480, 640, 42)
    rows = _drawn(2, 43)
    rows[0, 0], rows[0, 1], rows[1, 0], rows[1, 1] = 1, 0, 0, 1
    _check(_run(frames, labels, (120, 160), train=True, rows=rows, scale=4), frames, labels, (120, 160), True, rows)


def test_full_size_frames_no_scale():
    frames, labels = R.synthetic_frames(1, 480, 640, 44)
    rows = _drawn(1, 45)
    rows[0, 0], rows[0, 1] = 1, 1
    _check(_run(frames, labels, (480, 640), train=True, rows=rows, scale=1), frames, labels, (480, 640), True, rows)


def test_hue_alone_on_2_20_colours(colours):
    """A wrong rounding placement in either HSV direction hits about 0.2 % of colours: about 2 000 of these."""
    shifts = [0, 1, 128, 255]
    frames = np.repeat(colours, len(shifts), 0)
    rows = np.stack([R.make_row([3], shift=s) for s in shifts])
    imgs, _ = _run(frames, None, (1024, 1024), train=True, rows=rows, scale=1)
    for b, s in enumerate(shifts):
        want = R.to_yuv(R.hue(colours[0], s))
        assert np.array_equal(_bits(imgs[b]), _bits(want)), (s, int((_bits(imgs[b]) != _bits(want)).any(0).sum()))
    assert not np.array_equal(_bits(imgs[0]), _bits(R.to_yuv(colours[0])))          # the round trip of shift 0 is not the identity


@pytest.mark.parametrize("op", [R.OP_BRIGHTNESS, R.OP_CONTRAST, R.OP_SATURATION])
def test_blend_operations_alone_on_2_20_colours(colours, op):
    random.seed(50 + op)
    factors = [0.5, 1.0, 1.5, random.uniform(0.5, 1.5), random.uniform(0.5, 1.5)]
    frames = np.repeat(colours, len(factors), 0)
    rows = np.stack([R.make_row([op], **{("fb", "fc", "fs")[op]: f}) for f in factors])
    imgs, _ = _run(frames, None, (1024, 1024), train=True, rows=rows, scale=1)
    for b in range(len(factors)):
        want = R.to_yuv(R.color_ops(colours[0], rows[b]))
        assert np.array_equal(_bits(imgs[b]), _bits(want)), (factors[b], int((_bits(imgs[b]) != _bits(want)).any(0).sum()))


def test_uniform_image_contrast_mean_is_the_value():
    vals = [0, 1, 127, 200, 255]
    frames = np.stack([np.full((21, 70, 3), v, np.uint8) for v in vals])          # (21, 70) -> (10, 35) and the identity
    rows = np.stack([R.make_row([1, 0], fb=1.2, fc=0.3 + 0.2 * k) for k in range(len(vals))])
    for size in ((10, 35), (21, 70)):
        got = _run(frames, None, size, train=True, rows=rows)
        for b, v in enumerate(vals):
            assert R.contrast_mean(frames[b]) == v
            want = R.to_yuv(R.color_ops(np.full(size + (3,), v, np.uint8), rows[b]))
            assert np.array_equal(_bits(got[0][b]), _bits(want)), (size, v)
        _check(got, frames, None, size, True, rows)


@pytest.mark.parametrize("lab_dtype", [torch.uint8, torch.int32])
def test_all_mask_flag_sets_on_every_label_value(lab_dtype):
    frames, labels = R.synthetic_frames(2, 33, 47, 46, full_range_labels=True, cover_size=(16, 23))
    rows = _drawn(2, 47)
    for b in range(2):
        assert len(np.unique(R.resize_nearest(labels[b], (16, 23)))) == 256, "every label value 0..255 must reach the output"
    for flags in R.FLAG_SETS:
        _check(_run(frames, labels, (16, 23), train=True, rows=rows, flags=flags, lab_dtype=lab_dtype), frames, labels, (16, 23), True, rows,
               flags)


def test_unaligned_frame_buffer():
    """Frames that start 1 byte into an allocation and end at its last byte."""
    B, src, size = 2, (23, 69), (11, 17)
    frames, labels = R.synthetic_frames(B, src[0], src[1], 48)
    rows = _drawn(B, 49)
    buf = torch.zeros(1 + frames.size, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(frames).reshape(-1).to(DEV)
    f = buf[1:].view(B, src[0], src[1], 3)
    assert f.data_ptr() % 16 == 1 and f.is_contiguous()
    imgs, tgt = D.prepare_rgb_batch(f, torch.from_numpy(labels).to(DEV), params=torch.from_numpy(rows), img_size=size)
    _check((imgs.cpu().numpy(), tgt.cpu().numpy()), frames, labels, size, True, rows)


def test_validation_mode_is_training_mode_with_nothing_to_do():
    frames, labels = R.synthetic_frames(3, 61, 83, 51)
    rows = np.stack([R.make_row([]) for _ in range(3)])
    vi, vt = _run(frames, labels, (30, 41), train=False, scale=2)
    ti, tt = _run(frames, labels, (30, 41), train=True, rows=rows, scale=2)
    assert np.array_equal(_bits(vi), _bits(ti)) and np.array_equal(vt, tt)
    _check((vi, vt), frames, labels, (30, 41), False, None)


def test_deterministic_across_calls():
    frames, labels = R.synthetic_frames(4, 97, 131, 52)
    rows = _drawn(4, 53)
    a = _run(frames, labels, (40, 33), train=True, rows=rows)
    b = _run(frames, labels, (40, 33), train=True, rows=rows)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


def test_device_refusals():
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(2, 24, 32, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="params"):
        D.prepare_rgb_batch(f, lab, 2)
    with pytest.raises(ValueError, match="contiguous"):
        D.prepare_rgb_batch(f.transpose(1, 2), lab.transpose(1, 2), 2, train=False)
    with pytest.raises(Exception, match="shrinks an axis by more than 8"):
        D.prepare_rgb_batch(f, lab, 12, train=False)


def test_prepared_batch_trains_pb_fcn():
    """prepare_rgb_batch -> two SGD steps of PB_FCN (trainer.py) give the loss bits of the same tensors uploaded."""
    B, src, size = 3, (160, 288), (40, 72)
    frames, labels = R.synthetic_frames(B, src[0], src[1], 55)
    rows = _drawn(B, 56)
    wi, wt = R.prepare_batch(frames, labels, size, True, rows)
    losses = []
    for use_kernel in (True, False):
        torch.manual_seed(12345678)
        model = M.PB_FCN(32, 5, 1, False, 0).to(DEV)
        tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))
        if use_kernel:
            x, t = D.prepare_rgb_batch(torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(DEV), 4, params=torch.from_numpy(rows))
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(wi)) and np.array_equal(t.cpu().numpy(), wt)
        else:
            x, t = torch.from_numpy(wi).to(DEV), torch.from_numpy(wt).to(DEV)
        tr.step(x, t)
        tr.step(x, t)
        losses.append(tr.pop_metrics()["loss"])
    assert np.isfinite(losses[0]) and np.float64(losses[0]).tobytes() == np.float64(losses[1]).tobytes(), losses
