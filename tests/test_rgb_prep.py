"""CPU: the RGB batch preparation (RCV_OP_RGB_PREP, ``prepare_rgb_batch``) -- the NumPy restatement
(tests/rgb_prep_restatement.py) against live Pillow piece by piece (exhaustively where the domain allows) and as a whole chain for all
24 orders of the four operations, against the goldens (tests/golden/make_golden_rgb_prep.py), ``draw_color_jitter``, the plan-time
refusals on the planner handle, the Python-level refusals and the ``SSDataSet`` listing."""
import hashlib
import itertools
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageStat

from conftest import GOLDEN
import batch_prep_restatement as BR
import rgb_prep_restatement as R
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D

with open(os.path.join(GOLDEN, "rgb_prep.json")) as _f:
    META = json.load(_f)
KATS = np.load(os.path.join(GOLDEN, "rgb_prep.npz"))
FACTORS = sorted(set([0.0, 0.5, 1.0, 1.5] + [float(np.float32(v)) for v in np.linspace(0.0, 1.5, 43)] + [0.123456, 1.3333, 0.6789]))


def _sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def all_colours():
    k = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def _ragged(seed, H=37, W=53):
    frames, _ = R.synthetic_frames(1, H, W, seed)
    return frames[0]


def test_blend_equals_pillow_on_all_byte_pairs():
    assert len(FACTORS) >= 40 and {0.0, 0.5, 1.0, 1.5} <= set(FACTORS)
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for f in FACTORS:
        want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(x), f))
        assert int((want != R.blend(d, x, f)).sum()) == 0, f


def test_luma_and_hsv_equal_pillow_on_all_colours(all_colours):
    im = Image.fromarray(all_colours)
    assert int((np.asarray(im.convert("L")) != R.luma(all_colours)).sum()) == 0
    assert int((np.asarray(im.convert("HSV")) != R.rgb_to_hsv(all_colours)).sum()) == 0
    back = np.asarray(Image.fromarray(all_colours, "HSV").convert("RGB"))
    assert int((back != R.hsv_to_rgb(all_colours)).sum()) == 0


def test_hue_round_trip_is_lossy_and_still_applied():
    k = (17 * np.arange(1 << 16, dtype=np.int64)) % (1 << 24)
    rgb = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8).reshape(256, 256, 3)
    back = R.hue(rgb, 0)
    same = float((back == rgb).all(-1).mean())
    assert 0.05 < same < 0.5          # most colours do not come back: a shift of 0 may not be skipped
    assert np.array_equal(back, np.asarray(Image.fromarray(rgb).convert("HSV").convert("RGB")))


@pytest.mark.parametrize("seed", [1, 2])
def test_enhance_operations_and_hue_on_ragged_images(seed):
    rgb = _ragged(seed)
    im = Image.fromarray(rgb)
    assert R.contrast_mean(rgb) == int(ImageStat.Stat(im.convert("L")).mean[0] + 0.5)
    for f in (0.0, 0.5, 0.73, 1.0, 1.27, 1.5):
        assert np.array_equal(R.brightness(rgb, f), np.asarray(ImageEnhance.Brightness(im).enhance(f))), f
        assert np.array_equal(R.contrast(rgb, f), np.asarray(ImageEnhance.Contrast(im).enhance(f))), f
        assert np.array_equal(R.saturation(rgb, f), np.asarray(ImageEnhance.Color(im).enhance(f))), f
    for shift in (0, 1, 77, 128, 255):
        assert np.array_equal(R.hue(rgb, shift), R.pillow_color_ops(rgb, R.make_row([3], shift=shift))), shift


def test_uniform_image_contrast_mean_is_the_value():
    for v in (0, 1, 127, 254, 255):
        assert R.contrast_mean(np.full((5, 7, 3), v, np.uint8)) == v


def test_whole_chain_all_24_orders_against_pillow_calls():
    frames, labels = R.synthetic_frames(24, 33, 47, 5)
    for b, perm in enumerate(itertools.permutations(range(4))):
        row = R.make_row(list(perm), fb=0.6 + 0.03 * b, fc=1.45 - 0.03 * b, fs=0.62 + 0.033 * b, shift=(37 * b + 3) & 255, hflip=b & 1, vflip=b & 2)
        gi, gl, gb = R.prepare_image(frames[b], labels[b], (16, 23), True, row, pillow=True, bytes_out=True)
        wi, wl, wb = R.prepare_image(frames[b], labels[b], (16, 23), True, row, bytes_out=True)
        assert np.array_equal(gb, wb), perm                                  # bytes after step 3
        assert np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gl, wl)      # float32 bits after step 4 (the float64 matrix restated)
        small = np.asarray(Image.fromarray(frames[b]).resize((23, 16), Image.BILINEAR))
        if b & 1:
            small = small[:, ::-1]
        if b & 2:
            small = small[::-1]
        assert np.array_equal(R.pillow_color_ops(np.ascontiguousarray(small), row), wb)      # ... and the resize is Pillow's too


@pytest.mark.parametrize("tag", sorted(META["configs"]))
def test_restatement_equals_goldens(tag):
    c = META["configs"][tag]
    size, flags = tuple(c["size"]), R.FLAG_SETS[c["flags"]]
    frames, labels = R.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"], cover_size=size)
    rows = KATS[tag + "/params"]
    for b in range(c["B"]):
        wi, wl, wb = R.prepare_image(frames[b], labels[b], size, True, rows[b], flags, bytes_out=True)
        assert np.array_equal(wb, KATS[tag + "/train_bytes"][b])
        assert np.array_equal(_bits(wi), _bits(KATS[tag + "/train_imgs"][b])) and np.array_equal(wl, KATS[tag + "/train_labels"][b].astype(np.int64))
    ti, tt = R.prepare_batch(frames, labels, size, True, rows, flags)
    vi, vt = R.prepare_batch(frames, labels, size, False, None, flags)
    assert _sha(ti, tt) == c["train_sha256"] and _sha(vi, vt) == c["val_sha256"]
    assert np.array_equal(vt, KATS[tag + "/val_labels"].astype(np.int64))


def test_yuv_definition_and_the_other_byte_to_float_form():
    # the definition on a few colours by hand: float64, products summed left to right, one rounding
    for rgb in ((0, 0, 0), (255, 255, 255), (12, 200, 77), (255, 0, 1)):
        c = [v / 255.0 for v in rgb]
        want = []
        for k in range(3):
            v = c[0] * float(R.YUV[k, 0]) + c[1] * float(R.YUV[k, 1])
            v = v + c[2] * float(R.YUV[k, 2])
            want.append(np.float32((v - 0.5) / 0.5 if k == 0 else v / 0.5))
        got = R.to_yuv(np.array([rgb], np.uint8))[:, 0]
        assert np.array_equal(_bits(got), _bits(np.array(want, np.float32)))
    # how many float32 outputs the other form, byte * (1 / 255.0), would change over all 2^24 colours (DESIGN 4.10 quotes the count)
    total = colours = 0
    k = np.arange(1 << 16, dtype=np.uint32)
    for hi in range(256):
        rgb = np.stack([np.full_like(k, hi), (k >> 8) & 255, k & 255], -1).astype(np.uint8)
        d = _bits(R.to_yuv(rgb)) != _bits(R.to_yuv(rgb, reciprocal=True))
        total += int(d.sum())
        colours += int(d.any(0).sum())
    print("byte * (1 / 255.0) changes %d of %d float32 outputs, in %d colours" % (total, 3 << 24, colours))
    assert {"outputs_that_differ": total, "colours_that_differ": colours} == META["reciprocal_form"]
    assert 0 < total < 1000          # the two forms are not the same function, and differ rarely


def _draw(seed, B, **kw):
    random.seed(seed)
    np.random.seed(seed)
    return D.draw_color_jitter(B, **kw)


def test_draw_color_jitter():
    a, b = _draw(7, 16), _draw(7, 16)
    assert a.dtype == torch.float32 and tuple(a.shape) == (16, 12) and a.device.type == "cpu" and torch.equal(a, b)
    assert not torch.equal(a, _draw(8, 16))
    for row in a.numpy():
        assert row[0] in (0, 1) and row[1] in (0, 1) and row[2] == 4 and sorted(row[3:7]) == [0, 1, 2, 3] and row[11] == 0
        assert 0.5 <= row[7] <= 1.5 and 0.5 <= row[8] <= 1.5 and np.float32(0.6) <= row[9] <= np.float32(1.4)
        assert row[10] == int(row[10]) and (0 <= row[10] <= 76 or 179 <= row[10] <= 255)          # int(h * 255) & 255, |h| <= 0.3
    # the goldens' rows are these draws
    for tag, c in META["configs"].items():
        if tag != "perm24":
            assert np.array_equal(_bits(_draw(c["draw_seed"], c["B"]).numpy()), _bits(KATS[tag + "/params"]))
    # both flip draws are the first two draws after the re-seed: the label's transforms, re-seeded alike, see the same two
    np.random.seed(7)
    for i in range(16):
        random.seed(np.random.randint(2147483647))
        assert (random.random() < 0.5, random.random() < 0.5) == (bool(a[i, 0]), bool(a[i, 1]))
        random.uniform(0, 1), random.uniform(0, 1), random.uniform(0, 1), random.uniform(0, 1), random.shuffle([0, 1, 2, 3])
    # hue = 0 shortens the list and leaves the earlier draws where they were
    nh = _draw(7, 16, hue=0)
    assert torch.equal(nh[:, :2], a[:, :2]) and torch.equal(nh[:, 7:10], a[:, 7:10]) and bool((nh[:, 2] == 3).all())
    assert bool((nh[:, 6] == -1).all()) and bool((nh[:, 10] == 0).all())
    for row in nh.numpy():
        assert sorted(row[3:6]) == [0, 1, 2]
    # no vertical flip: one draw fewer, none drawn for it
    nv = _draw(7, 16, vflip=False)
    assert bool((nv[:, 1] == 0).all()) and torch.equal(nv[:, 0], a[:, 0])
    # without the re-seed the rows follow the random module's own state
    random.seed(3)
    r1 = D.draw_color_jitter(4, reseed=False)
    random.seed(3)
    assert torch.equal(r1, D.draw_color_jitter(4, reseed=False))
    # validation strengths: nothing to do
    z = _draw(7, 2, brightness=0, contrast=0, saturation=0, hue=0)
    assert bool((z[:, 2] == 0).all()) and bool((z[:, 3:7] == -1).all()) and bool((z[:, 7:10] == 1).all())


@pytest.mark.parametrize("src,size", [((480, 640), (120, 160)), ((33, 47), (16, 23)), ((97, 131), (40, 33)), ((32, 32), (32, 32))])
def test_library_tables_equal_restatement(src, size):
    assert R.scaled_size(480, 640, 4) == (120, 160) and R.scaled_size(33, 47, 2) == (16, 23) and R.scaled_size(45, 67, 1) == (45, 67)
    for n_in, n_out in ((src[1], size[1]), (src[0], size[0])):
        tab = D.bilinear_table(n_in, n_out)
        if n_in != n_out:
            first, count, coef = BR.bilinear_coeffs(n_in, n_out)
            assert np.array_equal(tab[:, 0], first) and np.array_equal(tab[:, 1], count) and np.array_equal(tab[:, 2:], coef)
        assert np.array_equal(D.nearest_table(n_in, n_out), BR.nearest_index(n_in, n_out))


def _taps(n_in, n_out):
    return D.bilinear_table(n_in, n_out).shape[1] - 2


def _rec(B=32, Hs=480, Ws=640, H=120, W=160, lab=4, train=1, mask=0, stats=1, tables=True, kx=None, ky=None):
    t = 64 if tables else 0          # (a planner handle never reads through a pointer)
    return L.make_op(L.OP_RGB_PREP, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, inmode2=lab, aux0=train, aux1=mask, count=stats, p_x1=t, p_x2=t,
                     p_x3=t if lab else 0, p_x4=t if lab else 0)


@pytest.mark.parametrize("B,Hs,Ws,H,W,groups", [(32, 480, 640, 120, 160, 45), (8, 480, 640, 480, 640, 150), (64, 32, 32, 32, 32, 1),
                                               (2, 97, 131, 40, 33, 5)])
def test_plan_on_the_planner_handle(B, Hs, Ws, H, W, groups):
    h = L.planner_handle(256)
    for lab in (0, 1, 4):
        for train, stats in ((0, 0), (0, 1), (1, 0), (1, 1)):
            op = L.OpList([_rec(B=B, Hs=Hs, Ws=Ws, H=H, W=W, lab=lab, train=train, stats=stats, mask=5)])
            # one uint32 partial sum per workgroup of the statistics launch, which only training mode with a contrast runs
            assert L.op_workspace(h, op.arr[0]) == (4 * B * groups if train and stats else 0)
            assert op.labels(h) == ["rgb_prep"]
    with pytest.raises(L.RcvError, match="planning-only handle"):
        L.OpList([_rec(B=B, Hs=Hs, Ws=Ws, H=H, W=W)]).run(h, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), "every size must be >= 1"), (dict(H=0, ky=3), "every size must be >= 1"), (dict(W=0, kx=3), "every size must be >= 1"),
    (dict(Hs=0, ky=3), "every size must be >= 1"), (dict(Ws=0, kx=3), "every size must be >= 1"),
    (dict(H=59, ky=19), "shrinks an axis by more than 8"), (dict(W=79, kx=19), "shrinks an axis by more than 8"),
    (dict(lab=8), "label element size 8 unsupported"), (dict(lab=2), "label element size 2 unsupported"),
    (dict(tables=False), "null table"), (dict(tables=False, lab=0), "null table"), (dict(kx=7), "taps per column / row"),
    (dict(mask=16), "maskLabel flags 16"), (dict(stats=2), "statistics 2 out of range"), (dict(train=2), "train 2"),
])
def test_plan_time_refusals(kw, msg):
    h = L.planner_handle(256)
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(h, _rec(**kw))
    assert L.op_workspace(h, _rec(H=60, W=80)) == 4 * 32 * 8 * 2          # a factor of exactly 8 is inside


def test_python_refusals():
    assert robocupvision_amd.prepare_rgb_batch is D.prepare_rgb_batch and robocupvision_amd.draw_color_jitter is D.draw_color_jitter
    assert robocupvision_amd.SSDataSet is D.SSDataSet and {"prepare_rgb_batch", "draw_color_jitter", "SSDataSet"} <= set(D.__all__)
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    lab = torch.zeros(2, 24, 32, dtype=torch.int32)
    rows = _draw(1, 2)
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_rgb_batch(f, lab, 2, params=rows)          # CPU tensors: there is no CPU path
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_rgb_batch(f, None, 1, train=False)
    with pytest.raises(TypeError):
        D.prepare_rgb_batch(f.float(), lab, 2, params=rows)
    with pytest.raises(TypeError):
        D.prepare_rgb_batch(f, lab.long(), 2, params=rows)
    with pytest.raises(TypeError):
        D.prepare_rgb_batch(f, lab, 2, params=torch.zeros(2, 8))          # the rows of draw_jitter are not these
    with pytest.raises(ValueError):
        D.prepare_rgb_batch(f[:, :, :, :2], lab, 2, params=rows)
    with pytest.raises(ValueError):
        D.prepare_rgb_batch(f, lab[:1], 2, params=rows)
    with pytest.raises(ValueError, match="params"):
        D.prepare_rgb_batch(f, lab, 2)
    with pytest.raises(ValueError, match="scale"):
        D.prepare_rgb_batch(f, lab, 0.5, params=rows)
    with pytest.raises(ValueError, match="exactly one axis"):
        D.prepare_rgb_batch(f, lab, params=rows, img_size=(24, 16))
    bad = rows.clone()
    bad[1, 3:7] = torch.tensor([1.0, 1.0, 2.0, 3.0])          # contrast twice: one mean cannot serve both
    with pytest.raises(ValueError, match="each at most once"):
        D.prepare_rgb_batch(f, lab, 2, params=bad)
    bad = rows.clone()
    bad[0, 2] = 5
    with pytest.raises(ValueError, match="n_ops"):
        D.prepare_rgb_batch(f, lab, 2, params=bad)


def _tree(root, names, txt, split):
    os.makedirs(os.path.join(root, split, "images"))
    os.makedirs(os.path.join(root, split, "labels"))
    for name in names:
        for sub in ("images", "labels"):
            open(os.path.join(root, split, sub, name), "wb").close()
        if name in txt:
            with open(os.path.join(root, split, "images", name[:-4] + ".txt"), "w") as f:
                f.write(txt[name])


def test_dataset_listing_and_decoding(tmp_path):
    lst = META["listing"]
    root = str(tmp_path / "data")
    _tree(root, lst["files"], lst["txt"], "train")
    _tree(root, lst["files"], {k: v for k, v in lst["txt"].items() if k != lst["files"][0]}, "val")
    for cam, want in lst["cameras"].items():
        ds = D.SSDataSet(root, "train", camera=cam)
        assert ds.images == want and ds.labels == want and len(ds) == len(want)
    assert D.SSDataSet(root, "val", camera="top").images == lst["cameras"]["both"]      # a missing .txt: no filter (dataset.py:153,160)
    fr, lb = R.synthetic_frames(2, 9, 11, 4, full_range_labels=True)
    root2 = str(tmp_path / "d2")
    base = os.path.join(root2, "val")
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "labels"))
    for i in range(2):
        Image.fromarray(fr[i]).save(os.path.join(base, "images", "f%d.png" % i))
        Image.fromarray(lb[i].astype(np.uint8)).save(os.path.join(base, "labels", "f%d.png" % i))
    ds = D.SSDataSet(root2, split="val")
    assert len(ds) == 2
    for i in range(2):
        item = ds[i]
        assert len(item) == 2 and item[0].dtype == np.uint8 and item[1].dtype == np.int32
        assert np.array_equal(item[0], fr[i]) and np.array_equal(item[1], lb[i])
