"""CPU: the batch preparation (RCV_OP_BATCH_PREP, robocupvision_amd/data.py) -- the NumPy restatement against live Pillow and against
the reference's goldens (tests/golden/make_golden_batch_prep.py), the library's host tables against the restatement's, ``draw_jitter``
against the draws the reference made, the plan-time refusals on the planner handle, the Python-level refusals and the file listing."""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
import batch_prep_restatement as R
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D

with open(os.path.join(GOLDEN, "batch_prep.json")) as _f:
    META = json.load(_f)
KATS = np.load(os.path.join(GOLDEN, "batch_prep.npz"))


def _sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("src,size", R.SHAPE_PAIRS)
def test_restatement_equals_pillow(src, size):
    frames, labels = R.synthetic_frames(1, src[0], src[1], 3, full_range_labels=True)
    want = np.asarray(Image.fromarray(frames[0]).resize((size[1], size[0]), Image.BILINEAR))
    got = R.resize_bilinear(frames[0], size)
    assert got.dtype == np.uint8 and got.shape == want.shape and int((got != want).sum()) == 0
    lab = Image.fromarray(labels[0].astype(np.uint8)).convert("I")
    want_l = np.asarray(lab.resize((size[1], size[0]), Image.NEAREST))
    assert int((R.resize_nearest(labels[0], size) != want_l).sum()) == 0


@pytest.mark.parametrize("tag", sorted(META["configs"]))
def test_restatement_equals_goldens(tag):
    c = META["configs"][tag]
    B, size, ft = c["B"], tuple(c["size"]), c["finetune"]
    frames, labels = R.synthetic_frames(B, c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"], cover_size=size)
    # validation path: bit for bit
    vi, vt = R.prepare_batch(frames, labels, size, finetune=ft, train=False)
    assert np.array_equal(_bits(vi), _bits(KATS[tag + "/val_imgs"])) and np.array_equal(vt, KATS[tag + "/val_labels"].astype(np.int64))
    assert _sha(vi, vt) == c["val_sha256"]
    # maskLabel, all 16 flag sets
    for k, flags in enumerate(R.FLAG_SETS):
        assert np.array_equal(R.mask_label(vt, *flags), KATS[tag + "/masked"][k].astype(np.int64)), flags
    # training path: labels and Y bit for bit, U / V within 2^-22 (|m0 U| + |m1 V|): both sides are within 2^-23 of exact
    rows = KATS[tag + "/params"]
    ti, tt = R.prepare_batch(frames, labels, size, finetune=ft, train=True, params=rows)
    gi = KATS[tag + "/train_imgs"]
    assert np.array_equal(tt, KATS[tag + "/train_labels"].astype(np.int64))
    assert np.array_equal(_bits(ti[:, 0]), _bits(gi[:, 0]))
    for b in range(B):
        small = R.resize_bilinear(frames[b], size)
        bound = 2.0 ** -22 * R.uv_bound(small, ft, rows[b], rows[b, 0] != 0)
        err = np.abs(ti[b, 1:].astype(np.float64) - gi[b, 1:].astype(np.float64))
        assert bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("tag", sorted(META["full"]))
def test_restatement_full_size_sha(tag):
    c = META["full"][tag]
    frames, labels = R.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"])
    vi, vt = R.prepare_batch(frames, labels, tuple(c["size"]), train=False)
    assert _sha(vi, vt) == c["val_sha256"]


@pytest.mark.parametrize("tag", sorted(META["configs"]))
def test_draw_jitter_reproduces_the_reference_draws(tag):
    c = META["configs"][tag]
    random.seed(c["draw_seed"])
    torch.manual_seed(c["draw_seed"])
    rows = D.draw_jitter(c["B"])
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (c["B"], 8) and rows.device.type == "cpu"
    assert np.array_equal(_bits(rows.numpy()), _bits(KATS[tag + "/params"]))
    assert [int(v) for v in rows[:, 0]] == c["flips"]


def test_draw_jitter_matrix_off_still_draws():
    random.seed(5)
    torch.manual_seed(5)
    on = D.draw_jitter(3)
    random.seed(5)
    torch.manual_seed(5)
    off = D.draw_jitter(3, h=0.0)
    assert bool((off[:, 7] == 1).all()) and bool((on[:, 7] == 0).all())
    assert torch.equal(on[:, :3], off[:, :3])          # the same stream of draws: flip, b_val, c_val of every image are unchanged


@pytest.mark.parametrize("src,size", R.SHAPE_PAIRS + [((24, 32), (24, 32))])
def test_library_tables_equal_restatement(src, size):
    for n_in, n_out in ((src[1], size[1]), (src[0], size[0])):
        tab = D.bilinear_table(n_in, n_out)
        assert tab.dtype == np.int32
        if n_in == n_out:
            assert np.array_equal(tab[:, 0], np.arange(n_out)) and bool((tab[:, 1] == 1).all()) and bool((tab[:, 2] == 1 << 22).all())
            assert not tab[:, 3:].any()
        else:
            first, count, coef = R.bilinear_coeffs(n_in, n_out)
            assert np.array_equal(tab[:, 0], first) and np.array_equal(tab[:, 1], count) and np.array_equal(tab[:, 2:], coef)
        assert np.array_equal(D.nearest_table(n_in, n_out), R.nearest_index(n_in, n_out))
    for ft in (False, True):
        assert torch.equal(D.norm_table(ft), R.norm_table(ft))
        assert D.MEAN[ft] == R.MEAN[ft] and D.STD[ft] == R.STD[ft]


def _taps(n_in, n_out):
    return D.bilinear_table(n_in, n_out).shape[1] - 2


def _rec(B=64, Hs=480, Ws=640, H=120, W=160, lab=4, train=1, mask=0, tables=True, kx=None, ky=None):
    t = 64 if tables else 0          # (a planner handle never reads through a pointer)
    return L.make_op(L.OP_BATCH_PREP, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, inmode2=lab, aux0=train, aux1=mask, p_x1=t, p_x2=t, p_x3=t, p_x4=t, p_x5=t)


@pytest.mark.parametrize("B,H,W", [(64, 120, 160), (32, 240, 320), (32, 480, 640)])
def test_plan_on_the_planner_handle(B, H, W):
    h = L.planner_handle(256)
    for lab in (1, 4):
        for train in (0, 1):
            op = L.OpList([_rec(B=B, H=H, W=W, lab=lab, train=train, mask=5)])
            assert L.op_workspace(h, op.arr[0]) == 0
            assert op.labels(h) == ["batch_prep"]
    with pytest.raises(L.RcvError, match="planning-only handle"):
        L.OpList([_rec(B=B, H=H, W=W)]).run(h, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), "every size must be >= 1"), (dict(H=0, ky=3), "every size must be >= 1"), (dict(W=0, kx=3), "every size must be >= 1"),
    (dict(Hs=0, ky=3), "every size must be >= 1"), (dict(Ws=0, kx=3), "every size must be >= 1"),
    (dict(H=59, ky=19), "shrinks an axis by more than 8"), (dict(W=79, kx=19), "shrinks an axis by more than 8"),
    (dict(lab=8), "label element size 8 unsupported"), (dict(lab=2), "label element size 2 unsupported"),
    (dict(tables=False), "null table"), (dict(kx=7), "taps per column / row"), (dict(mask=16), "maskLabel flags 16 out of range"),
])
def test_plan_time_refusals(kw, msg):
    h = L.planner_handle(256)
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(h, _rec(**kw))
    # a factor of exactly 8 is inside
    assert L.op_workspace(h, _rec(H=60, W=80)) == 0


def test_python_refusals():
    assert robocupvision_amd.prepare_batch is D.prepare_batch and robocupvision_amd.draw_jitter is D.draw_jitter
    assert robocupvision_amd.SSYUVDataset is D.SSYUVDataset and robocupvision_amd.data is D
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    lab = torch.zeros(2, 24, 32, dtype=torch.int32)
    rows = torch.zeros(2, 8)
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_batch(f, lab, (12, 16), params=rows)          # CPU tensors: there is no CPU path
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_batch(f, lab.to(torch.uint8), (24, 32), train=False)
    with pytest.raises(TypeError):
        D.prepare_batch(f.float(), lab, (12, 16), params=rows)
    with pytest.raises(TypeError):
        D.prepare_batch(f, lab.long(), (12, 16), params=rows)
    with pytest.raises(ValueError):
        D.prepare_batch(f[:, :, :, :2], lab, (12, 16), params=rows)
    with pytest.raises(ValueError):
        D.prepare_batch(f, lab[:1], (12, 16), params=rows)
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.prepare_batch(f, lab, (24, 16), params=rows)          # exactly one axis kept: the reference's quirk is refused by name
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.prepare_batch(f, lab, (12, 32), train=False)


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
        ds = D.SSYUVDataset(root, train=True, camera=cam)
        assert ds.images == want and ds.labels == want and len(ds) == len(want)
    assert D.SSYUVDataset(root, train=False, camera="top").images == lst["val_without_one_txt"]
    # decoding: what Image.open(..).convert('RGB') / .convert('I') hold, and nothing else
    fr, lb = R.synthetic_frames(2, 9, 11, 4, full_range_labels=True)
    root2 = str(tmp_path / "ft")
    base = os.path.join(root2, "FinetuneHorizon", "val")
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "labels"))
    for i in range(2):
        Image.fromarray(fr[i]).save(os.path.join(base, "images", "f%d.png" % i))
        Image.fromarray(lb[i].astype(np.uint8)).save(os.path.join(base, "labels", "f%d.png" % i))
    ds = D.SSYUVDataset(root2, train=False, finetune=True)
    assert len(ds) == 2
    for i in range(2):
        item = ds[i]
        assert len(item) == 2 and item[0].dtype == np.uint8 and item[1].dtype == np.int32
        assert np.array_equal(item[0], fr[i]) and np.array_equal(item[1], lb[i])
