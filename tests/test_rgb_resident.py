"""CPU: the RGB loader and LabelProp frame pairs from the device-resident store (RCV_OP_RGB_PREP_IDX, RCV_OP_LP_PAIR_PREP,
``RGBEpochLoader`` / ``LPDataSet`` / ``LPEpochLoader`` of robocupvision_amd/data.py) -- the restatements of the two records
(tests/rgb_resident_restatement.py) against the batch restatement and ``assemble_np``, the power of that equality (three wrong pair
forms each give other bits), ``draw_color_jitter_rows`` against ``draw_color_jitter`` bit for bit, plans and refusals on the planner
handle, the loaders' bookkeeping and the listing of LabelProp sequences.  None of it needs a device; nothing has a tolerance."""
import ctypes
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import labelprop_restatement as LR
import resident_restatement as RR
import rgb_prep_restatement as R
import rgb_resident_restatement as RG
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D

try:
    from PIL import Image
except ImportError:          # the Pillow cross-checks and the PNG listing are skipped without it; everything else runs
    Image = None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(n, seed, **kw):
    random.seed(seed)
    np.random.seed(seed)
    return D.draw_color_jitter(n, **kw).numpy()


# ------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("src,size", RR.SHAPES)
@pytest.mark.parametrize("train", [False, True])
def test_indexed_restatement_equals_batch_restatement_on_the_gathered_store(src, size, train):
    frames, labels = R.synthetic_frames(5, src[0], src[1], 21)
    flags = (True, False, True, False)
    for index in ([4, 3, 2, 1, 0], [1, 1, 4, 1], [0, 4, 2, 2, 3, 1, 0, 4, 4], [3]):
        rows = _rows(len(index), len(index)) if train else None
        gi, gt, bad = RG.prepare_rgb_indexed(frames, labels, index, size, train=train, params=rows, flags=flags)
        wi, wt = R.prepare_batch(frames[index], labels[index], size, train=train, params=rows, flags=flags)
        assert bad == 0 and np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gt, wt)
    gi, gt, bad = RG.prepare_rgb_indexed(frames, labels, [0, 5, -1, 2], size, flags=flags)
    wi, wt = R.prepare_batch(frames[[0, 2]], labels[[0, 2]], size, flags=flags)
    assert bad == 2 and not gi[1:3].any() and not gt[1:3].any()
    assert np.array_equal(_bits(gi[[0, 3]]), _bits(wi)) and np.array_equal(gt[[0, 3]], wt)


@pytest.mark.parametrize("src,size", RR.SHAPES)
@pytest.mark.parametrize("train", [False, True])
def test_pair_restatement_equals_assembly_of_the_batch_restatement(src, size, train):
    H, W = size
    frames, labels = R.synthetic_frames(5, H, W, 23)          # the store is at the network's size
    labels[2, 1, 1] = 7                                        # outside [0, 5): no class channel
    pairs = np.array([[0, 1], [3, 2], [4, 4], [1, 2]])
    rows = _rows(len(pairs), 3) if train else None
    gx, gt, bad = RG.prepare_lp_pairs(frames, labels, pairs, train=train, params=rows)
    flat = pairs.reshape(-1)
    wi, wt = R.prepare_batch(frames[flat], labels[flat], size, train=train, params=None if rows is None else np.repeat(rows, 2, 0))
    wx, wtt = LR.assemble_np(wi.reshape(len(pairs), 2, 3, H, W), wt.reshape(len(pairs), 2, H, W))
    assert bad == 0 and gx.shape == (8, 8, H, W) and np.array_equal(_bits(gx), _bits(wx)) and np.array_equal(gt, wtt)
    other = gt[[1, 0, 3, 2, 5, 4, 7, 6]] == 7                  # a sample's class channels come from the OTHER frame's label
    assert other.sum() == 2 and (gx[:, 3:].transpose(0, 2, 3, 1)[other] == -1).all()
    # a pair with one index outside the store: both samples zeros, counted once
    gx, gt, bad = RG.prepare_lp_pairs(frames, labels, [[0, 1], [2, 5], [-1, 9]], train=train, params=None if rows is None else rows[:3])
    assert bad == 2 and not gx[2:].any() and not gt[2:].any() and gx[:2].any()
    if Image is not None:          # one pair per shape through Pillow's own calls
        px, pt, _ = RG.prepare_lp_pairs(frames, labels, pairs[1:2], train=train, params=None if rows is None else rows[1:2], pillow=True)
        qx, qt, _ = RG.prepare_lp_pairs(frames, labels, pairs[1:2], train=train, params=None if rows is None else rows[1:2])
        assert np.array_equal(_bits(px), _bits(qx)) and np.array_equal(pt, qt)


def power_case():
    """A pair and a row on which a wrong pair form shows: a contrast and both flips; frames of different mean luma; label planes that
    differ and are not mirror-symmetric."""
    H, W = 16, 16
    frames, labels = R.synthetic_frames(2, H, W, 31)
    frames = frames.copy()
    frames[1] = (frames[1] // 3).astype(np.uint8)             # a much darker frame b
    labels = labels.copy()
    labels[0] = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :]) % 5
    labels[1] = (np.arange(H)[:, None] + np.arange(W)[None, :] * 2 + 1) % 5
    row = R.make_row([R.OP_BRIGHTNESS, R.OP_CONTRAST, R.OP_SATURATION, R.OP_HUE], fb=1.1, fc=0.6, fs=1.2, shift=17, hflip=True, vflip=True)
    return frames, labels, np.array([[0, 1]]), row[None]


def test_equality_tells_the_wrong_pair_forms_apart():
    frames, labels, pairs, rows = power_case()
    assert R.contrast_mean(frames[0]) != R.contrast_mean(frames[1])
    for lab in labels:
        assert not np.array_equal(lab, lab[::-1]) and not np.array_equal(lab, lab[:, ::-1]) and not np.array_equal(lab, lab[::-1, ::-1])
    assert not np.array_equal(labels[0], labels[1])
    right = RG.prepare_lp_pairs(frames, labels, pairs, train=True, params=rows)
    for variant in ("pooled_mean", "own_label", "vflip_a_only"):
        wrong = RG.prepare_lp_pairs(frames, labels, pairs, train=True, params=rows, variant=variant)
        differ = int((_bits(right[0]) != _bits(wrong[0])).sum()) + int((right[1] != wrong[1]).sum())
        assert differ > 0, variant
    # the variants are variants of the right form: with nothing to get wrong they agree with it
    calm = R.make_row([R.OP_BRIGHTNESS], fb=1.1)[None]
    for variant in ("pooled_mean", "vflip_a_only"):
        a = RG.prepare_lp_pairs(frames, labels, pairs, train=True, params=calm)
        b = RG.prepare_lp_pairs(frames, labels, pairs, train=True, params=calm, variant=variant)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]), variant


# ------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("n", [0, 1, 37])
@pytest.mark.parametrize("seeds", [(1, 1), (20261020, 3)])
@pytest.mark.parametrize("kw", [dict(), dict(vflip=False), dict(saturation=0.0), dict(hue=0.0, brightness=0.0)])
def test_draw_color_jitter_rows_equals_draw_color_jitter(n, seeds, kw):
    def seeded(fn):
        random.seed(seeds[0])
        np.random.seed(seeds[1])
        rows = fn(n, **kw)
        return rows, random.random(), int(np.random.randint(2147483647))          # the rows, and where both generators were left

    a, b = seeded(D.draw_color_jitter), seeded(D.draw_color_jitter_rows)
    assert b[0].dtype == torch.float32 and tuple(b[0].shape) == (n, 12) and b[0].device.type == "cpu"
    assert np.array_equal(_bits(a[0].numpy()), _bits(b[0].numpy()))
    assert a[1] == b[1] and a[2] == b[2]
    if n:
        want_ops = 4 - sum(1 for k in ("brightness", "contrast", "saturation", "hue") if kw.get(k, 1.0) == 0.0)
        assert bool((b[0][:, 2] == want_ops).all())
        if kw.get("vflip") is False:
            assert not b[0][:, 1].any()


# ------------------------------------------------------------------------------------------ plans and refusals
def _taps(n_in, n_out):
    return D.bilinear_table(n_in, n_out).shape[1] - 2


def _rec_idx(B=32, N=4096, Hs=120, Ws=160, H=120, W=160, lab=1, train=1, mask=0, stats=1, tables=True, kx=None, ky=None, idx=8, index=64,
             counter=64):
    t = 64 if tables else 0          # (a planner handle never reads through a pointer)
    return L.make_op(L.OP_RGB_PREP_IDX, n=B, stride=N, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, inmode2=lab, inmode=idx, aux0=train, aux1=mask, count=stats, p_x1=t, p_x2=t,
                     p_x3=t if lab else 0, p_x4=t if lab else 0, p_in_aux=index, p_epi_aux=counter)


def _rec_pair(B=8, N=4096, Hs=120, Ws=160, H=120, W=160, lab=1, train=1, stats=1, idx=8, index=64, counter=64, classes=5):
    return L.make_op(L.OP_LP_PAIR_PREP, n=B, stride=N, h=Hs, w=Ws, ho=H, wo=W, cout=classes, inmode2=lab, inmode=idx, aux0=train, count=stats,
                     p_in_aux=index, p_epi_aux=counter)


def test_plan_on_the_planner_handle():
    h = L.planner_handle(256)
    # one uint32 partial sum per workgroup of the statistics launch, which only training mode with a contrast runs
    for (Hs, Ws, H, W), groups in (((120, 160, 120, 160), 10), ((480, 640, 120, 160), 45), ((37, 70, 37, 70), 2), ((44, 280, 11, 70), 4)):
        for lab in (0, 1, 4):
            for idx in (4, 8):
                for train, stats in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    op = L.OpList([_rec_idx(B=9, N=5, Hs=Hs, Ws=Ws, H=H, W=W, lab=lab, idx=idx, train=train, stats=stats, mask=5)])
                    assert L.op_workspace(h, op.arr[0]) == (4 * 9 * groups if train and stats else 0)
                    assert op.arr[0].i[L.RCV_I_NPART] == (9 * groups if train and stats else 0) and op.labels(h) == ["rgb_prep_idx"]
    for (H, W), groups in (((120, 160), 10), ((16, 16), 1), ((37, 70), 2)):
        for lab in (1, 4):
            for idx in (4, 8):
                for train, stats in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    op = L.OpList([_rec_pair(B=3, N=7, Hs=H, Ws=W, H=H, W=W, lab=lab, idx=idx, train=train, stats=stats)])
                    assert L.op_workspace(h, op.arr[0]) == (4 * 2 * 3 * groups if train and stats else 0)          # over the 2B frames
                    assert op.labels(h) == ["lp_pair_prep"]
    for rec in (_rec_idx(), _rec_pair()):
        with pytest.raises(L.RcvError, match="planning-only handle"):
            L.OpList([rec]).run(h, 0)


@pytest.mark.parametrize("rec,kw,msg", [
    # what RCV_OP_RGB_PREP refuses
    (_rec_idx, dict(B=0), "every size must be >= 1"), (_rec_idx, dict(Ws=0, kx=3), "every size must be >= 1"),
    (_rec_idx, dict(Hs=480, Ws=640, W=79, kx=19), "shrinks an axis by more than 8"), (_rec_idx, dict(lab=2), "label element size 2 unsupported"),
    (_rec_idx, dict(tables=False), "null table"), (_rec_idx, dict(ky=5), "taps per column / row"),
    (_rec_idx, dict(mask=16), "maskLabel flags 16 / statistics 1 out of range"), (_rec_idx, dict(stats=2), "statistics 2 out of range"),
    (_rec_idx, dict(train=2), "train 2 /"), (_rec_idx, dict(N=1 << 17), "more than 2\\^31 pixels"),
    # its own
    (_rec_idx, dict(N=0), "a store of 0 images"), (_rec_idx, dict(N=-3), "a store of -3 images"),
    (_rec_idx, dict(idx=2), "index element size 2 unsupported"), (_rec_idx, dict(idx=0), "index element size 0 unsupported"),
    (_rec_idx, dict(index=0), "null index or null bad-index counter"), (_rec_idx, dict(counter=0), "null index or null bad-index counter"),
    # the pair record
    (_rec_pair, dict(classes=4), "4 classes unsupported"), (_rec_pair, dict(B=0), "every size must be >= 1"),
    (_rec_pair, dict(N=0), "a store of 0 images"), (_rec_pair, dict(Hs=480, Ws=640), "only the no-resize form is built.*ResidentDataset"),
    (_rec_pair, dict(lab=0), "label element size 0 unsupported"), (_rec_pair, dict(lab=8), "label element size 8 unsupported"),
    (_rec_pair, dict(idx=2), "index element size 2 unsupported"), (_rec_pair, dict(train=3), "train 3 / statistics 1 out of range"),
    (_rec_pair, dict(N=1 << 17), "more than 2\\^31 pixels"), (_rec_pair, dict(B=1 << 13), "more than 2\\^31 pixels"),
    (_rec_pair, dict(index=0), "null index or null bad-index counter"), (_rec_pair, dict(counter=0), "null index or null bad-index counter"),
])
def test_plan_time_refusals(rec, kw, msg):
    h = L.planner_handle(256)
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(h, rec(**kw))
    assert L.op_workspace(h, rec()) == 4 * rec().i[L.RCV_I_N] * 10 * (2 if rec is _rec_pair else 1)


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/rcv.h").read(), flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("rcv_rgb_prep_indexed", "rcv_lp_pair_prep"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTS and getattr(L.load(), name).argtypes
    assert L.OP_RGB_PREP_IDX == 53 and L.OP_LP_PAIR_PREP == 54
    assert re.search(r"RCV_OP_RGB_PREP_IDX\s*=\s*%d\b" % L.OP_RGB_PREP_IDX, src) and re.search(r"RCV_OP_LP_PAIR_PREP\s*=\s*%d\b" % L.OP_LP_PAIR_PREP, src)
    for name in ("prepare_lp_pairs", "draw_color_jitter_rows", "RGBEpochLoader", "LPDataSet", "LPEpochLoader"):
        assert getattr(robocupvision_amd, name) is getattr(D, name) and name in D.__all__


# ------------------------------------------------------------------------------------------ loaders and listing
class _Store:          # what the loaders' bookkeeping asks of a store: its length
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _windows(n):
    return torch.stack([torch.arange(n), torch.arange(n) + 1], 1)


@pytest.mark.parametrize("make", [lambda n, bs, **kw: D.RGBEpochLoader(_Store(n), bs, **kw),
                                  lambda n, bs, **kw: D.LPEpochLoader(_Store(n + 1), _windows(n), bs, **kw)], ids=["rgb", "lp"])
def test_loader_bookkeeping(make):
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(4))
    ld = make(10, 4)
    assert ld.plan(perm) == [(0, 4), (4, 8), (8, 10)] and len(ld) == 3 and torch.equal(ld.share(perm), perm)
    ld = make(10, 4, drop_last=True)
    assert ld.plan(perm) == [(0, 4), (4, 8)] and len(ld) == 2
    parts = []
    for rank in (0, 1):
        ld = make(10, 4, rank=rank, world=2)
        assert ld.plan(perm) == [(0, 4), (4, 5)] and len(ld) == 2 and torch.equal(ld.share(perm), perm[rank::2])
        parts.append(torch.cat([ld.share(perm)[a:b] for a, b in ld.plan(perm)]))
    assert sorted(torch.cat(parts).tolist()) == list(range(10)) and len(set(parts[0].tolist()) & set(parts[1].tolist())) == 0
    assert [len(make(10, 4, rank=r, world=3)) for r in range(3)] == [1, 1, 1] and len(make(8, 4, drop_last=True)) == 2
    for kw in (dict(bs=0), dict(bs=4, rank=2, world=2), dict(bs=4, world=0)):
        with pytest.raises(ValueError):
            make(10, **kw)


def test_lp_loader_refuses_longer_windows():
    with pytest.raises(ValueError, match="windows of 3 frames: only pairs are built"):
        D.LPEpochLoader(_Store(5), torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(TypeError):
        D.LPEpochLoader(_Store(5), torch.zeros(3, 2))
    with pytest.raises(TypeError):
        D.LPEpochLoader(_Store(5), [[0, 1]])
    assert D.LPEpochLoader(_Store(5), _windows(4)).batch_size == 8          # labelPropTrain.py's batch


@pytest.mark.skipif(Image is None, reason="the PNG tree is written with Pillow")
def test_lp_dataset_listing(tmp_path):
    rng = np.random.RandomState(5)
    names = {"seq10": ["1.png", "2.png", "10.png"], "seq2": ["7.png", "8.png", "9.png", "100.png"]}
    written = {}
    for d, files in names.items():
        for sub in ("images", "labels"):
            (tmp_path / "LabelProp" / "Real" / "train" / d / sub).mkdir(parents=True)
        for f in files:
            frame = rng.randint(0, 256, (6, 8, 3)).astype(np.uint8)
            label = rng.randint(0, 5, (6, 8)).astype(np.uint8)
            Image.fromarray(frame).save(str(tmp_path / "LabelProp" / "Real" / "train" / d / "images" / f))
            Image.fromarray(label).save(str(tmp_path / "LabelProp" / "Real" / "train" / d / "labels" / f))
            written[(d, f)] = (frame, label)
    (tmp_path / "LabelProp" / "Real" / "train" / "notes.txt").write_text("not a directory")
    ds = D.LPDataSet(str(tmp_path), train=True, finetune=True)
    # directories and files in natural-key order: seq2 before seq10, 2.png before 10.png, 9.png before 100.png
    order = [("seq2", f) for f in names["seq2"]] + [("seq10", f) for f in names["seq10"]]
    assert len(ds) == 5 and len(ds.frames) == 7 and ds.windows.dtype == torch.int64
    assert ds.windows.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5], [5, 6]]          # none crosses the directory boundary between 3 and 4
    assert [len(x) for x in ds.images] == [4, 3] and [len(x) for x in ds.labels] == [4, 3]
    for i, key in enumerate(order):
        frame, label = ds.frames[i]
        assert frame.dtype == np.uint8 and frame.shape == (6, 8, 3) and label.dtype == np.int32 and label.shape == (6, 8)
        assert np.array_equal(frame, written[key][0]) and np.array_equal(label, written[key][1])
    assert D.LPDataSet(str(tmp_path), len_seq=3).windows.tolist() == [[0, 1, 2], [1, 2, 3], [4, 5, 6]]
    assert len(D.LPDataSet(str(tmp_path), len_seq=4)) == 1 and len(D.LPDataSet(str(tmp_path), train=False)) == 0
    assert len(D.LPDataSet(str(tmp_path), finetune=False)) == 0 and tuple(D.LPDataSet(str(tmp_path), train=False).windows.shape) == (0, 2)
    with pytest.raises(NotImplementedError, match="cv2.cvtColor"):
        ds[0]


def test_python_refusals():
    f = torch.zeros(3, 16, 16, 3, dtype=torch.uint8)
    lab = torch.zeros(3, 16, 16, dtype=torch.uint8)
    idx = torch.zeros(2, dtype=torch.int64)
    pairs = torch.zeros(2, 2, dtype=torch.int64)
    rows = torch.zeros(2, 12)
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_rgb_batch(f, lab, img_size=(16, 16), index=idx, params=rows)          # CPU tensors: there is no CPU path
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_lp_pairs(f, lab, pairs, params=rows)
    with pytest.raises(TypeError, match="uint8"):
        D.prepare_lp_pairs(f.float(), lab, pairs, params=rows)
    with pytest.raises(TypeError, match="uint8 or int32"):
        D.prepare_lp_pairs(f, lab.long(), pairs, params=rows)
    with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
        D.prepare_lp_pairs(f, lab[:2], pairs, params=rows)
    with pytest.raises(ValueError, match="num_class must be 5"):
        D.prepare_lp_pairs(f, lab, pairs, params=rows, num_class=4)
    for bad_pairs in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(2, 2), torch.zeros(0, 2, dtype=torch.int64)):
        with pytest.raises(TypeError, match=r"pairs must be a non-empty int32 or int64 \[B,2\]"):
            D.prepare_lp_pairs(f, lab, bad_pairs, params=rows)
    for bad_index in (torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2), torch.zeros(0, dtype=torch.int32)):
        with pytest.raises(TypeError, match=r"index must be a non-empty int32 or int64 \[B\]"):
            D.prepare_rgb_batch(f, lab, img_size=(16, 16), index=bad_index, params=rows)
    for bad_params in (torch.zeros(3, 12), torch.zeros(2, 8), torch.zeros(2, 12, dtype=torch.float64)):
        with pytest.raises(TypeError, match=r"float32 \[B,12\]"):
            D.prepare_lp_pairs(f, lab, pairs, params=bad_params)
        with pytest.raises(TypeError, match=r"float32 \[B,12\]"):
            D.prepare_rgb_batch(f, lab, img_size=(16, 16), index=idx, params=bad_params)
    with pytest.raises(ValueError, match="needs params"):
        D.prepare_lp_pairs(f, lab, pairs)
    twice = torch.zeros(2, 12)
    twice[1, 2:5] = torch.tensor([2.0, 1.0, 1.0])          # a contrast twice
    for call in (lambda: D.prepare_lp_pairs(f, lab, pairs, params=twice), lambda: D.prepare_rgb_batch(f, lab, img_size=(16, 16), index=idx, params=twice)):
        with pytest.raises(ValueError, match="row 1: n_ops 2.0 with operations"):
            call()
    ok_row = np.stack([R.make_row([R.OP_HUE, R.OP_CONTRAST]), R.make_row([R.OP_BRIGHTNESS])])
    assert D._check_color_rows(ok_row, "x").tolist() == [True, False]
