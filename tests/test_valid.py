"""Validation on the device (RCV_OP_CLS_VALID, RCV_OP_VALID_FOLD, ``model.validate``, ``metrics.ValidationState``,
``Trainer.validate``) without a device: the float64 restatement (tests/valid_restatement.py) pinned to the oracle's valid_metrics and to
a literal torch rendering of train.py:136-164, the proof that it tells three wrong readings of the source apart, what the library's
query accepts and refuses, and the argument errors of the Python surface."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import small_ops_cases as K      # noqa: E402
import small_ops_restatement as SR      # noqa: E402
import valid_restatement as V      # noqa: E402
import robocupvision_amd.model as M      # noqa: E402
from oracle import cpu_reference as O      # noqa: E402
from robocupvision_amd import _lib as L      # noqa: E402
from robocupvision_amd import metrics      # noqa: E402
from robocupvision_amd.train import Trainer      # noqa: E402

PLANES = [(3, 5, 7), (2, 17, 31)]
CLASSES = (2, 3, 5, 8)


def _maps(N, H, W, C, seed):
    """Class maps and labels inside [0, C), every class labelled and predicted somewhere."""
    rng = np.random.default_rng(seed)
    pred, tgt = rng.integers(0, C, (N, H, W)), rng.integers(0, C, (N, H, W))
    pred.reshape(-1)[:C] = np.arange(C)
    tgt.reshape(-1)[-C:] = np.arange(C)
    return pred, tgt


# ------------------------------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize("plane", PLANES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", CLASSES)
def test_restatement_equals_the_oracles_valid_metrics(plane, C):
    """oracle.cpu_reference.valid_metrics keeps the reference's fp32 accumulators: at most N * C terms of at most 1 per sum and one
    division, each rounded to 2^-24 relative -> 1e-5 relative covers 48 terms eight times over."""
    N, H, W = plane
    pred, tgt = _maps(N, H, W, C, 100 + C)
    ref = O.valid_metrics(torch.from_numpy(pred), torch.from_numpy(tgt), C)
    _, got = V.valid_pass([(pred, tgt, 0.0)], C)
    for k in ("pixel_acc", "mean_class_acc", "mean_iou"):
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, got[k], ref[k])
    assert np.allclose(got["confusion_percent"], ref["confusion_percent"].double().numpy(), rtol=1e-5, atol=0)
    assert np.array_equal(V.counts(pred, tgt, C), SR.confusion(pred, tgt, C))
    assert got["score"] == (got["mean_class_acc"] + got["mean_iou"]) / 2 and got["images"] == N and got["batches"] == 1


def _literal_valid(batches, C):
    """train.py:104-164 with torch masks, the accumulators in float64 (the reference's are fp32 tensors)."""
    conf, iou, lab_cnts = torch.zeros(C, C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    running_acc, img_cnt, losstotal = 0.0, 0, 0.0
    for pred_class, targets, loss in batches:
        pred_class, targets = torch.from_numpy(np.asarray(pred_class).astype(np.int64)), torch.from_numpy(np.asarray(targets).astype(np.int64))
        b_size = pred_class.shape[0]
        running_acc += torch.sum(pred_class == targets).item()
        losstotal += float(np.float32(loss))
        img_cnt += b_size
        mask_pred = torch.zeros(C, *pred_class.shape).long()
        mask_target = torch.zeros(C, *pred_class.shape).long()
        for c in range(C):
            mask_pred[c] = pred_class == c
            mask_target[c] = targets == c
        for img in range(b_size):
            for lab in range(C):
                lab_cnts[lab] += torch.sum(mask_target[lab, img]).item()
                for prd in range(C):
                    inter = torch.sum(mask_pred[prd, img] & mask_target[lab, img]).item()
                    conf[(prd, lab)] += inter
                    if lab == prd:
                        union = torch.sum(mask_pred[prd, img] | mask_target[lab, img]).item()
                        if union == 0:
                            iou[lab] += 1
                        else:
                            iou[lab] += inter / union
    counts = conf.clone()
    for lab in range(C):
        for prd in range(C):
            conf[(prd, lab)] /= (lab_cnts[lab] / 100.0)
    mean_iou = torch.sum(iou / img_cnt).item() / C * 100
    mean_class_acc = 0.0
    for j in range(C):
        mean_class_acc += conf[(j, j)].item() / C
    return dict(iou=iou.numpy(), counts=counts.numpy(), percent=conf.numpy(), mean_iou=mean_iou, mean_class_acc=mean_class_acc,
                correct=running_acc, loss=losstotal / len(batches), images=img_cnt)


def _odd_batches(C=5, odd=True):
    """Three batches of different N; class 3 is absent from image 0 of batch 0 in both maps (union 0 -> 1), class 4 is labelled
    nowhere (NaN); the labels of small_ops_cases.CONF_ODD_LABELS are all present, or with ``odd`` off replaced by class 0."""
    out = []
    for k, (N, H, W) in enumerate([(3, 5, 7), (2, 17, 31), (1, 5, 7)]):
        pred, tgt = K.build_confusion(N, H, W, C, seed=k)
        pred, tgt = np.minimum(pred, C - 1), tgt.copy()          # (a network's class is always < C; the labels keep their odd values)
        tgt[tgt == 4] = 0
        if not odd:
            tgt[(tgt < 0) | (tgt >= C)] = 0
        if k == 0:
            pred[0][pred[0] == 3] = 1
            tgt[0][tgt[0] == 3] = 2
        out.append((pred, tgt, np.float32(0.3 + 0.1 * k)))
    return out


def test_restatement_equals_the_literal_loop_bit_for_bit():
    C = 5
    batches = _odd_batches(C, odd=False)
    state, got = V.valid_pass(batches, C)
    ref = _literal_valid(batches, C)
    assert np.array_equal(state[4:4 + C], ref["iou"])                                  # the same additions in the same order
    assert np.array_equal(got["confusion"], ref["counts"].astype(np.int64))
    assert np.array_equal(got["confusion_percent"], ref["percent"], equal_nan=True)
    assert got["mean_iou"] == ref["mean_iou"] and got["loss"] == ref["loss"] and got["images"] == ref["images"] == 6
    assert math.isnan(got["mean_class_acc"]) and math.isnan(ref["mean_class_acc"]) and math.isnan(got["score"])      # class 4: 0 / 0
    assert np.isnan(got["confusion_percent"][:, 4]).all() and not np.isnan(got["confusion_percent"][:, :4]).any()
    pixels = sum(np.asarray(p).size for p, _, _ in batches)
    assert state[3] == pixels and got["pixel_acc"] == 100.0 * ref["correct"] / pixels
    # union 0 -> 1 happened: class 3 of image 0 of batch 0, class 4 of ... (predicted somewhere? then its union is not 0)
    c0 = V.counts(batches[0][0], batches[0][1], C)[0]
    assert c0[3, :].sum() + c0[:, 3].sum() == 0
    # labels outside the classes (maskLabel, -100): counts, loss and the accuracy over ALL pixels stay the literal loop's; the union
    # is formed from the counts, which hold no pixel with such a label, where train.py:149 still sees the prediction under it
    odd = _odd_batches(C)
    so, go = V.valid_pass(odd, C)
    ro = _literal_valid(odd, C)
    assert np.array_equal(go["confusion"], ro["counts"].astype(np.int64)) and go["pixel_acc"] == 100.0 * ro["correct"] / so[3]
    assert go["pixel_acc"] < got["pixel_acc"] and (so[4:4 + C] >= ro["iou"]).all() and (so[4:4 + C] <= ro["iou"] * 1.15).all()
    # the library's host arithmetic is the same arithmetic
    rep = metrics.validation_report(state.tolist(), C)
    for k in ("loss", "pixel_acc", "mean_iou", "images", "batches"):
        assert rep[k] == got[k], k
    assert math.isnan(rep["mean_class_acc"]) and math.isnan(rep["score"])
    assert np.array_equal(rep["confusion"].numpy(), got["confusion"]) and rep["confusion"].dtype == torch.int64
    assert np.array_equal(rep["confusion_percent"].numpy(), got["confusion_percent"], equal_nan=True)
    # ... and without a NaN class
    full = [(p, np.where(t == 0, np.where(p == 4, 4, 0), t), l) for p, t, l in batches]
    s2, g2 = V.valid_pass(full, C)
    r2 = metrics.validation_report(s2.tolist(), C)
    assert not math.isnan(g2["score"]) and all(r2[k] == g2[k] for k in ("loss", "pixel_acc", "mean_class_acc", "mean_iou", "score"))
    assert g2["mean_class_acc"] == _literal_valid(full, C)["mean_class_acc"]


@pytest.mark.parametrize("variant,key", [("iou_summed", "mean_iou"), ("acc_in_range", "pixel_acc"), ("union0_zero", "mean_iou")])
def test_wrong_readings_leave_the_restatement(variant, key):
    batches = _odd_batches(5)
    labels = np.concatenate([t.ravel() for _, t, _ in batches])
    for v in K.CONF_ODD_LABELS:
        assert ((labels == (5 if v is None else v))).any()
    _, good = V.valid_pass(batches, 5)
    _, bad = V.valid_pass(batches, 5, variant)
    assert good[key] != bad[key], (variant, good[key], bad[key])
    assert abs(good[key] - bad[key]) > 1e-3 * abs(good[key])


# ------------------------------------------------------------------------------------------ the library's query
def _op(n=2, h=3, w=4, cin=8, cout=5, inmode=0, flags=0, **kw):
    return L.make_op(L.OP_CLS_VALID, flags, n=n, h=h, w=w, cin=cin, cout=cout, inmode=inmode, **kw)


def _fold(n=2, h=3, w=4, cout=5, npart=0, **kw):
    return L.make_op(L.OP_VALID_FOLD, 0, n=n, h=h, w=w, cout=cout, npart=npart, **kw)


def _label(op):
    return L.OpList([op]).labels(L.planner_handle(256))[0]


def test_the_op_kinds_and_entry_points_exist():
    assert (L.OP_CLS_VALID, L.OP_VALID_FOLD, L.VALID_STATE) == (60, 61, 76)
    assert {"rcv_cls_valid", "rcv_valid_fold"} <= set(L.EXPORTS) and L.load().rcv_cls_valid.argtypes and L.load().rcv_valid_fold.argtypes
    assert hasattr(M.ROBO_UNet, "validate") and hasattr(Trainer, "validate") and hasattr(metrics, "ValidationState")


def test_the_query_sizes_the_partial_rows():
    h = L.planner_handle(256)
    for kw, per in ((dict(cin=8), 256), (dict(cin=16), 64), (dict(cin=8, inmode=1), 256), (dict(cin=16, flags=L.F_FUSED_UP, aux1=8), 64),
                    (dict(cin=8, flags=L.F_FUSED_UP, aux0=L.LOAD_AFFINE_RELU), 256)):
        for (n, hh, ww) in ((1, 1, 1), (2, 17, 31), (64, 120, 160)):
            op = _op(n=n, h=hh, w=ww, **kw)
            rows = min((n * hh * ww + per - 1) // per, 1024)
            assert L.op_workspace(h, op) == rows * 12 and op.i[L.RCV_I_NPART] == rows
            assert _label(op) == "cls_valid"
            if per == 256:      # the lane-per-pixel forms keep RCV_OP_CE_FWD's grid
                ce = L.make_op(L.OP_CE_FWD, 0, n=n, h=hh, w=ww, cout=5)
                assert L.op_workspace(h, ce) == rows * 12
    op = _op(inmode=2, cin=1)
    assert L.op_workspace(h, op) == 0 and op.i[L.RCV_I_NPART] == 0
    for c in range(1, 9):
        _label(_op(cout=c))
        _label(_fold(cout=c, p_x0=64))
    fold = _fold(npart=7, p_in2=64)
    assert _label(fold) == "valid_fold" and L.op_workspace(h, fold) == 0 and fold.i[L.RCV_I_NPART] == 7      # the row count is an input: kept


@pytest.mark.parametrize("op,what", [
    (lambda: _op(inmode=3), "source form 3 unknown"),
    (lambda: _op(inmode=-1), "source form -1 unknown"),
    (lambda: _op(cin=4), "4 input channels unsupported (8 or 16)"),
    (lambda: _op(cin=12), "12 input channels unsupported (8 or 16)"),
    (lambda: _op(cin=32), "32 input channels unsupported (8 or 16)"),
    (lambda: _op(cout=9), "9 classes unsupported (1..8)"),
    (lambda: _op(cout=0), "0 classes unsupported (1..8)"),
    (lambda: _op(n=0), "every size must be >= 1"),
    (lambda: _op(n=8, h=16384, w=16384), "N*H*W < 2^31"),
    (lambda: _op(inmode=1, cin=6), "6 floats per pixel for 5 classes"),
    (lambda: _op(inmode=1, cin=4), "4 floats per pixel for 5 classes"),
    (lambda: _op(inmode=1, flags=L.F_FUSED_UP), "RCV_F_FUSED_UP belongs to source form 0"),
    (lambda: _op(flags=L.F_FUSED_UP, aux1=6), "6 skip channels for 8 inputs"),
    (lambda: _op(flags=L.F_FUSED_UP, aux0=2), "skip load mode 2"),
    (lambda: _op(inmode=2, cin=1, p_part=64), "no loss is formed, so no partial rows"),
    (lambda: _op(inmode=2, cin=1, npart=3), "no loss is formed, so no partial rows"),
    (lambda: _fold(npart=3, p_in2=64, p_x0=64), "exactly one loss source"),
    (lambda: _fold(npart=0), "exactly one loss source"),
    (lambda: _fold(npart=0, p_in2=64), "0 partial rows with p[IN2] set"),
    (lambda: _fold(npart=3, p_x0=64), "3 partial rows with a scalar loss"),
    (lambda: _fold(cout=9, p_x0=64), "9 classes unsupported (1..8)"),
    (lambda: _fold(n=0, p_x0=64), "every size must be >= 1"),
])
def test_the_query_refuses_with_a_message(op, what):
    with pytest.raises(L.RcvError) as e:
        _label(op())
    assert what in str(e.value), str(e.value)
    with pytest.raises(L.RcvError) as e:      # the workspace query refuses the same records with the same words
        L.op_workspace(L.planner_handle(256), op())
    assert what in str(e.value), str(e.value)


def test_a_planner_handle_enqueues_nothing():
    lib = L.load()
    assert lib.rcv_valid_fold(L.planner_handle(256), None, None, 0, None, 2, 3, 4, 5, None, None) != 0
    assert lib.rcv_cls_valid(L.planner_handle(256), None, None, None, 2, 3, 4, 8, 5, None, None, None, None, None, 1 << 20, None, None) != 0


# ------------------------------------------------------------------------------------------ argument errors of the Python surface
class _FakeState:
    C = 5
    buf = torch.zeros(76, dtype=torch.float64)

    def counts_for(self, n):
        return torch.zeros(n, 5, 5, dtype=torch.int32)


def test_model_validate_argument_errors():
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16, dtype=torch.int64)
    m = M.ROBO_UNet()
    with pytest.raises(L.RcvError, match="training mode"):
        m.train().validate(x, t, _FakeState())
    m.eval()
    with pytest.raises(L.RcvError, match="HIP device only"):
        m.validate(x, t, _FakeState())
    with pytest.raises(TypeError, match="tensors"):
        m.validate(x.numpy(), t, _FakeState())
    with pytest.raises(TypeError, match="tensors"):
        m.validate(x, None, _FakeState())
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN(32, 5, 1, False, 1).eval().validate(x, t, _FakeState())
    with pytest.raises(L.RcvError, match="no per-pixel classifier"):
        M.Pool(8).eval().validate(x, t, _FakeState())


def test_validation_state_argument_errors():
    for bad in (0, 9, -1, 5.0, None):
        with pytest.raises(ValueError, match="1..8 classes"):
            metrics.ValidationState(bad)
    with pytest.raises(L.RcvError, match="HIP device"):
        metrics.ValidationState(5, "cpu")


def test_trainer_validate_argument_errors():
    with pytest.raises(L.RcvError, match="HIP device"):
        Trainer(M.ROBO_UNet())
    tr = Trainer.__new__(Trainer)          # the argument checks come before anything touches a device
    tr.model, tr.criterion, tr.optimizer, tr.prune_indices = M.ROBO_UNet().eval(), M.CrossEntropyLoss2d(), None, None
    with pytest.raises(TypeError, match="ValidationState"):
        tr.validate([], state=torch.zeros(76))
    with pytest.raises(TypeError, match="iterable"):
        tr.validate(3)
    with pytest.raises(ValueError, match="no batches"):
        tr.validate([])
    with pytest.raises(L.RcvError, match="HIP device"):
        tr.validate([(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64))])
