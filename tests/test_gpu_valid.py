"""GPU: validation on the device (RCV_OP_CLS_VALID, RCV_OP_VALID_FOLD, ``model.validate``, ``metrics.ValidationState``,
``Trainer.validate``).

Record level, through rcv_run on hand-made operands (tests/segment_restatement.py's random cases; labels of
small_ops_cases.build_confusion: about 5 % outside [0, C), 2^32 + 1 and -2^32 + 2 among them):
  * the class map equals RCV_OP_CLS_LABEL's on the same operands, exactly;
  * the counts equal small_ops_restatement.confusion of that map, exactly, and a second run into the same counts doubles them;
  * the loss rows, finalised, are within 1e-5 relative of small_ops_restatement.cross_entropy (float64) on the logits RCV_OP_CLS_FWD
    (RCV_OP_NHWC_TO_NCHW for the logits form) writes -- the bar of test_cross_entropy_beyond_a_streaming_pass;
  * for the lane-per-pixel forms (8-channel features, logits) the rows and the loss are bit for bit those of RCV_OP_CE_FWD on those
    logits.  RCV_OP_CE_FWD reads a label through an int: it is given the labels with every value outside [0, C) replaced by -100,
    which the int64 rule of the validation tail treats alike (weight 0, no bin).
The fold against tests/valid_restatement.py, all 76 doubles bit for bit; whole networks against ``Trainer.evaluate`` plus the
restatement."""
import numpy as np
import pytest
import torch

import segment_restatement as S
import small_ops_cases as K
import small_ops_restatement as R
import valid_restatement as V
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D
from robocupvision_amd import model as M
from robocupvision_amd.engine import CLS3_PAD
from robocupvision_amd.metrics import ValidationState
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = (1, 10, 30, 10, 2)


def _h():
    return L.handle(0)


def _cus():
    return int(L.load().rcv_num_cus(_h()))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _run(*ops):
    L.OpList(list(ops)).run(_h(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


def _ws(op):
    nbytes = L.op_workspace(_h(), op)
    t = torch.full(((nbytes + 3) // 4,), float("nan"), device=DEV)
    op.p[L.RCV_P_PART] = t.data_ptr()
    return t


def _source_kw(d, keep, shape, cin, cout, fused, form):
    N, H, W = shape
    kw = dict(n=N, h=H, w=W, cin=cin, cout=cout, p_in=keep["t"].data_ptr(), p_bias=keep["bias"].data_ptr())
    if form == 0:
        kw["p_w"] = keep["w"].data_ptr()
    if fused:
        kw.update(aux0=d["mode2"], aux1=d["r"].shape[1], p_in_c=keep["tc"].data_ptr(), p_x3=keep["r"].data_ptr(), p_x4=keep["rc"].data_ptr())
    return kw


def _labels(shape, cout, seed):
    N, H, W = shape
    return K.build_confusion(N, H, W, cout, seed)[1], np.random.default_rng(seed).uniform(0.5, 6.0, cout).astype(np.float32)


def _drawn(draw, logits64, shape, cout, seed):
    """Operands for which fp32 CAN meet the 1e-5 relative bar.  A pixel's nll is (mx - vt) + logf(se), se a sum of up to C terms in
    class order; once the term exp(0) = 1 is in the sum every further addition rounds at ulp(1): |error| <= (C + 1) 2^-24 absolute,
    whatever the size of the nll.  RCV_OP_CE_FWD itself is therefore 1e-5 relative to float64 only where the loss is at least
    (C + 1) 2^-24 / 1e-5 (0.054 for 8 classes).  The mean over many pixels under labels drawn independently of the logits is O(1);
    a plane of one or a few pixels can fall under that floor (one confidently right pixel: 0.007), so the operands are drawn again
    until the FLOAT64 loss of the draw -- the restatement alone decides, before anything runs on the device -- is twice above it."""
    N, H, W = shape
    tgt, cw = _labels(shape, cout, seed)
    floor = 2 * (cout + 1) * 2.0 ** -24 / 1e-5
    for _ in range(200):
        d = draw()
        ref = R.cross_entropy(logits64(d).reshape(N, H, W, cout).transpose(0, 3, 1, 2), tgt, cw)
        if cout == 1 or not ref["sum_w"] > 0 or ref["loss"] >= floor:
            return d
    raise AssertionError("no draw with a float64 loss above %.3g for %s, %d classes" % (floor, shape, cout))


def _check_record(d, shape, cin, cout, fused, form, seed):
    """One case through RCV_OP_CLS_LABEL, the logits-writing record, RCV_OP_CE_FWD and twice through RCV_OP_CLS_VALID."""
    N, H, W = shape
    flags = L.F_FUSED_UP if fused else 0
    keep = {k: _dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    tgt, cw = _labels(shape, cout, seed)
    tgt_d, cw_d = _dev(tgt), _dev(cw)
    src = _source_kw(d, keep, shape, cin, cout, fused, form)
    # the references on the same operands: the class map, the logits, the loss of RCV_OP_CE_FWD
    lab_ref = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    logits = torch.full((N, cout, H, W), float("nan"), device=DEV)
    _run(L.make_op(L.OP_CLS_LABEL, flags, inmode=form, p_out=lab_ref.data_ptr(), **src),
         L.make_op(L.OP_CLS_FWD, flags, p_out=logits.data_ptr(), **src) if form == 0 else
         L.make_op(L.OP_NHWC_TO_NCHW, 0, p_out=logits.data_ptr(), **src))
    in_range = (tgt >= 0) & (tgt < cout)
    tgt_ce = _dev(np.where(in_range, tgt, -100))
    loss_ce = torch.full((4,), float("nan"), device=DEV)
    ce = L.make_op(L.OP_CE_FWD, 0, n=N, h=H, w=W, cout=cout, p_in=logits.data_ptr(), p_in2=tgt_ce.data_ptr(), p_w=cw_d.data_ptr(), p_out=loss_ce.data_ptr())
    ce_rows = _ws(ce)
    _run(ce)
    # the record under test, twice into one counts buffer; then the fold finalises the rows
    lab = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(N, cout, cout, dtype=torch.int32, device=DEV)
    op = L.make_op(L.OP_CLS_VALID, flags, inmode=form, p_in2=tgt_d.data_ptr(), p_x0=cw_d.data_ptr(), p_x2=counts.data_ptr(), p_out=lab.data_ptr(), **src)
    rows = _ws(op)
    g = op.i[L.RCV_I_NPART]
    _run(op)
    what = "%s cin %d cout %d fused %d form %d" % (shape, cin, cout, fused, form)
    assert torch.equal(lab, lab_ref), what
    want = R.confusion(lab_ref.cpu().numpy(), tgt, cout)
    first = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(first, want), what
    assert int(want.sum()) == int((in_range & (lab_ref.cpu().numpy() < cout)).sum()) and (cout == 1 or int(want.sum()) < N * H * W or N * H * W < 20)
    op.p[L.RCV_P_OUT] = None          # no class map asked for: nothing is written there
    lab.fill_(0xAB)
    _run(op)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), 2 * want), what
    assert bool((lab == 0xAB).all())
    got_rows = rows[:3 * g].cpu().numpy().reshape(g, 3)
    assert not np.isnan(got_rows).any(), "a partial row was not written"
    state = torch.zeros(L.VALID_STATE, dtype=torch.float64, device=DEV)
    _run(L.make_op(L.OP_VALID_FOLD, 0, n=N, h=H, w=W, cout=cout, npart=g, p_in=counts.data_ptr(), p_in2=rows.data_ptr(), p_out=state.data_ptr()))
    loss = float(state[0])
    ref = R.cross_entropy(logits.cpu().numpy(), tgt, cw)
    print("%s: loss %.9g, float64 %.9g, RCV_OP_CE_FWD %.9g" % (what, loss, ref["loss"], float(loss_ce[0])))
    if ref["sum_w"] > 0:
        assert abs(loss - ref["loss"]) <= 1e-5 * abs(ref["loss"]), what
        assert abs(got_rows[:, 1].astype(np.float64).sum() - ref["sum_w"]) <= 1e-5 * ref["sum_w"]
    assert int(got_rows[:, 2].sum()) == ref["correct"] == int(np.trace(want.sum(0)))
    assert not bool(counts.any()) and float(state[2]) == N and float(state[3]) == N * H * W
    if not (form == 0 and cin == 16):          # a lane per pixel: RCV_OP_CE_FWD's grid, mapping and order
        assert g == ce.i[L.RCV_I_NPART]
        assert np.array_equal(got_rows.view(np.uint32), ce_rows[:3 * g].cpu().numpy().reshape(g, 3).view(np.uint32)), what
        assert np.float32(loss).view(np.uint32) == loss_ce[:1].cpu().numpy().view(np.uint32)[0] or (np.isnan(loss) and ref["sum_w"] == 0), what


SMALL_PLANES = [(1, 1, 1), (3, 5, 7), (2, 17, 31), (300, 1, 1)]
CONFIGS = [("c8", 8, False, S.PLAIN, None), ("c8_up_plain", 8, True, S.PLAIN, 8), ("c8_up_affine_relu", 8, True, S.AFFINE_RELU, 8),
           ("c8_up_skip4", 8, True, S.AFFINE, 4), ("c16", 16, False, S.PLAIN, None), ("c16_up_skip8", 16, True, S.AFFINE_RELU, 8),
           ("c16_up_skip16", 16, True, S.AFFINE, 16)]


@pytest.mark.parametrize("tag,cin,fused,mode2,rch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_record_from_features(tag, cin, fused, mode2, rch):
    rng = np.random.default_rng(4100 + cin + 3 * fused)
    big = K.big_planes(_cus())["reducing"][1 if cin == 16 else 0]          # beyond the grid cap: the odd plane for four lanes per pixel
    assert big[0] * big[1] * big[2] > 256 * 4 * _cus()
    for cout in (1, 2, 5, 8):
        for k, shape in enumerate(SMALL_PLANES + [big]):
            d = _drawn(lambda: S.random_case(rng, shape, cin, cout, fused, mode2, rch), lambda d: S.case_logits(d)[1], shape, cout, 10 * cout + k)
            _check_record(d, shape, cin, cout, fused, 0, 10 * cout + k)


def test_record_from_padded_logits():
    rng = np.random.default_rng(4200)
    big = K.big_planes(_cus())["reducing"][1]
    for cout in (1, 2, 5, 8):
        for k, shape in enumerate(SMALL_PLANES + [big]):
            def draw():
                z = (2 * rng.standard_normal((int(np.prod(shape)), CLS3_PAD))).astype(np.float32)
                z[:, cout:] = 100.0          # the padding is not a logit
                return dict(t=z, bias=(0.1 * rng.standard_normal(cout)).astype(np.float32))
            d = _drawn(draw, lambda d: S.logits_padded(d["t"], cout, d["bias"]), shape, cout, 10 * cout + k)
            _check_record(d, shape, CLS3_PAD, cout, False, 1, 10 * cout + k)


def test_record_from_a_class_map_counts_only():
    for cout in (1, 2, 5, 8):
        for k, (N, H, W) in enumerate(SMALL_PLANES + [K.big_planes(_cus())["reducing"][0]]):
            pred, tgt = K.build_confusion(N, H, W, cout, 50 + k)
            pred_d, tgt_d = _dev(pred), _dev(tgt)
            counts = torch.zeros(N, cout, cout, dtype=torch.int32, device=DEV)
            op = L.make_op(L.OP_CLS_VALID, 0, n=N, h=H, w=W, cin=1, cout=cout, inmode=L.CLS_LABEL_CLASSMAP, p_in=pred_d.data_ptr(),
                           p_in2=tgt_d.data_ptr(), p_x2=counts.data_ptr())
            assert L.op_workspace(_h(), op) == 0
            _run(op)
            _run(op)
            assert np.array_equal(counts.cpu().numpy().astype(np.int64), 2 * R.confusion(pred, tgt, cout)), (cout, N, H, W)


def test_null_operands_are_refused_at_enqueue():
    x, w = torch.zeros(494, 8, device=DEV), torch.zeros(5, 8, device=DEV)
    t = torch.zeros(494, dtype=torch.int64, device=DEV)
    c = torch.zeros(2, 5, 5, dtype=torch.int32, device=DEV)
    base = dict(n=2, h=13, w=19, cin=8, cout=5)
    full = dict(p_in=x.data_ptr(), p_w=w.data_ptr(), p_in2=t.data_ptr(), p_x2=c.data_ptr())
    for drop, msg in (("p_in", "null input, targets"), ("p_in2", "null input, targets"), ("p_x2", "null input, targets"), ("p_w", "null classifier weight")):
        op = L.make_op(L.OP_CLS_VALID, 0, **base, **{k: v for k, v in full.items() if k != drop})
        ws = _ws(op)
        with pytest.raises(L.RcvError, match=msg):
            _run(op)
        del ws
    with pytest.raises(L.RcvError, match="null partial rows"):
        _run(L.make_op(L.OP_CLS_VALID, 0, **base, **full))
    op = L.make_op(L.OP_CLS_VALID, 0, **base, **full)
    ws = _ws(op)
    op.i[L.RCV_I_NPART] += 1
    with pytest.raises(L.RcvError, match="workspace rows"):
        _run(op)
    with pytest.raises(L.RcvError, match="null counts"):
        _run(L.make_op(L.OP_VALID_FOLD, 0, n=2, h=13, w=19, cout=5, npart=0, p_x0=x.data_ptr()))


# ------------------------------------------------------------------------------------------ the fold
def test_fold_three_batches_bit_for_bit():
    """Three batches of different N into one state, once with the loss as partial rows and once as a device scalar.  The rows are
    small integers: their float64 sums are exact in any order, so the fp32 loss is fp32(sum0 / sum1) whatever the order."""
    C = 5
    rng = np.random.default_rng(77)
    by_rows = torch.zeros(L.VALID_STATE, dtype=torch.float64, device=DEV)
    by_scalar = torch.zeros(L.VALID_STATE, dtype=torch.float64, device=DEV)
    want = V.new_state()
    for k, (N, H, W) in enumerate([(3, 5, 7), (70, 3, 2), (1, 17, 31)]):          # 70 images: more than one round of 256 / C per class
        pred, tgt = K.build_confusion(N, H, W, C, 60 + k)
        pred = np.minimum(pred, C - 1)
        if k == 0:          # class 3 in neither mask of image 1: union 0 -> 1
            pred[1][pred[1] == 3] = 0
            tgt[1][tgt[1] == 3] = 0
        g = 5 + 300 * k
        rows = np.stack([rng.integers(1, 50, g), rng.integers(1, 9, g), rng.integers(0, 9, g)], 1).astype(np.float32)
        loss32 = np.float32(rows[:, 0].astype(np.float64).sum() / rows[:, 1].astype(np.float64).sum())
        cnt = V.counts(pred, tgt, C)
        assert np.array_equal(cnt, R.confusion(pred, tgt, C))
        want = V.fold(want, cnt, loss32, H, W)
        pred_d, tgt_d, rows_d, loss_d = _dev(pred), _dev(tgt), _dev(rows), _dev(np.array([loss32]))
        counts = torch.zeros(N, C, C, dtype=torch.int32, device=DEV)
        count_op = L.make_op(L.OP_CLS_VALID, 0, n=N, h=H, w=W, cin=1, cout=C, inmode=L.CLS_LABEL_CLASSMAP, p_in=pred_d.data_ptr(),
                             p_in2=tgt_d.data_ptr(), p_x2=counts.data_ptr())
        dims = dict(n=N, h=H, w=W, cout=C, p_in=counts.data_ptr())
        _run(count_op, L.make_op(L.OP_VALID_FOLD, 0, npart=g, p_in2=rows_d.data_ptr(), p_out=by_rows.data_ptr(), **dims))
        assert not bool(counts.any()), "the fold clears the counts it read"
        _run(count_op, L.make_op(L.OP_VALID_FOLD, 0, npart=0, p_x0=loss_d.data_ptr(), p_out=by_scalar.data_ptr(), **dims))
        assert not bool(counts.any())
    for name, got in (("rows", by_rows), ("scalar", by_scalar)):
        got = got.cpu().numpy()
        differ = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert differ.size == 0, (name, differ.tolist(), got[differ].tolist(), want[differ].tolist())
    assert want[1] == 3 and want[2] == 74 and want[3] == 3 * 35 + 70 * 6 + 527


# ------------------------------------------------------------------------------------------ whole networks
def _build(make, seed=5):
    torch.manual_seed(seed)
    net = make()
    for m in net.modules():          # running statistics a validation pass would meet, not the initial (0, 1)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net.to(DEV).eval()


def _targets(shape, C, seed):
    """int64 labels with -100 and C among them (maskLabel, ignore_index)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, shape, generator=g)
    t.view(-1)[::41] = -100
    t.view(-1)[5::53] = C
    return t.to(DEV)


def _loop(trainer, batches, C):
    """The per-batch loop this pass replaces: Trainer.evaluate, torch.max, float(loss), then the restatement."""
    out = []
    for x, t in batches:
        pred, loss, _ = trainer.evaluate(x, t)
        out.append((torch.max(pred, 1)[1].cpu().numpy(), t.cpu().numpy(), np.float32(float(loss))))
    return V.valid_pass(out, C)


def _same_state(state, want, loss_bits=True):
    got = state.buf.cpu().numpy()
    lo = 0 if loss_bits else 1
    differ = np.nonzero(got[lo:].view(np.uint64) != want[lo:].view(np.uint64))[0] + lo
    assert differ.size == 0, (differ.tolist(), got[differ].tolist(), want[differ].tolist())
    if not loss_bits:
        assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]), (got[0], want[0])


NETS = [
    ("robo", lambda: M.ROBO_UNet(), (2, 3, 48, 64), WEIGHTS),
    ("v2_cls3x3", lambda: M.ROBO_UNet(v2=True, classSize=3), (2, 3, 48, 64), WEIGHTS),
    ("cls5x5", lambda: M.ROBO_UNet(classSize=5), (2, 3, 48, 64), WEIGHTS),
    ("pb_fcn_k5", lambda: M.PB_FCN(32, 5, 5, False, 0), (2, 3, 48, 64), WEIGHTS),
    ("labelprop", lambda: M.LabelProp(5, 32, 0), (2, 8, 24, 32), (1, 6, 1, 3, 2)),          # labelPropTrain.py:94
]


@pytest.mark.parametrize("tag,make,shape,weights", NETS, ids=[n[0] for n in NETS])
def test_network_validate_equals_the_loop(tag, make, shape, weights):
    net = _build(make)
    # (AdamL1's parameter groups are the U-Net's: PB_FCN and LabelProp train under SGD, trainer.py:176-178)
    tr = Trainer(net, class_weights=weights, optimizer=None if isinstance(net, M.ROBO_UNet) else SGD(net, lr=1e-2, momentum=0.5, weight_decay=1e-3))
    torch.manual_seed(31)
    batches = [(torch.randn(*shape, device=DEV), _targets((shape[0],) + shape[2:], 5, 32 + k)) for k in range(2)]
    want, rep = _loop(tr, batches, 5)
    state = ValidationState(5, DEV)
    w = torch.tensor(weights, dtype=torch.float32, device=DEV)
    for x, t in batches:
        lab = net.validate(x, t, state, weight=w, labels=True)
        assert lab.dtype == torch.uint8 and torch.equal(lab, torch.max(net(x), 1)[1].to(torch.uint8)) and torch.equal(lab, net.predict(x))
    assert net.validate(batches[0][0], batches[0][1], ValidationState(5, DEV), weight=w) is None
    _same_state(state, want, loss_bits=tag != "labelprop")
    got = state.compute()
    print("%s: %s" % (tag, {k: got[k] for k in ("loss", "pixel_acc", "mean_class_acc", "mean_iou", "score")}))
    for k in ("pixel_acc", "mean_class_acc", "mean_iou", "score", "images", "batches"):
        assert got[k] == rep[k], (k, got[k], rep[k])
    assert np.array_equal(got["confusion"].numpy(), rep["confusion"]) and got["images"] == 2 * shape[0]
    assert sum(1 for (_, k) in net._get_engine().plans if k == "") == 1          # one eval-valid plan, in the one cache
    state.reset()
    assert not bool(state.buf.any())


@pytest.mark.parametrize("nC", range(1, 9))
def test_every_class_count(nC):
    net = _build(lambda: M.ROBO_UNet(nClass=nC))
    tr = Trainer(net, class_weights=[1.0 + c for c in range(nC)])
    torch.manual_seed(40 + nC)
    batches = [(torch.randn(1, 3, 16, 16, device=DEV), _targets((1, 16, 16), nC, 50 + nC))]
    want, _ = _loop(tr, batches, nC)
    state = ValidationState(nC, DEV)
    net.validate(batches[0][0], batches[0][1], state, weight=tr.criterion.weight)
    _same_state(state, want)


def _store(n=5, size=(48, 64)):
    rng = np.random.default_rng(8)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8))
    labels = torch.from_numpy(rng.integers(0, 5, (n,) + size, dtype=np.uint8))
    return D.ResidentDataset.from_tensors(frames, labels, size, device=DEV)


@pytest.mark.parametrize("dice", [False, True], ids=["cross_entropy", "dice"])
def test_trainer_validate_over_an_epoch_loader(dice):
    """5 images in batches of 2: the last batch is short (another plan, another counts buffer)."""
    net = _build(lambda: M.ROBO_UNet())
    tr = Trainer(net, class_weights=WEIGHTS, use_dice=dice, decay=1e-6)
    loader = D.EpochLoader(_store(), 2, train=False, shuffle=False)
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    want, rep = _loop(tr, batches, 5)
    state = ValidationState(5, DEV)
    got = tr.validate(loader, state)
    _same_state(state, want)
    reg = float(tr.optimizer.l1_term())
    assert got["reg"] == reg and got["loss"] == rep["loss"] + reg and got["pruned"] == M.count_zero_weights(net)
    for k in ("pixel_acc", "mean_class_acc", "mean_iou", "score", "images", "batches"):
        assert got[k] == rep[k] or (np.isnan(got[k]) and np.isnan(rep[k])), (k, got[k], rep[k])
    assert got["images"] == 5 and got["batches"] == 3
    # a fresh state by default; with prune indices the regulariser stays out of the loss
    again = tr.validate(loader)
    assert again["loss"] == got["loss"] and again["images"] == 5
    tr.prune_indices = []
    assert tr.validate(loader)["loss"] == rep["loss"]


def test_validate_sees_the_weights_of_a_trainer_step():
    net = _build(lambda: M.ROBO_UNet())
    tr = Trainer(net, class_weights=WEIGHTS, lr=1e-2, decay=1e-6)
    torch.manual_seed(23)
    x, t = torch.randn(2, 3, 48, 64, device=DEV), _targets((2, 48, 64), 5, 24)
    before = ValidationState(5, DEV)
    first = net.validate(x, t, before, weight=tr.criterion.weight, labels=True).clone()
    tr.step(x, t)
    net.eval()
    want, _ = _loop(tr, [(x, t)], 5)
    after = ValidationState(5, DEV)
    second = net.validate(x, t, after, weight=tr.criterion.weight, labels=True)
    _same_state(after, want)
    assert bool((second != first).any()) and float(after.buf[0]) != float(before.buf[0])


def test_validate_refusals_on_the_device():
    net = _build(lambda: M.ROBO_UNet())
    x, t = torch.randn(1, 3, 16, 16, device=DEV), torch.zeros(1, 16, 16, dtype=torch.int64, device=DEV)
    with pytest.raises(L.RcvError, match="counts 3 classes"):
        net.validate(x, t, ValidationState(3, DEV))
    with pytest.raises(L.RcvError, match="targets must be"):
        net.validate(x, t[:, :8], ValidationState(5, DEV))
    with pytest.raises(L.RcvError, match="class weights"):
        net.validate(x, t, ValidationState(5, DEV), weight=torch.ones(4, device=DEV))
    s = ValidationState(5, DEV)
    with pytest.raises(L.RcvError, match="uint8"):
        s.update_from_map(t, t, torch.zeros(1, device=DEV))
    with pytest.raises(L.RcvError, match="one-element tensor"):
        s.update_from_map(t.to(torch.uint8), t, 0.5)
    assert not bool(s.buf.any())
