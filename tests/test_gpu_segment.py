"""GPU: class maps and colour masks on the device (RCV_OP_CLS_LABEL, RCV_OP_FRAME_PREP, ``predict``, ``Segmenter``).

Kernel level, one record at a time through rcv_run against the float64 restatement (tests/segment_restatement.py):
  * integer-grid operands, every logit exact in fp32, many exact ties: class map and colour image equal the restatement EVERYWHERE
    (the first index wins), in both store shapes, on 2x13x19 = 494 pixels (no multiple of 4, 64 or 256);
  * random operands: every pixel whose float64 top-2 margin exceeds 2 (CIN + 3) 2^-24 max_c(sum_k |v_k| |W_ck| + |b_c|) -- the fp32
    dot-product bound, derived in segment_restatement.margin_bound -- must match exactly, and at most 1 pixel in 10 000 may fall under
    it; 1x480x640 is more pixels than one sweep of the 1024 x 256-thread grid (the grid-stride loop and its tail);
  * NaN logits, classes outside the palette, the class-map source form.
Network level: ``predict`` against the golden-pinned eval path of the same model object, ``torch.max(model(x), 1)[1]``, exactly equal;
stale plans; ``Segmenter`` against the composition of the existing pieces; the metrics take the map unchanged."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import batch_prep_restatement as BR
import segment_restatement as R
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D
from robocupvision_amd import model as M
from robocupvision_amd import palette as P
from robocupvision_amd.engine import CLS3_PAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAL = np.array([[3, 1, 4], [1, 5, 9], [2, 6, 5], [35, 89, 79], [32, 38, 46], [26, 43, 38], [32, 79, 50], [28, 84, 197]], np.uint8)


def _h():
    return L.handle(0)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _run(op):
    L.OpList([op]).run(_h(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


def _label_op(d, shape, cin, cout, fused, store, colour=True, form=0):
    """Runs one RCV_OP_CLS_LABEL record on the operands of a case dict; outputs prefilled with 0xAB so that an unwritten byte shows."""
    N, H, W = shape
    keep = {k: _dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    lab = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    col = torch.full((N, H, W, 3), 0xAB, dtype=torch.uint8, device=DEV)
    pal = _dev(PAL)
    kw = dict(n=N, h=H, w=W, cin=cin, cout=cout, inmode=form, count=store, p_in=keep["t"].data_ptr(), p_bias=keep["bias"].data_ptr(),
              p_out=lab.data_ptr(), p_x0=col.data_ptr() if colour else 0, p_x1=pal.data_ptr() if colour else 0)
    if form == 0:
        kw["p_w"] = keep["w"].data_ptr()
    if fused:
        kw.update(aux0=d["mode2"], aux1=d["r"].shape[1], p_in_c=keep["tc"].data_ptr(), p_x3=keep["r"].data_ptr(), p_x4=keep["rc"].data_ptr())
    _run(L.make_op(L.OP_CLS_LABEL, L.F_FUSED_UP if fused else 0, **kw))
    return lab.cpu().numpy(), col.cpu().numpy()


CONFIGS = [("c8", 8, False, R.PLAIN, None), ("c8_up_plain", 8, True, R.PLAIN, 8), ("c8_up_affine", 8, True, R.AFFINE, 8),
           ("c8_up_affine_relu", 8, True, R.AFFINE_RELU, 8), ("c8_up_skip4", 8, True, R.AFFINE, 4), ("c16", 16, False, R.PLAIN, None),
           ("c16_up_skip4", 16, True, R.AFFINE, 4), ("c16_up_skip8", 16, True, R.AFFINE_RELU, 8), ("c16_up_skip16", 16, True, R.PLAIN, 16)]


# ------------------------------------------------------------------------------------------ 1. exact ties and order
@pytest.mark.parametrize("tag,cin,fused,mode2,rch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_exact_ties_first_index_wins(tag, cin, fused, mode2, rch):
    rng = np.random.default_rng(101)
    shape = (2, 13, 19)
    for cout in (1, 2, 5, 8):
        d = R.exact_case(rng, shape, cin, cout, fused, mode2, rch)
        v, lg = R.case_logits(d)
        want = R.first_argmax(lg).reshape(shape)
        ties = int((R.top2_margin(lg) == 0).sum())
        print("%s cout %d: %d of %d pixels tie exactly, classes seen %s" % (tag, cout, ties, want.size, sorted(set(want.ravel().tolist()))))
        assert cout < 3 or ties >= 20
        for store in (1, 4, 0):
            lab, col = _label_op(d, shape, cin, cout, fused, store)
            assert np.array_equal(lab, want), (cout, store, int((lab != want).sum()))
            assert np.array_equal(col, R.colour_image(want, PAL)), (cout, store)
            if cout == 1:
                assert not lab.any()
        lab, col = _label_op(d, shape, cin, cout, fused, 4, colour=False)
        assert np.array_equal(lab, want) and bool((col == 0xAB).all())          # no colour pointer: nothing is written there


def test_exact_ties_logits_form():
    rng = np.random.default_rng(102)
    shape = (2, 13, 19)
    for cout in (1, 2, 5, 8):
        z = rng.integers(-3, 4, (494, CLS3_PAD)).astype(np.float32)
        z[:, cout:] = 100.0          # the padding is not a logit
        d = dict(t=z, bias=rng.integers(-2, 3, cout).astype(np.float32))
        want = R.first_argmax(R.logits_padded(z, cout, d["bias"])).reshape(shape)
        assert cout == 1 or int((R.top2_margin(R.logits_padded(z, cout, d["bias"])) == 0).sum()) >= 20
        for store in (1, 4):
            lab, col = _label_op(d, shape, CLS3_PAD, cout, False, store, form=1)
            assert np.array_equal(lab, want) and np.array_equal(col, R.colour_image(want, PAL)), (cout, store)


# ------------------------------------------------------------------------------------------ 2. random data
@pytest.mark.parametrize("shape", [(2, 13, 19), (3, 40, 24), (1, 480, 640)], ids=lambda s: "x".join(map(str, s)))
def test_random_data_outside_the_fp32_margin(shape):
    rng = np.random.default_rng(1234)
    total = int(np.prod(shape))
    assert shape != (1, 480, 640) or total > 1024 * 256
    for (cin, cout, fused, mode2, rch) in ((8, 5, True, R.AFFINE, 8), (8, 2, False, R.PLAIN, None), (16, 5, True, R.AFFINE_RELU, 8),
                                           (16, 8, True, R.AFFINE, 16), (8, 3, True, R.AFFINE_RELU, 4)):
        d = R.random_case(rng, shape, cin, cout, fused, mode2, rch)
        v, lg = R.case_logits(d)
        want = R.first_argmax(lg).reshape(shape)
        out = (R.top2_margin(lg) <= R.margin_bound(v, d["w"], d["bias"], cin)).reshape(shape)
        for store in (1, 4):
            lab, col = _label_op(d, shape, cin, cout, fused, store)
            differ = lab != want
            print("%s cin %d cout %d store %d: %d of %d pixels under the fp32 margin, %d differ" % (shape, cin, cout, store, int(out.sum()), total,
                                                                                                 int(differ.sum())))
            assert int(out.sum()) * 10000 <= total, (int(out.sum()), total)
            assert not (differ & ~out).any(), int((differ & ~out).sum())
            assert np.array_equal(col, R.colour_image(lab, PAL))          # colour = palette[the class the kernel took], everywhere
    # the logits form: one fp32 addition per logit
    z = rng.standard_normal((total, CLS3_PAD)).astype(np.float32)
    d = dict(t=z, bias=(0.1 * rng.standard_normal(5)).astype(np.float32))
    lg = R.logits_padded(z, 5, d["bias"])
    out = (R.top2_margin(lg) <= R.margin_bound(z[:, :5], np.eye(5), d["bias"], CLS3_PAD)).reshape(shape)
    lab, col = _label_op(d, shape, CLS3_PAD, 5, False, 0, form=1)
    assert int(out.sum()) * 10000 <= total and not ((lab != R.first_argmax(lg).reshape(shape)) & ~out).any()
    assert np.array_equal(col, R.colour_image(lab, PAL))


# ------------------------------------------------------------------------------------------ 3. NaN and bad classes
def test_nan_never_wins_and_bad_classes_are_black():
    rng = np.random.default_rng(103)
    shape = (2, 13, 19)
    z = rng.integers(-3, 4, (494, CLS3_PAD)).astype(np.float32)
    nan = rng.random((494, CLS3_PAD)) < 0.3
    nan[:40] = True          # all-NaN pixels
    nan[40:80, 0] = True
    z[nan] = np.nan
    d = dict(t=z, bias=np.zeros(5, np.float32))
    want = R.first_argmax(z[:, :5]).reshape(shape)
    assert not want.ravel()[:40].any() and int(np.isnan(z[:, :5]).all(1).sum()) >= 40
    for store in (1, 4):
        lab, col = _label_op(d, shape, CLS3_PAD, 5, False, store, form=1)
        assert np.array_equal(lab, want) and np.array_equal(col, R.colour_image(want, PAL))
        assert not np.isnan(z[np.arange(494), lab.ravel()])[~np.isnan(z[:, :5]).all(1)].any()          # a NaN never won
    # features with a NaN: every logit of the pixel is NaN -> class 0
    dd = R.exact_case(rng, shape, 8, 5, False)
    dd["t"][::7, 3] = np.nan
    lab, _ = _label_op(dd, shape, 8, 5, False, 0)
    want = R.first_argmax(R.case_logits(dd)[1]).reshape(shape)
    assert np.array_equal(lab, want) and not lab.ravel()[::7].any()

    # source form 2: class maps with values beyond the palette
    cm = rng.integers(0, 12, shape).astype(np.uint8)
    cm[0, 0, :4] = (255, 8, 7, 0)
    for t in (_dev(cm), _dev(cm.astype(np.int64) - (cm == 11) * 20)):          # int64: negative classes too
        ref = R.colour_image(t.cpu().numpy(), PAL)
        got = P.colorize(t, _dev(PAL))
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,) and np.array_equal(got.cpu().numpy(), ref)
        for store in (1, 4):
            col = torch.full(shape + (3,), 0xAB, dtype=torch.uint8, device=DEV)
            pal = _dev(PAL)
            _run(L.make_op(L.OP_CLS_LABEL, 0, n=2, h=13, w=19, cin=1, cout=8, inmode=2, inmode2=t.element_size(), count=store, p_in=t.data_ptr(),
                           p_x0=col.data_ptr(), p_x1=pal.data_ptr()))
            assert np.array_equal(col.cpu().numpy(), ref)
    # ... on a map of test 1 it equals that test's colour output; the default palette; Colorize's layout
    d1 = R.exact_case(np.random.default_rng(101), shape, 8, 5, False)
    lab, col = _label_op(d1, shape, 8, 5, False, 0)
    assert np.array_equal(P.colorize(_dev(lab), PAL).cpu().numpy(), col)
    assert np.array_equal(robocupvision_amd.colorize(_dev(lab)).cpu().numpy(), R.colour_image(lab, R.PALETTE5))
    one = robocupvision_amd.Colorize()(_dev(cm[0]))
    assert one.device.type == "cuda" and tuple(one.shape) == (3, 13, 19) and np.array_equal(one.cpu().numpy(), R.colorize_five_masks(cm[0], 5))
    assert np.array_equal(robocupvision_amd.Colorize(3)(_dev(cm[1])[None]).cpu().numpy(), R.colorize_five_masks(cm[1], 3))
    assert tuple(P.colorize(_dev(cm[0])).shape) == (13, 19, 3)


def test_null_operands_are_refused_at_enqueue():
    x = torch.zeros(494, 8, device=DEV)
    w = torch.zeros(5, 8, device=DEV)
    lab = torch.zeros(494, dtype=torch.uint8, device=DEV)
    base = dict(n=2, h=13, w=19, cin=8, cout=5)
    for kw, msg in ((dict(p_w=w.data_ptr(), p_out=lab.data_ptr()), "null input"), (dict(p_in=x.data_ptr(), p_out=lab.data_ptr()), "null classifier weight"),
                    (dict(p_in=x.data_ptr(), p_w=w.data_ptr()), "null output"),
                    (dict(p_in=x.data_ptr(), p_w=w.data_ptr(), p_out=lab.data_ptr(), p_x0=lab.data_ptr()), "needs the palette")):
        with pytest.raises(L.RcvError, match=msg):
            _run(L.make_op(L.OP_CLS_LABEL, 0, **base, **kw))
    with pytest.raises(L.RcvError, match="operands missing"):
        _run(L.make_op(L.OP_CLS_LABEL, L.F_FUSED_UP, p_in=x.data_ptr(), p_w=w.data_ptr(), p_out=lab.data_ptr(), **base))
    with pytest.raises(L.RcvError, match="colour image: null output"):
        _run(L.make_op(L.OP_CLS_LABEL, 0, n=2, h=13, w=19, cin=1, cout=8, inmode=2, inmode2=1, p_in=lab.data_ptr()))
    with pytest.raises(L.RcvError, match="frame prep: null operand"):
        fx = torch.zeros(64, dtype=torch.int32, device=DEV)
        _run(L.make_op(L.OP_FRAME_PREP, n=1, h=8, w=8, ho=8, wo=8, cin=3, cout=3, p_x1=fx.data_ptr(), p_x2=fx.data_ptr(), p_x5=fx.data_ptr()))


# ------------------------------------------------------------------------------------------ 4. frames only
def _frames(B, Hs, Ws, seed):
    return BR.synthetic_frames(B, Hs, Ws, seed)[0]


assert ((97, 131), (40, 33)) in BR.SHAPE_PAIRS


@pytest.mark.parametrize("src,size", [((24, 32), (12, 16)), ((48, 64), (48, 64)), ((97, 131), (40, 33))])
def test_prepare_frames_equals_prepare_batch(src, size):
    frames = _dev(_frames(3, src[0], src[1], 5))
    zero = torch.zeros(3, src[0], src[1], dtype=torch.uint8, device=DEV)
    for ft in (False, True):
        got = D.prepare_frames(frames, size, finetune=ft)
        want = D.prepare_batch(frames, zero, size, finetune=ft, train=False)[0]
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3) + tuple(size)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_prepare_frames_equals_the_goldens():
    with open(os.path.join(GOLDEN, "batch_prep.json")) as f:
        meta = json.load(f)
    kats = np.load(os.path.join(GOLDEN, "batch_prep.npz"))
    assert meta["configs"]
    for tag, c in sorted(meta["configs"].items()):
        size = tuple(c["size"])
        frames, _ = BR.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"], cover_size=size)
        got = D.prepare_frames(_dev(frames), size, finetune=c["finetune"]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(kats[tag + "/val_imgs"], np.float32).view(np.uint32)), tag


# ------------------------------------------------------------------------------------------ network level
def _build(make, seed=5):
    torch.manual_seed(seed)
    net = make()
    for m in net.modules():          # running statistics a validation pass would meet, not the initial (0, 1)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net.to(DEV).eval()


def _check_predict(net, x, palette=None):
    want = torch.max(net(x), 1)[1].to(torch.uint8)
    lab = net.predict(x)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (x.shape[0],) + tuple(x.shape[2:]) and lab.is_contiguous()
    assert torch.equal(lab, want), int((lab != want).sum())
    lab2, col = net.predict(x, colour=True, palette=palette)
    pal = P.device_palette(palette, DEV)
    assert torch.equal(lab2, want) and lab2.data_ptr() != lab.data_ptr()          # a fresh tensor per call
    assert col.dtype == torch.uint8 and tuple(col.shape) == tuple(lab.shape) + (3,) and torch.equal(col, pal[lab2.long()])
    assert torch.equal(net.predict(x), want)          # the cached plan, behind its head
    return want


NETS = [
    ("robo", lambda: M.ROBO_UNet(), (2, 3, 48, 64)),
    ("robo_c1", lambda: M.ROBO_UNet(nClass=1), (1, 3, 48, 64)),
    ("robo_c3", lambda: M.ROBO_UNet(nClass=3), (1, 3, 48, 64)),
    ("robo_c8", lambda: M.ROBO_UNet(nClass=8), (1, 3, 48, 64)),
    ("v2_cls3x3", lambda: M.ROBO_UNet(v2=True, classSize=3, levels=1, bellySize=9), (1, 3, 48, 64)),
    ("unet", lambda: M.ROBO_UNet(pool=True, levels=3, bellySize=0), (1, 3, 48, 64)),
    ("pb_fcn", lambda: M.PB_FCN(32, 5, 1, False, 0), (2, 3, 48, 64)),
    ("pb_fcn_2", lambda: M.PB_FCN_2(False), (2, 3, 48, 64)),
    ("labelprop", lambda: M.LabelProp(5, 32), (2, 8, 24, 32)),
    ("robo_odd_plane", lambda: M.ROBO_UNet(), (3, 3, 40, 56)),
]


@pytest.mark.parametrize("tag,make,shape", NETS, ids=[n[0] for n in NETS])
def test_predict_equals_the_eval_path(tag, make, shape):
    net = _build(make)
    torch.manual_seed(17)
    x = torch.randn(*shape, device=DEV)
    want = _check_predict(net, x, palette=None if tag != "robo_c8" else PAL)
    n_class = net(x).shape[1]
    seen = sorted(set(want.cpu().numpy().ravel().tolist()))
    print("%s: classes seen %s of %d" % (tag, seen, n_class))
    assert n_class == 1 or len(seen) > 1
    if tag == "robo_c1":
        assert not want.any()
    if tag == "labelprop":          # what _engine_inputs accepts: NHWC memory as well
        assert torch.equal(net.predict(x.contiguous(memory_format=torch.channels_last)), want)
    eng = net._get_engine()
    assert sorted(str(k) for (_, k) in eng.plans) == ["False", "None"]          # eval and eval-labels, one cache


def test_predict_refusals_on_the_device():
    net = _build(lambda: M.ROBO_UNet())
    x = torch.randn(1, 3, 48, 64, device=DEV)
    with pytest.raises(L.RcvError, match=r"call `\.eval\(\)` first"):
        net.train().predict(x)
    net.eval()
    with pytest.raises(ValueError):
        net.predict(x, colour=True, palette=torch.zeros(9, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        net.predict(x, colour=True, palette=torch.zeros(5, 3))
    with pytest.raises(ValueError):
        net.predict(x[:, :2])
    with pytest.raises(L.RcvError, match="pool_cls"):
        pb = _build(lambda: M.PB_FCN_2(True))
        pb._get_engine().predict([x], False, None)


@pytest.mark.parametrize("how", ["trainer_step", "data_edit"])
def test_predict_after_the_parameters_changed(how):
    from robocupvision_amd.train import Trainer
    net = _build(lambda: M.ROBO_UNet())
    torch.manual_seed(23)
    x = torch.randn(2, 3, 48, 64, device=DEV)
    first = net.predict(x).clone()
    assert torch.equal(first, torch.max(net(x), 1)[1].to(torch.uint8))
    if how == "trainer_step":
        tr = Trainer(net, class_weights=[1, 10, 30, 10, 2], lr=1e-2, decay=1e-6)
        tr.step(x, torch.randint(0, 5, (2, 48, 64), device=DEV))
        net.eval()
    else:
        list(net.segmenter.parameters())[0].data.neg_()          # the classifier's weight; no version counter moves
        net.invalidate()
    second = net.predict(x)
    assert torch.equal(second, torch.max(net(x), 1)[1].to(torch.uint8))
    assert bool((second != first).any())


@pytest.mark.parametrize("size", [(24, 32), (48, 64)])
def test_segmenter_equals_the_composition(size):
    net = _build(lambda: M.ROBO_UNet()).train()
    frames = _dev(_frames(2, 48, 64, 9))
    seg = robocupvision_amd.Segmenter(net, img_size=size)
    assert net.training is False
    lab, col = seg(frames)
    imgs = D.prepare_batch(frames, torch.zeros(2, 48, 64, dtype=torch.uint8, device=DEV), size, train=False)[0]
    want = torch.max(net(imgs), 1)[1].to(torch.uint8)
    assert tuple(lab.shape) == (2,) + size and torch.equal(lab, want)
    assert torch.equal(col, P.device_palette(None, DEV)[want.long()])
    lab2, col2 = robocupvision_amd.Segmenter(net, img_size=size, finetune=True, palette=PAL[:6])(frames)
    imgs = D.prepare_batch(frames, torch.zeros(2, 48, 64, dtype=torch.uint8, device=DEV), size, finetune=True, train=False)[0]
    want = torch.max(net(imgs), 1)[1].to(torch.uint8)
    assert torch.equal(lab2, want) and torch.equal(col2, _dev(PAL)[want.long()])


def test_metrics_take_the_map_unchanged():
    from robocupvision_amd.metrics import DetectionMetrics, SegmentationMetrics
    net = _build(lambda: M.ROBO_UNet())
    torch.manual_seed(29)
    x = torch.randn(2, 3, 48, 64, device=DEV)
    t = torch.randint(0, 5, (2, 48, 64), device=DEV)
    lab = net.predict(x)
    want = torch.max(net(x), 1)[1]
    a, b = SegmentationMetrics(5, DEV), SegmentationMetrics(5, DEV)
    a.update(lab, t)
    b.update(want.to(torch.uint8), t)
    assert torch.equal(a.conf, b.conf) and float(a.conf.sum()) == 2 * 48 * 64
    da, db = DetectionMetrics(5, device=DEV), DetectionMetrics(5, device=DEV)
    da.update(lab, t)
    db.update(want, t)
    assert da.compute() == db.compute()
