"""CPU: class maps and colour masks (RCV_OP_CLS_LABEL, RCV_OP_FRAME_PREP; csrc/cls_label.hip, robocupvision_amd/palette.py, infer.py) --
the float64 restatement (tests/segment_restatement.py) pinned to torch on the CPU, the records on the planner handle with every
plan-time refusal, the Python-level refusals and the exported names."""
import numpy as np
import pytest
import torch

import segment_restatement as R
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import data as D
from robocupvision_amd import model as M
from robocupvision_amd import palette as P
from robocupvision_amd.engine import CLS3_PAD


# ------------------------------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize("cin,cout,fused,mode2,rch", [
    (8, 5, False, R.PLAIN, None), (8, 5, True, R.PLAIN, 8), (8, 3, True, R.AFFINE, 8), (8, 8, True, R.AFFINE_RELU, 4),
    (16, 5, True, R.AFFINE_RELU, 8), (16, 2, True, R.AFFINE, 16), (16, 1, False, R.PLAIN, None)])
def test_features_form_equals_torch(cin, cout, fused, mode2, rch):
    rng = np.random.default_rng(11)
    for make in (R.exact_case, R.random_case):
        d = make(rng, (2, 13, 19), cin, cout, fused, mode2, rch)
        v, lg = R.case_logits(d)
        # the same network tail in torch, float64, NCHW
        t = torch.from_numpy(d["t"]).double()
        x = t
        if fused:
            tc, rc = torch.from_numpy(d["tc"]).double(), torch.from_numpy(d["rc"]).double()
            x = torch.relu(t * tc[0] + tc[1])
            b = torch.from_numpy(d["r"]).double()
            if mode2 != R.PLAIN:
                b = b * rc[0] + rc[1]
            if mode2 == R.AFFINE_RELU:
                b = torch.relu(b)
            x = x.clone()
            x[:, :b.shape[1]] += b
        nchw = x.reshape(2, 13, 19, cin).permute(0, 3, 1, 2)
        want = torch.nn.functional.conv2d(nchw, torch.from_numpy(d["w"]).double()[:, :, None, None], torch.from_numpy(d["bias"]).double())
        got = torch.from_numpy(lg.reshape(2, 13, 19, cout)).permute(0, 3, 1, 2)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
        if make is R.exact_case:
            assert torch.equal(got, want)          # integer grid: exact in any order
        cls = R.first_argmax(lg).reshape(2, 13, 19)
        assert np.array_equal(cls, torch.max(want, 1)[1].numpy().astype(np.uint8))          # the pin: torch's first maximum
        assert np.array_equal(cls, R.first_argmax_loop(lg).reshape(2, 13, 19))
        if make is R.exact_case and cout > 2:
            assert int((R.top2_margin(lg) == 0).sum()) >= 20          # the exact cases do tie (494 pixels)


def test_logits_form_and_first_maximum_rule():
    rng = np.random.default_rng(12)
    z = rng.integers(-3, 4, (2, 13, 19, CLS3_PAD)).astype(np.float32)
    bias = rng.integers(-2, 3, 5).astype(np.float32)
    lg = R.logits_padded(z, 5, bias)
    want = torch.from_numpy(z).double()[..., :5] + torch.from_numpy(bias).double()
    assert torch.equal(torch.from_numpy(lg), want)
    assert np.array_equal(R.first_argmax(lg), torch.max(want, 3)[1].numpy().astype(np.uint8))
    # ties, NaN, infinities
    rows = np.array([[1, 3, 3, 2], [np.nan, 1, np.nan, 1], [np.nan] * 4, [-np.inf] * 4, [np.nan, -np.inf, 0, np.inf], [2, 2, 2, 2],
                     [np.inf, np.inf, 0, 0]], np.float64)
    assert R.first_argmax(rows).tolist() == [1, 1, 0, 0, 3, 0, 0] == R.first_argmax_loop(rows).tolist()
    assert R.first_argmax(np.zeros((4, 1))).tolist() == [0, 0, 0, 0]


def test_palette_lookup_equals_the_five_mask_loop():
    rng = np.random.default_rng(13)
    gray = rng.integers(0, 12, (13, 19)).astype(np.uint8)
    for n in (1, 3, 5):
        want = R.colorize_five_masks(gray, n)
        got = R.colour_image(gray, P.labelcolormap(n)).transpose(2, 0, 1)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(P.labelcolormap(5), R.PALETTE5) and P.labelcolormap(5).dtype == np.uint8
    assert P.labelcolormap(5).tolist() == [[0, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255]]
    assert np.array_equal(P.labelcolormap(7)[5:], np.zeros((2, 3), np.uint8)) and np.array_equal(P.labelcolormap(2), R.PALETTE5[:2])
    # classes beyond the palette and negative int64 classes are black
    cm = np.array([[0, 4, 8, 255], [-1, 7, 5, 1]], np.int64)
    assert R.colour_image(cm).tolist() == [[[0, 0, 0], [255, 255, 255], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 255]]]
    full = P.device_palette(None, "cpu")
    assert full.dtype == torch.uint8 and tuple(full.shape) == (8, 3) and np.array_equal(full.numpy(), R.palette8())


# ------------------------------------------------------------------------------------------ the records on the planner handle
def _rec(N=64, H=120, W=160, cin=8, cout=5, form=0, flags=0, elem=0, aux0=0, aux1=0, colour=False, palette=False, shape=0):
    return L.make_op(L.OP_CLS_LABEL, flags, n=N, h=H, w=W, cin=cin, cout=cout, inmode=form, inmode2=elem, aux0=aux0, aux1=aux1, count=shape,
                     p_x0=64 if colour else 0, p_x1=64 if palette else 0)          # (a planner handle never reads through a pointer)


@pytest.mark.parametrize("N,H,W", [(64, 120, 160), (32, 480, 640)])
def test_cls_label_plans_on_the_planner_handle(N, H, W):
    h = L.planner_handle(256)
    recs = []
    for cout in range(1, 9):
        for cin in (8, 16):
            recs.append(_rec(N, H, W, cin, cout))
            for mode in (L.LOAD_PLAIN, L.LOAD_AFFINE, L.LOAD_AFFINE_RELU):
                recs.append(_rec(N, H, W, cin, cout, flags=L.F_FUSED_UP, aux0=mode, aux1=0, colour=True, palette=True))
            recs.append(_rec(N, H, W, cin, cout, flags=L.F_FUSED_UP, aux1=4, shape=1))
        recs.append(_rec(N, H, W, CLS3_PAD, cout, form=1, colour=True, palette=True, shape=4))
        recs.append(_rec(N, H, W, 1, cout, form=2, elem=1, colour=True, palette=True))
        recs.append(_rec(N, H, W, 1, cout, form=2, elem=8, colour=True, palette=True))
    for op in recs:
        assert L.op_workspace(h, op) == 0
    assert L.OpList(recs).labels(h) == ["cls_label"] * len(recs)
    with pytest.raises(L.RcvError, match="planning-only handle"):
        L.OpList([recs[0]]).run(h, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(cout=0), "0 classes unsupported"), (dict(cout=9), "9 classes unsupported"),
    (dict(cin=4), "4 input channels unsupported"), (dict(cin=12), "12 input channels unsupported"),
    (dict(form=1, cin=4, cout=5), "4 floats per pixel for 5 classes"), (dict(form=1, cin=6, cout=5), "6 floats per pixel for 5 classes"),
    (dict(flags=L.F_FUSED_UP, aux1=3), "3 skip channels for 8 inputs"), (dict(flags=L.F_FUSED_UP, aux1=12), "12 skip channels for 8 inputs"),
    (dict(flags=L.F_FUSED_UP, cin=16, aux1=20), "20 skip channels for 16 inputs"), (dict(flags=L.F_FUSED_UP, aux0=2), "skip load mode 2"),
    (dict(form=3), "source form 3 unknown"), (dict(form=-1), "source form -1 unknown"),
    (dict(form=2, elem=4), "element size 4 unsupported"), (dict(form=2, elem=0), "element size 0 unsupported"),
    (dict(N=32768, H=256, W=256), r"N\*H\*W < 2\^31"), (dict(N=0), "every size must be >= 1"),
    (dict(colour=True), "needs the palette"), (dict(shape=2), "store shape 2 unknown"),
    (dict(form=1, flags=L.F_FUSED_UP), "belongs to source form 0"),
])
def test_cls_label_plan_time_refusals(kw, msg):
    h = L.planner_handle(256)
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(h, _rec(**kw))
    assert L.op_workspace(h, _rec(N=32767, H=256, W=256)) == 0          # 2^31 - 65536 pixels is inside


def _taps(n_in, n_out):
    return D.bilinear_table(n_in, n_out).shape[1] - 2


def _frec(B=64, Hs=480, Ws=640, H=120, W=160, tables=True, kx=None, ky=None):
    t = 64 if tables else 0
    return L.make_op(L.OP_FRAME_PREP, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=_taps(Ws, W) if kx is None else kx,
                     cout=_taps(Hs, H) if ky is None else ky, p_x1=t, p_x2=t, p_x5=t)


@pytest.mark.parametrize("B,H,W", [(64, 120, 160), (32, 480, 640)])
def test_frame_prep_plans_on_the_planner_handle(B, H, W):
    h = L.planner_handle(256)
    op = L.OpList([_frec(B=B, H=H, W=W)])
    assert L.op_workspace(h, op.arr[0]) == 0 and op.labels(h) == ["frame_prep"]
    with pytest.raises(L.RcvError, match="planning-only handle"):
        op.run(h, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), "every size must be >= 1"), (dict(H=59, ky=19), "shrinks an axis by more than 8"), (dict(tables=False), "null table"),
    (dict(kx=7), "taps per column / row")])
def test_frame_prep_plan_time_refusals(kw, msg):
    with pytest.raises(L.RcvError, match=msg):
        L.op_workspace(L.planner_handle(256), _frec(**kw))
    # the labelled record keeps its own refusals next to the new one
    with pytest.raises(L.RcvError, match="label element size 8 unsupported"):
        L.op_workspace(L.planner_handle(256), L.make_op(L.OP_BATCH_PREP, n=2, h=24, w=32, ho=12, wo=16, cin=_taps(32, 16), cout=_taps(24, 12),
                                                        inmode2=8, p_x1=64, p_x2=64, p_x3=64, p_x4=64, p_x5=64))


# ------------------------------------------------------------------------------------------ the Python surface
def test_exported_names():
    from robocupvision_amd.infer import Segmenter
    assert robocupvision_amd.Segmenter is Segmenter and robocupvision_amd.colorize is P.colorize
    assert robocupvision_amd.Colorize is P.Colorize and robocupvision_amd.labelcolormap is P.labelcolormap
    assert robocupvision_amd.prepare_frames is D.prepare_frames
    for cls in (M.ROBO_UNet, M.PB_FCN, M.PB_FCN_2, M.LabelProp):
        assert callable(getattr(cls, "predict"))
    assert L.OP_CLS_LABEL == 37 and L.OP_FRAME_PREP == 38


def test_predict_refusals():
    x = torch.zeros(1, 3, 48, 64)
    net = M.ROBO_UNet()
    with pytest.raises(L.RcvError, match=r"call `\.eval\(\)` first"):
        net.predict(x)
    with pytest.raises(L.RcvError, match="HIP device only"):
        net.eval().predict(x)                               # CPU tensor: there is no CPU path
    with pytest.raises(L.RcvError, match="HIP device only"):
        M.LabelProp(5, 32).eval().predict(torch.zeros(1, 8, 24, 32))
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN(32, 5, 1, False, 1).eval().predict(x)
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN_2(True).eval().predict(x)
    with pytest.raises(L.RcvError, match="classify mode"):
        robocupvision_amd.Segmenter(M.PB_FCN_2(True))
    with pytest.raises(L.RcvError, match="no per-pixel classifier"):
        M.Conv(8, 8, 3).eval().predict(torch.zeros(1, 8, 8, 8))
    with pytest.raises(TypeError):
        net.predict(None)


def test_labels_plan_refuses_graphs_without_a_pixel_classifier():
    from robocupvision_amd.engine import Engine
    for net, word in ((M.PB_FCN_2(True), "pool_cls"), (M.PB_FCN(32, 5, 1, False, 1), "pool_cls")):
        eng = Engine(net._graph(), list(net.parameters()), M._bn_modules(net), dry_run=True)
        x = torch.zeros(1, 3, 48, 64)
        eng._plan_for([x], False)                              # the eval plan lowers
        with pytest.raises(L.RcvError, match=word):
            eng._plan_for([x], False, labels=True)
    blk = M.Conv(8, 8, 3)
    eng = Engine(blk._block_graph(), list(blk.parameters()), M._bn_modules(blk), dry_run=True)
    with pytest.raises(L.RcvError, match="fwd_mat"):
        eng._plan_for([torch.zeros(1, 8, 8, 8)], False, labels=True)


@pytest.mark.parametrize("make,shape,tail", [
    (lambda: M.ROBO_UNet(), (2, 3, 48, 64), 1), (lambda: M.ROBO_UNet(v2=True, classSize=3, levels=1, bellySize=9), (1, 3, 48, 64), 2),
    (lambda: M.PB_FCN(32, 5, 1, False, 0), (2, 3, 48, 64), 1), (lambda: M.LabelProp(5, 32), (2, 24, 32, 8), 1)])
def test_labels_plan_lowering(make, shape, tail):
    """The eval-labels plan is the eval plan with another tail: same records up to the classifier, RCV_OP_CLS_LABEL at the end, no
    logits buffer; cached beside the other variants under its own key."""
    from robocupvision_amd.engine import Engine
    net = make()
    eng = Engine(net._graph(), list(net.parameters()), M._bn_modules(net), dry_run=True)
    x = torch.zeros(*shape)
    ev, lb = eng._plan_for([x], False), eng._plan_for([x], False, labels=True)
    assert lb is not ev and eng._plan_for([x], False, labels=True) is lb and len(eng.plans) == 2
    assert [k for (_, k) in eng.plans] == [False, None]          # a truth value for every reader of the cache: only True is training
    kinds_e, kinds_l = [op.kind for op in ev.fwd.arr[:ev.fwd.n]], [op.kind for op in lb.fwd.arr[:lb.fwd.n]]
    assert kinds_l[:-1] == kinds_e[:-1] and kinds_l[-1] == L.OP_CLS_LABEL
    assert kinds_e[-1] == (L.OP_NHWC_TO_NCHW if tail == 2 else L.OP_CLS_FWD)
    assert lb.fwd.labels(eng.handle)[-1] == "cls_label" and lb.label_op == lb.fwd.n - 1
    op = lb.fwd.arr[lb.label_op]
    assert op.i[L.RCV_I_INMODE] == (L.CLS_LABEL_LOGITS if tail == 2 else L.CLS_LABEL_FEATURES)
    assert lb.logits is None and not lb.logits_slots and lb.label_shape == ((shape[0],) + (shape[2:] if shape[1] == 3 else shape[1:3]))
    n_logits = 4 * shape[0] * 5 * lb.label_shape[1] * lb.label_shape[2]
    assert ev.bytes - lb.bytes == n_logits


def test_palette_and_frame_refusals():
    with pytest.raises(ValueError):
        P.device_palette(torch.zeros(9, 3, dtype=torch.uint8), "cpu")
    with pytest.raises(ValueError):
        P.device_palette(torch.zeros(5, 4, dtype=torch.uint8), "cpu")
    with pytest.raises(TypeError):
        P.device_palette(torch.zeros(5, 3), "cpu")
    with pytest.raises(ValueError):
        robocupvision_amd.Segmenter(M.ROBO_UNet(), palette=np.zeros((9, 3), np.uint8))
    padded = P.device_palette(np.array([[1, 2, 3], [4, 5, 6]], np.uint8), "cpu")
    assert padded.tolist() == [[1, 2, 3], [4, 5, 6]] + [[0, 0, 0]] * 6
    lab = torch.zeros(2, 13, 19, dtype=torch.uint8)
    with pytest.raises(L.RcvError, match="HIP device only"):
        P.colorize(lab)
    with pytest.raises(L.RcvError, match="HIP device only"):
        P.Colorize()(lab[0])
    with pytest.raises(TypeError):
        P.colorize(lab.float())
    with pytest.raises(ValueError):
        P.colorize(lab[None])
    with pytest.raises(ValueError):
        P.Colorize(9)
    f = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    with pytest.raises(L.RcvError, match="HIP device only"):
        D.prepare_frames(f, (12, 16))
    with pytest.raises(TypeError):
        D.prepare_frames(f.float(), (12, 16))
    with pytest.raises(ValueError):
        D.prepare_frames(f[:, :, :, :2], (12, 16))
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.prepare_frames(f, (24, 16))
    with pytest.raises(ValueError, match="dataset.py:118-121"):
        D.prepare_frames(f, (12, 32), finetune=True)
    assert robocupvision_amd.Segmenter(M.ROBO_UNet()).model.training is False
