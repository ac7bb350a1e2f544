"""The 5x5 classifier convolution family without a device: what the library's query accepts and refuses (include/rcv.h RCV_OP_CONV5,
RCV_OP_WGRAD5, RCV_OP_WGRAD5_REDUCE, RCV_OP_PACK5), the modules and their lowering, the exported configuration, and the float64
restatement (tests/cls5_restatement.py) pinned to torch.nn.functional.conv2d and its autograd."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cls5_restatement as R      # noqa: E402
import robocupvision_amd.model as M      # noqa: E402
from robocupvision_amd import _lib as L      # noqa: E402
from robocupvision_amd import export      # noqa: E402
from robocupvision_amd.engine import Engine      # noqa: E402


def _label(op):
    return L.OpList([op]).labels(L.planner_handle(256))[0]


def _conv(cin, cout, n=2, h=3, w=4, stride=1, dil=1, inmode=L.LOAD_PLAIN, **kw):
    return L.make_op(L.OP_CONV5, kw.pop("flags", 0), n=n, h=h, w=w, cin=cin, cout=cout, ho=h, wo=w, stride=stride, dil=dil, inmode=inmode, **kw)


def _wgrad(cin, cout=8, n=2, h=3, w=4, stride=1, dil=1, inmode=L.LOAD_PLAIN, inmode2=L.LOAD_PLAIN):
    return L.make_op(L.OP_WGRAD5, L.F_BIAS, n=n, h=h, w=w, cin=cin, cout=cout, ho=h, wo=w, stride=stride, dil=dil, inmode=inmode,
                     inmode2=inmode2)


@pytest.mark.parametrize("plane", [(3, 4), (120, 160)])
@pytest.mark.parametrize("cin", [8, 16])
def test_the_query_accepts_the_classifier_records(plane, cin):
    h, w = plane
    tile = "16x16" if w <= 16 else "8x32"
    assert _label(_conv(cin, 8, h=h, w=w)) == "conv5_mfma<%d,%s>" % (cin, tile)                      # forward, 1..8 classes padded to 8
    assert _label(_conv(8, cin, h=h, w=w, flags=L.F_RESID, stats=L.STATS_BWD_DEC)) == "conv5_mfma<8,%s>" % tile      # data gradient
    assert _label(_wgrad(cin, h=h, w=w)) == "wgrad5_mfma<%d,%s>" % (cin, tile)
    for mode in (L.LOAD_AFFINE, L.LOAD_AFFINE_RELU):
        _label(_conv(cin, 8, h=h, w=w, inmode=mode))
        _label(_wgrad(cin, h=h, w=w, inmode=mode))
    for classes in (1, 5, 8):
        assert _label(L.make_op(L.OP_PACK5, 0, cin=cin, cout=classes)) == "pack5<fwd>"
        assert _label(L.make_op(L.OP_PACK5, L.F_FLIP, cin=cin, cout=classes)) == "pack5<dgrad>"
        assert _label(L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=cin, cout=classes, nsplit=3)) == "wgrad5_reduce"
    # workspaces: one statistics row per 256-pixel tile; one partial filter + bias row per split (at most one per compute unit)
    tiles = 2 * -(-h // (16 if w <= 16 else 8)) * -(-w // (16 if w <= 16 else 32))
    op = _conv(8, cin, h=h, w=w, stats=L.STATS_BWD_ENC)
    assert L.op_workspace(L.planner_handle(256), op) == tiles * 2 * cin * 4 and op.i[L.RCV_I_NPART] == tiles
    op = _wgrad(cin, h=h, w=w)
    assert L.op_workspace(L.planner_handle(256), op) == min(tiles, 256) * (25 * 8 * 16 + 8) * 4 and op.i[L.RCV_I_NSPLIT] == min(tiles, 256)
    assert L.op_workspace(L.planner_handle(256), _conv(cin, 8, h=h, w=w)) == 0


@pytest.mark.parametrize("op,what", [
    (lambda: _conv(4, 8), "channels 4 -> 8"),
    (lambda: _conv(32, 8), "channels 32 -> 8"),
    (lambda: _conv(16, 16), "at most 8 classes"),                 # more than 8 padded class channels
    (lambda: _conv(8, 12), "channels 8 -> 12"),
    (lambda: _conv(8, 8, stride=2), "stride 1 / dilation 1"),
    (lambda: _conv(8, 8, dil=2), "stride 1 / dilation 1"),
    (lambda: _conv(8, 8, inmode=L.LOAD_GRAD_ENC), "load mode 2"),
    (lambda: _conv(8, 8, inmode=L.LOAD_NCHW), "load mode 4"),
    (lambda: L.make_op(L.OP_CONV5, 0, n=2, h=6, w=8, cin=8, cout=8, ho=3, wo=4, stride=1, dil=1), "output plane"),
    (lambda: _wgrad(4), "channels 4"),
    (lambda: _wgrad(32), "channels 32"),
    (lambda: _wgrad(8, cout=16), "at most 8 classes"),
    (lambda: _wgrad(8, stride=2), "stride 1 / dilation 1"),
    (lambda: _wgrad(8, dil=2), "stride 1 / dilation 1"),
    (lambda: _wgrad(8, inmode2=L.LOAD_AFFINE), "pointwise operand"),
    (lambda: L.make_op(L.OP_PACK5, 0, cin=8, cout=9), "9 classes"),
    (lambda: L.make_op(L.OP_PACK5, 0, cin=4, cout=5), "4 input channels"),
    (lambda: L.make_op(L.OP_PACK5, L.F_FLIP, cin=32, cout=5), "32 input channels"),
    (lambda: L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=8, cout=9, nsplit=2), "9 classes"),
    (lambda: L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=32, cout=5, nsplit=2), "32 input channels"),
])
def test_the_query_refuses_with_a_message(op, what):
    with pytest.raises(L.RcvError) as e:
        _label(op())
    assert what in str(e.value), str(e.value)
    with pytest.raises(L.RcvError):      # the workspace query refuses the same records
        L.op_workspace(L.planner_handle(256), op())


def test_named_entry_points_are_exported():
    lib = L.load()
    assert lib.rcv_conv5x5 and lib.rcv_wgrad5x5
    h = L.planner_handle(256)
    assert lib.rcv_conv5x5(h, _wgrad(8), None) != 0 and b"RCV_OP_CONV5" in lib.rcv_last_error()
    assert lib.rcv_wgrad5x5(h, _conv(8, 8), None) != 0 and b"RCV_OP_WGRAD5" in lib.rcv_last_error()


# ------------------------------------------------------------------------------------------ modules and lowering
def _lower(model, shape=(2, 3, 48, 64), training=True, labels=False):
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    return eng, eng._plan_for([torch.zeros(shape)], training, labels)


def test_ult_classifier_takes_size_5():
    c = M.UltClassifier(8, 5, False, size=5)
    assert tuple(c.layers.Class.weight.shape) == (5, 8, 5, 5) and c.layers.Class.padding == (2, 2)
    with pytest.raises(NotImplementedError):
        M.UltClassifier(8, 5, False, size=7)


def test_pooled_5x5_heads_say_that_they_are_not_built():
    with pytest.raises(NotImplementedError, match="5x5 classifier behind the pool is not built"):
        M.UltClassifier(8, 5, True, size=5)
    with pytest.raises(NotImplementedError, match="5x5 classifier behind the pool is not built"):
        M.PB_FCN(32, 5, 5, False, 1)._graph()
    with pytest.raises(NotImplementedError, match="5x5 classifier behind the pool is not built"):
        M.Classifier(64, 5, poolSize=4, kernelSize=5)._head_node(("in", 0))
    M.PB_FCN(32, 5, 1, False, 1)._graph()       # the 1x1 pooled head is untouched


NETS = {
    "pbfcn": (lambda c: M.PB_FCN(32, c, 5, False, 0), 8),
    "pbfcn_noscale": (lambda c: M.PB_FCN(32, c, 5, True, 0), 8),
    "robo": (lambda c: M.ROBO_UNet(nClass=c, classSize=5), 8),
    "v2": (lambda c: M.ROBO_UNet(nClass=c, v2=True, classSize=5, levels=1, bellySize=2), 16),
}


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("classes", [1, 2, 3, 4, 5, 6, 7, 8])
def test_5x5_networks_lower_in_every_mode(net, classes):
    make, cin = NETS[net]
    model = make(classes)
    eng, plan = _lower(model)
    f, b = plan.fwd.labels(eng.handle), plan.bwd.labels(eng.handle)
    conv = "conv5_mfma<%d,8x32>" % cin
    assert f[-2:] == [conv, "nhwc_to_nchw"] and f.count("pack5<fwd>") == 1 and f.count("pack5<dgrad>") == 1
    assert b[:4] == ["nchw_to_nhwc", "wgrad5_mfma<%d,8x32>" % cin, "wgrad5_reduce", "conv5_mfma<8,8x32>"]
    # the data gradient carries the epilogue of the producer: a decoder block (statistics rows) or, v2, the concat (none)
    dgrad = plan.bwd.arr[3]
    assert dgrad.kind == L.OP_CONV5 and dgrad.i[L.RCV_I_COUT] == cin
    assert dgrad.i[L.RCV_I_STATS] == (L.STATS_NONE if net == "v2" else L.STATS_BWD_DEC)
    side = [plan.bwd.arr[k].flags & L.F_SIDE_STREAM for k in range(4)]
    assert side[1] and side[2] and not side[0] and not side[3]      # the filter gradient leaves the critical path, as the 3x3 one does
    model.eval()
    eng, plan = _lower(model, training=False)
    assert plan.fwd.labels(eng.handle)[-2:] == [conv, "nhwc_to_nchw"] and plan.bwd.n == 0
    eng, plan = _lower(model, training=False, labels=True)
    assert plan.fwd.labels(eng.handle)[-2:] == [conv, "cls_label"]
    assert plan.fwd.arr[plan.label_op].i[L.RCV_I_INMODE] == L.CLS_LABEL_LOGITS


def test_nine_classes_and_wide_inputs_stay_refused():
    for model, what in ((M.PB_FCN(32, 9, 5, False, 0), "9 classes"), (M.ROBO_UNet(planes=32, classSize=5), "channels 32"),
                        (M.ROBO_UNet(planes=4, classSize=5), "channels 4")):
        with pytest.raises(L.RcvError) as e:
            _lower(model)
        assert what in str(e.value), str(e.value)
    with pytest.raises(NotImplementedError):
        M.Conv(8, 8, size=5)


def test_1x1_and_3x3_classifier_plans_are_what_they_were():
    """The kernel labels of one 1x1 and one 3x3 classifier net as the parent commit reports them (scripts/plan_diff.sh compares whole
    lists): the 5x5 branch adds records to its own plans only."""
    eng, plan = _lower(M.ROBO_UNet())
    f, b = plan.fwd.labels(eng.handle), plan.bwd.labels(eng.handle)
    assert f[-1] == "cls_fwd" and b[0] == "cls_bwd" and not any("5" in s.split("<")[0] for s in f + b)
    eng, plan = _lower(M.ROBO_UNet(v2=True, classSize=3, levels=1, bellySize=2))
    f, b = plan.fwd.labels(eng.handle), plan.bwd.labels(eng.handle)
    assert f[-2:] == ["convs_mfma<1,5,16>", "nhwc_to_nchw"], f[-2:]
    assert b[:4] == ["nchw_to_nhwc", "wgrad_mfma<1,1,1,1,4,f0>", "nop", "convs_mfma<1,5,8>"], b[:4]      # (nop: the reduction, batched further down)
    assert not any(s.startswith(("conv5", "wgrad5", "pack5")) for s in f + b)


def test_export_writes_size_5_pad_2_for_the_segmenter():
    cfg = export.net_cfg(M.PB_FCN(32, 5, 5, False, 0))
    assert "size=5" in cfg and "pad=2" in cfg
    block = [b for b in cfg.split("[convolutional]") if "size=5" in b]
    assert block and all("pad=2" in b and "filters=5" in b for b in block)


# ------------------------------------------------------------------------------------------ the restatement against conv2d in float64
@pytest.mark.parametrize("cin,classes,plane", [(8, 5, (3, 4)), (16, 8, (5, 7)), (8, 1, (9, 6)), (16, 5, (8, 33))])
def test_restatement_equals_conv2d_and_its_autograd(cin, classes, plane):
    H, W = plane
    gen = torch.Generator().manual_seed(7 + cin + classes)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    N = 2
    x, c = rnd(N, H, W, cin), rnd(5, cin)
    w, bias = rnd(classes, cin, 5, 5).requires_grad_(), rnd(classes).requires_grad_()
    g, resid = rnd(N, H, W, 8), rnd(N, H, W, cin)
    g[..., classes:] = 0
    for mode in (R.LOAD_PLAIN, R.LOAD_AFFINE, R.LOAD_AFFINE_RELU):
        v = R.load(mode, x, c).requires_grad_()
        expect = {R.LOAD_PLAIN: x, R.LOAD_AFFINE: x * c[0] + c[1], R.LOAD_AFFINE_RELU: torch.relu(x * c[0] + c[1])}[mode]
        assert torch.equal(v.detach(), expect)
        ref = F.conv2d(v.permute(0, 3, 1, 2), w, bias, padding=2).permute(0, 2, 3, 1)
        # pack layout, forward: [25][CIN][16], out[t][ci][co] = w[co][ci][t]
        p = R.pack5(w.detach(), False)
        assert p.shape == (25, cin, 16) and not p[:, :, classes:].any()
        assert torch.equal(p[:, :, :classes], w.detach().reshape(classes, cin, 25).permute(2, 1, 0))
        z = R.conv5(v.detach(), p, 8, bias=torch.cat([bias.detach(), torch.zeros(8 - classes, dtype=torch.float64)]))
        assert torch.allclose(z[..., :classes], ref.detach(), rtol=0, atol=1e-12) and not z[..., classes:].any()
        # backward of sum(ref * g): data, filter and bias gradients
        dv, dw, db = torch.autograd.grad(ref, (v, w, bias), g[..., :classes])
        # pack layout, data gradient: [25][8][16], out[t][co][ci] = w[co][ci][24 - t]
        pd = R.pack5(w.detach(), True)
        assert pd.shape == (25, 8, 16) and not pd[:, classes:].any() and not pd[:, :, cin:].any()
        assert torch.equal(pd[:, :classes, :cin], w.detach().reshape(classes, cin, 25).flip(2).permute(2, 0, 1))
        assert torch.allclose(R.conv5(g, pd, cin), dv, rtol=0, atol=1e-12)
        assert torch.allclose(R.conv5(g, pd, cin, resid=resid), dv + resid, rtol=0, atol=1e-12)
        rw, rb = R.wgrad5(v.detach(), g)
        assert torch.allclose(rw[:classes], dw, rtol=0, atol=1e-11) and torch.allclose(rb[:classes], db, rtol=0, atol=1e-11)
        assert not rw[classes:].any() and not rb[classes:].any()
    # statistics rows of a data-gradient writer
    e, epi_c = rnd(N, H, W, cin), rnd(3, cin)
    out = R.conv5(g, R.pack5(w.detach(), True), cin, resid=resid)
    enc, dec = R.stats_rows(R.STATS_BWD_ENC, out, e, epi_c), R.stats_rows(R.STATS_BWD_DEC, out, e, epi_c)
    assert torch.allclose(enc[0], out.sum((0, 1, 2))) and torch.allclose(enc[1], (out * (e - epi_c[2])).sum((0, 1, 2)))
    m = (e * epi_c[0] + epi_c[1] > 0).double()
    assert torch.allclose(dec[0], (out * m).sum((0, 1, 2))) and torch.allclose(dec[1], (out * m * (e - epi_c[2])).sum((0, 1, 2)))
