"""CPU: the softmax tail's restatement (tests/proba_restatement.py) pinned to torch.softmax in float64, its counted rounding bound,
the pseudo-label rule, and the refusals of ``proba`` / ``Segmenter(pseudo_labels=...)`` that need no device."""
import math

import numpy as np
import pytest
import torch

import lp_input_restatement as LP
import proba_restatement as P
import robocupvision_amd
import robocupvision_amd.model as M
from plan_census import label_of
from robocupvision_amd import _lib as L


@pytest.mark.parametrize("C", range(1, 9))
def test_softmax_is_torch_softmax_in_float64(C):
    rng = np.random.default_rng(50 + C)
    for z in (3.0 * rng.standard_normal((2, C, 5, 7)), rng.uniform(-60, 60, (2, C, 5, 7)), 1e4 + rng.standard_normal((2, C, 5, 7)),
              np.repeat(rng.standard_normal((2, 1, 5, 7)), C, axis=1)):
        z = z.astype(np.float32)
        want = torch.softmax(torch.from_numpy(z).double(), 1).numpy()
        got, cls = P.proba(z)
        assert got.dtype == np.float64 and float(np.abs(got - want).max()) <= 4 * 2.0 ** -53
        assert np.array_equal(cls, P.S.first_argmax_loop(np.moveaxis(z, 1, -1)))
        assert float(np.abs(got.sum(1) - 1.0).max()) <= C * 2.0 ** -52


def test_bound_is_the_soft_prior_bound_generalised():
    u = 2.0 ** -24
    assert P.U == u
    for C in range(1, 9):
        first_order = (C / math.e + C + 8) * u
        assert first_order < P.proba_bound(C) <= first_order + 2 * u
    assert [round(P.proba_bound(C) / u) for C in (1, 2, 5, 8)] == [11, 12, 16, 20]
    # 2 * q - 1: twice the error of q plus the subtraction's rounding -- the bound lp_input_restatement states for five classes
    assert 2 * P.proba_bound(5) <= LP.SOFT_BOUND < 2 * P.proba_bound(5) + 2 * u
    # the restatement itself is lp_input_restatement's softmax
    z = (3.0 * np.random.default_rng(1).standard_normal((2, 5, 3, 4))).astype(np.float32)
    assert np.array_equal(2.0 * P.softmax(z, axis=1) - 1.0, LP.soft_prior(z))


def test_confidence_and_pseudo_labels():
    prob = np.array([[[[0.9, 0.5]], [[0.1, 0.5]]]], np.float32)          # [1, 2, 1, 2]
    cls = np.array([[[0, 0]]], np.uint8)
    conf = P.confidence(prob, cls)
    assert conf.dtype == np.float32 and conf.tolist() == [[[np.float32(0.9), 0.5]]]
    assert P.pseudo_labels(conf, cls, 0.9).tolist() == [[[0, -100]]]          # fp32(0.9) >= fp32(0.9): the comparison runs in fp32
    assert P.pseudo_labels(conf, cls, 0.0).tolist() == [[[0, 0]]] and P.pseudo_labels(conf, cls, 1.0).tolist() == [[[-100, -100]]]
    assert P.pseudo_labels(np.array([np.nan, 1.0], np.float32), np.array([3, 4]), 0.0).tolist() == [-100, 4]
    assert P.pseudo_labels(conf, cls, 0.9).dtype == np.int64


def test_record_is_planned_and_refused_on_the_planner():
    h = L.planner_handle()
    assert L.OP_CLS_PROBA == 67 and "rcv_cls_proba" in L.EXPORTS and hasattr(L.load(), "rcv_cls_proba")
    for cin, fused, form in ((8, False, 0), (8, True, 0), (16, False, 0), (16, True, 0), (8, False, 1)):
        op = L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP if fused else 0, n=3, h=5, w=7, cin=cin, cout=5, inmode=form, aux0=L.LOAD_AFFINE_RELU, aux1=8)
        assert label_of(h, op) == "cls_proba" and L.op_workspace(h, op) == 0
    for kw, word in ((dict(inmode=2), "source form"), (dict(cout=0), "classes"), (dict(cout=9), "classes"), (dict(cin=12), "input channels"),
                     (dict(inmode=1, cin=4), "floats per pixel"), (dict(n=0), "every size"), (dict(n=70000, h=200, w=200), "2\\^31")):
        with pytest.raises(L.RcvError, match=word):
            L.op_workspace(h, L.make_op(L.OP_CLS_PROBA, 0, **{**dict(n=3, h=5, w=7, cin=8, cout=5, inmode=0), **kw}))
    with pytest.raises(L.RcvError, match="skip channels"):
        L.op_workspace(h, L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, n=3, h=5, w=7, cin=8, cout=5, inmode=0, aux1=6))


def test_proba_refusals_without_a_device():
    x = torch.zeros(1, 3, 48, 64)
    net = M.ROBO_UNet()
    for cls in (M.ROBO_UNet, M.PB_FCN, M.PB_FCN_2, M.LabelProp, M.FCN):
        assert callable(getattr(cls, "proba"))
    with pytest.raises(L.RcvError, match=r"call `\.eval\(\)` first"):
        net.proba(x)
    with pytest.raises(L.RcvError, match="HIP device only"):
        net.eval().proba(x)
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN_2(True).eval().proba(x)
    with pytest.raises(L.RcvError, match="no per-pixel classifier"):
        M.Conv(8, 8, 3).eval().proba(torch.zeros(1, 8, 8, 8))
    with pytest.raises(TypeError):
        net.proba(None)
    with pytest.raises(ValueError, match="threshold"):
        robocupvision_amd.Segmenter(net, pseudo_labels=-0.1)
    with pytest.raises(ValueError):
        robocupvision_amd.Segmenter(net, pseudo_labels="high")


def test_proba_plan_refuses_graphs_without_a_pixel_classifier():
    from robocupvision_amd.engine import Engine
    net = M.PB_FCN_2(True)
    eng = Engine(net._graph(), list(net.parameters()), M._bn_modules(net), dry_run=True)
    with pytest.raises(L.RcvError, match="pool_cls"):
        eng._plan_for([torch.zeros(1, 3, 48, 64)], False, labels="proba")
