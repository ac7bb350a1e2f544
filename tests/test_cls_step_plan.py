"""CPU: the training-step form of the fused 1x1 classifier (RCV_OP_CE_NORM + RCV_OP_CLS_STEP, csrc/small_kernels.hip) as the engine
plans it -- the third variant beside the fused-loss lists (Engine._cls_step_variant), lowered through the planning-only handle."""
import pytest
import torch

import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd.engine import Engine

HEADLINE = dict(noScale=True, planes=8, depth=4, levels=2, bellySize=5, bellyPlanes=128)      # bench.py robo_unet_640x480_bs32


def _lower(model, shape=(1, 3, 48, 64)):
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    plan = eng._plan_for([torch.zeros(shape)], True)
    return eng, plan, eng._ce_variant(plan)


def test_step_variant_of_the_headline_plan():
    torch.manual_seed(12345678)
    eng, plan, ce = _lower(M.ROBO_UNet(**HEADLINE))
    st = ce["step"]
    assert st is not None
    # backward: same length and indices, nothing launched in slot 0, every other record the fused-loss list's
    assert st["bwd"].n == plan.bwd.n == ce["bwd"].n
    assert st["bwd"].arr[0].kind == L.OP_NOP and ce["bwd"].arr[0].kind == L.OP_CLS_BWD
    for k in range(1, plan.bwd.n):
        assert bytes(st["bwd"].arr[k]) == bytes(ce["bwd"].arr[k]), k
    # forward: the fused-loss list without its classifier record, then the pre-pass and the fused record
    assert st["fwd"].n == ce["fwd"].n + 1
    for k in range(ce["fwd"].n - 1):
        assert bytes(st["fwd"].arr[k]) == bytes(ce["fwd"].arr[k]), k
    norm, step = st["fwd"].arr[st["fwd"].n - 2], st["fwd"].arr[st["fwd"].n - 1]
    assert (norm.kind, step.kind) == (L.OP_CE_NORM, L.OP_CLS_STEP)
    assert st["fwd"].labels(eng.handle)[-2:] == ["ce_norm", "cls_step"] and st["bwd"].labels(eng.handle)[0] == "nop"
    # the fused record writes where the two records wrote: same buffers, same workspace rows
    f, b = ce["fwd"].arr[ce["kf"]], ce["bwd"].arr[ce["kb"]]
    assert step.p[L.RCV_P_RESID] == f.p[L.RCV_P_OUT] == plan.logits.data_ptr()
    assert step.p[L.RCV_P_IN_AUX] == f.p[L.RCV_P_X2] == ce["argmax"].data_ptr()
    assert step.p[L.RCV_P_X5] == ce["loss_out"].data_ptr() and step.p[L.RCV_P_IN2_C] == f.p[L.RCV_P_PART]
    for slot in (L.RCV_P_OUT, L.RCV_P_PART, L.RCV_P_X1, L.RCV_P_X2, L.RCV_P_EPI_AUX, L.RCV_P_EPI_C, L.RCV_P_X3, L.RCV_P_X4, L.RCV_P_W, L.RCV_P_BIAS):
        assert step.p[slot] == b.p[slot], slot
    assert step.p[L.RCV_P_IN_C] == norm.p[L.RCV_P_PART] and norm.p[L.RCV_P_PART]
    assert step.i[L.RCV_I_NPART] == b.i[L.RCV_I_NPART] == f.i[L.RCV_I_NPART] == norm.i[L.RCV_I_NPART] > 0
    # algorithmic work
    px, cin, cout = 1 * 48 * 64, 8, 5
    assert Engine.op_work(step) == (6.0 * cin * cout * px, 4.0 * px * (cin + cin + cout + cin) + 9.0 * px)
    assert Engine.op_work(norm) == (0.0, 8.0 * px)
    assert Engine.op_work(st["bwd"].arr[0]) == (0.0, 0.0)


def test_step_variant_exists_where_the_issue_scopes_it():
    """Every class count of the 8-channel fused classifier has it; LabelProp's tail and 16-channel inputs keep their paths."""
    for n_class in range(1, 9):
        _eng, _plan, ce = _lower(M.ROBO_UNet(nClass=n_class))
        assert ce["step"] is not None, n_class
    eng, plan = _lower(M.ROBO_UNet(planes=16))[:2]
    assert not eng._ce_variant(plan)
    model = M.LabelProp(5, 32)
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    plan = eng._plan_for([torch.zeros(2, 48, 64, 8)], True)
    ce = eng._ce_variant(plan)
    assert ce and ce["step"] is None


def test_step_records_are_refused_by_the_query_like_by_the_launch():
    h = L.planner_handle(256)
    label = lambda op: L.OpList([op]).labels(h)[0]
    both = L.F_FUSED_UP | L.F_FUSED_CE
    kw = dict(n=2, h=8, w=8, stats=L.STATS_BWD_DEC)
    assert label(L.make_op(L.OP_CLS_STEP, both, cin=8, cout=5, **kw)) == "cls_step"
    assert label(L.make_op(L.OP_CE_NORM, 0, n=2, h=8, w=8, cout=5)) == "ce_norm"
    op = L.make_op(L.OP_CLS_STEP, both, cin=8, cout=5, **kw)
    bwd = L.make_op(L.OP_CLS_BWD, both, cin=8, cout=5, **kw)
    assert L.op_workspace(h, op) == L.op_workspace(h, bwd) and op.i[L.RCV_I_NPART] == bwd.i[L.RCV_I_NPART]
    bad = [
        L.make_op(L.OP_CLS_STEP, both, cin=16, cout=5, **kw),
        L.make_op(L.OP_CLS_STEP, both, cin=8, cout=9, **kw),
        L.make_op(L.OP_CLS_STEP, both, cin=8, cout=0, **kw),
        L.make_op(L.OP_CLS_STEP, L.F_FUSED_UP, cin=8, cout=5, **kw),
        L.make_op(L.OP_CLS_STEP, L.F_FUSED_CE, cin=8, cout=5, **kw),
        L.make_op(L.OP_CLS_STEP, both, cin=8, cout=5, n=2, h=8, w=8, stats=L.STATS_NONE),
        L.make_op(L.OP_CLS_STEP, both, cin=8, cout=5, aux0=L.LOAD_GRAD_ENC, **kw),
        L.make_op(L.OP_CLS_STEP, both, cin=8, cout=5, aux1=4, **kw),
        L.make_op(L.OP_CE_NORM, 0, n=2, h=8, w=8, cout=9),
        L.make_op(L.OP_CE_NORM, 0, n=0, h=8, w=8, cout=5),
    ]
    for op in bad:
        with pytest.raises(L.RcvError):
            label(op)
