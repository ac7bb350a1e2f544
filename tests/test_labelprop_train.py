"""CPU: LabelProp's training step (labelPropTrain.py:162-215) -- the plans on the planner handle, the query-time refusals of the
new records, the float64 restatement of the tail and of the batch assembly against the reference's goldens
(tests/golden/make_golden_labelprop_train.py), and the Python-level refusals."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, sd_hash
import labelprop_restatement as R
import small_ops_restatement as S
import robocupvision_amd
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd.engine import Engine
from robocupvision_amd.train import Trainer

with open(os.path.join(GOLDEN, "labelprop_train.json")) as _f:
    META = json.load(_f)


def kats(tag):
    return np.load(os.path.join(GOLDEN, "labelprop_train_%s.npz" % tag[3:]))


def _lower(model, shape, training=True):
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    return eng, eng._plan_for([torch.zeros(shape)], training)


def _is_tail(op, kind=L.OP_LP_TAIL_FWD):
    return op.kind == kind and bool(op.flags & L.F_FUSED_UP) and op.i[L.RCV_I_CIN] == 16 and op.i[L.RCV_I_AUX1] == 8


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (2, 40, 24, 8), (16, 120, 160, 8)])
def test_training_plan_lowers_with_one_tail_launch(shape):
    """Fails on a tree without the feature: the engine refuses every training graph that holds an add_slice node."""
    model = M.LabelProp(5, 32)
    eng, plan = _lower(model, shape, training=True)
    assert len(eng.param_list) == 35 and all(eng.param_used) and sum(p.numel() for p in eng.param_list) == 92277
    fwd = [plan.fwd.arr[k] for k in range(plan.fwd.n)]
    bwd = [plan.bwd.arr[k] for k in range(plan.bwd.n)]
    assert sum(_is_tail(op) for op in fwd) == 1 and _is_tail(fwd[-1])
    assert not any(op.kind in (L.OP_MATERIALIZE, L.OP_ADD_SLICE) for op in fwd)
    b0 = bwd[0]
    assert (b0.kind == L.OP_LP_TAIL_BWD and b0.flags & L.F_FUSED_UP and b0.i[L.RCV_I_AUX1] == 8 and b0.i[L.RCV_I_STATS] == L.STATS_BWD_DEC
            and b0.p[L.RCV_P_IN_AUX] and b0.p[L.RCV_P_OUT])
    assert sum(op.kind in (L.OP_CLS_BWD, L.OP_LP_TAIL_BWD) for op in bwd) == 1 and not any(op.kind == L.OP_BWD_STATS for op in bwd)
    assert not any(op.kind in (L.OP_CLS_FWD, L.OP_CE_FWD, L.OP_CE_BWD) for op in fwd + bwd)
    # the 8-channel skip gradient rides into down1's data-gradient launch as its residual: no accumulation pass
    resid = [op for op in bwd if op.flags & L.F_RESID and op.p[L.RCV_P_RESID] == b0.p[L.RCV_P_IN_AUX]]
    assert len(resid) == 1 and resid[0].kind == L.OP_TCONV and resid[0].i[L.RCV_I_COUT] == 8
    assert plan.bwd.labels(eng.handle)[0] == "lp_tail_bwd<5,0>"
    # the fused-loss variant: forward tail with the loss, backward tail that forms d loss / d logits itself
    ce = eng._ce_variant(plan)
    assert plan.fwd.labels(eng.handle)[-1] == "lp_tail_fwd<0>"
    assert ce and ce["fwd"].labels(eng.handle)[-1] == "lp_tail_fwd<1>" and ce["bwd"].labels(eng.handle)[0] == "lp_tail_bwd<5,1>"
    # gradient-ready marks tile the flat buffer from the top down, as for the other nets
    assert plan.bwd_marks and plan.bwd_marks[-1][1] == 0 and plan.bwd_marks[-1][0] == plan.bwd.n
    assert all(a[1] >= b[1] and a[0] < b[0] for a, b in zip(plan.bwd_marks, plan.bwd_marks[1:]))


def test_eval_plan_is_unchanged():
    eng, plan = _lower(M.LabelProp(5, 32), (2, 120, 160, 8), training=False)
    labels = plan.fwd.labels(eng.handle)
    assert labels[-1] == "cls_fwd" and _is_tail(plan.fwd.arr[plan.fwd.n - 1], L.OP_CLS_FWD) and plan.bwd.n == 0
    assert not any(l in ("materialize", "add_slice", "combine") for l in labels)
    assert sum(plan.fwd.arr[k].kind in (L.OP_CONV, L.OP_TCONV) for k in range(plan.fwd.n)) == 10


@pytest.mark.parametrize("n_class", [1, 3, 8])
def test_other_class_counts_plan(n_class):
    eng, plan = _lower(M.LabelProp(n_class, 32), (2, 16, 16, 8))
    assert eng._ce_variant(plan) and plan.bwd.labels(eng.handle)[0] == "lp_tail_bwd<%d,0>" % n_class


def test_add_slice_outside_the_tail_is_refused_in_training_with_what_is_built():
    model = M.LabelProp(5, 32)
    g = model._graph()
    g["nodes"][-2]["src"], g["nodes"][-2]["add"] = ("node", 0), ("node", 0)      # an 8-channel conv block as the source
    g["nodes"][-1] = {"op": "mat", "src": ("node", len(g["nodes"]) - 2)}
    eng = Engine(g, list(model.parameters()), M._bn_modules(model), dry_run=True)
    with pytest.raises(L.RcvError, match="LabelProp's tail only"):
        eng._plan_for([torch.zeros(2, 16, 16, 8)], True)


def _rec(kind, flags=L.F_FUSED_UP, **kw):
    base = dict(n=2, h=9, w=11, cin=16, cout=5, aux0=L.LOAD_AFFINE_RELU, aux1=8)
    if kind == L.OP_LP_TAIL_BWD:
        base["stats"] = L.STATS_BWD_DEC
    base.update(kw)
    return L.make_op(kind, flags, **base)


def test_the_query_refuses_what_the_launch_would_refuse():
    h = L.planner_handle(256)
    for kind in (L.OP_LP_TAIL_FWD, L.OP_LP_TAIL_BWD):
        for flags in (L.F_FUSED_UP, L.F_FUSED_UP | L.F_FUSED_CE):
            for ok in (dict(), dict(cout=1), dict(cout=8), dict(aux1=4), dict(aux1=12), dict(aux1=16), dict(aux0=L.LOAD_PLAIN),
                       dict(aux0=L.LOAD_AFFINE)):
                op = _rec(kind, flags, **ok)
                nbytes = L.op_workspace(h, op)
                if kind == L.OP_LP_TAIL_BWD:
                    co = op.i[L.RCV_I_COUT]
                    assert nbytes == 4 * op.i[L.RCV_I_NPART] * (2 * 16 + co * 16 + co) and op.i[L.RCV_I_NPART] >= 1
                elif flags & L.F_FUSED_CE:
                    assert nbytes == 4 * 3 * op.i[L.RCV_I_NPART] and op.i[L.RCV_I_NPART] >= 1
            for bad in (dict(aux1=6), dict(aux1=20), dict(aux1=0), dict(aux1=-4), dict(cout=9), dict(cout=0), dict(aux0=L.LOAD_NCHW),
                        dict(aux0=L.LOAD_GRAD_DEC), dict(cin=8), dict(cin=12), dict(cin=32), dict(n=0), dict(stats=L.STATS_FWD)):
                with pytest.raises(L.RcvError):
                    L.op_workspace(h, _rec(kind, flags, **bad))
                with pytest.raises(L.RcvError):
                    L.OpList([_rec(kind, flags, **bad)]).labels(h)
    for st in (L.STATS_NONE, L.STATS_FWD, L.STATS_BWD_ENC):          # the backward owes upConv3 its BatchNorm-backward sums
        with pytest.raises(L.RcvError, match="statistics kind"):
            L.op_workspace(h, _rec(L.OP_LP_TAIL_BWD, stats=st))
    for kind in (L.OP_LP_TAIL_FWD, L.OP_LP_TAIL_BWD):                 # the input is always formed from the block's stored tensors
        with pytest.raises(L.RcvError, match="RCV_F_FUSED_UP"):
            L.op_workspace(h, _rec(kind, L.F_FUSED_CE))
    # the classifier records keep their refusals: what they accepted before is all they accept
    with pytest.raises(L.RcvError, match="8 input channels only"):
        L.op_workspace(h, L.make_op(L.OP_CLS_BWD, L.F_FUSED_UP, n=2, h=8, w=8, cin=16, cout=5, stats=L.STATS_BWD_DEC))
    with pytest.raises(L.RcvError):
        L.op_workspace(h, L.make_op(L.OP_CLS_FWD, L.F_FUSED_UP | L.F_FUSED_CE, n=2, h=8, w=8, cin=16, cout=5, aux1=8))
    # the batch-assembly record
    L.op_workspace(h, L.make_op(L.OP_LP_BATCH, 0, n=8, cin=3, h=120, w=160, cout=5))
    for bad in (dict(cout=4), dict(cout=6), dict(n=0), dict(cin=0), dict(h=0), dict(n=40000, h=512, w=512)):
        kw = dict(n=8, cin=3, h=120, w=160, cout=5)
        kw.update(bad)
        with pytest.raises(L.RcvError):
            L.op_workspace(h, L.make_op(L.OP_LP_BATCH, 0, **kw))


# ------------------------------------------------------------------------------------------ the restatement against the reference
def test_restatement_of_the_batch_assembly_equals_the_fixture():
    for tag in R.SMALL:
        k = kats(tag)
        x, t = R.assemble_np(k[tag + "/images"], k[tag + "/labels"])
        assert np.array_equal(x, k[tag + "/x"]) and np.array_equal(t, k[tag + "/t"]) and x.dtype == np.float32
        P, H, W, seed = R.CONFIGS[tag]
        im, lab = R.synthetic_pairs(P, H, W, seed)
        assert np.array_equal(im.numpy(), k[tag + "/images"]) and np.array_equal(lab.numpy(), k[tag + "/labels"])
    x, _ = R.assemble_np(np.zeros((1, 2, 3, 2, 2), np.float32), np.array([[[[0, 5], [-1, 4]], [[7, 1], [2, -100]]]]))
    assert np.array_equal(x[0, 3:, 0, 0], [-1] * 5) and np.array_equal(x[1, 3:, 0, 1], [-1] * 5) and x[0, 4, 0, 1] == 1


def test_large_configuration_regenerates_from_its_seed():
    tag = "lp_16x120x160"
    m = META[tag]
    im, lab = R.synthetic_pairs(m["P"], m["H"], m["W"], m["seed"])
    assert abs(float(im.double().sum()) - m["images_sum"]) < 1e-6 and int(lab.sum()) == m["labels_sum"]
    x, _ = R.assemble_np(im.numpy(), lab.numpy())
    assert abs(float(x.astype(np.float64).sum()) - m["x_sum"]) < 1e-6


def test_restatement_of_the_tail_agrees_with_the_reference():
    tag = "lp_2x16x16"
    k = kats(tag)
    t, top = k[tag + "/tail/t"], k[tag + "/tail/top"]
    mean, var = k[tag + "/tail/mean"], k[tag + "/tail/var"]
    scale = k[tag + "/tail/bn_weight"].astype(np.float64) / np.sqrt(var + 1e-5)
    tc = np.stack([scale, k[tag + "/tail/bn_bias"] - mean * scale, mean])
    w, b = k[tag + "/tail/cls_weight"].reshape(5, 16), k[tag + "/tail/cls_bias"]
    v, logits = R.tail_forward_np(t, tc, top, w, b)
    assert np.abs(logits - k[tag + "/logits"]).max() <= 1e-5 * np.abs(k[tag + "/logits"]).max()
    loss, dl = R.ce_np(logits, k[tag + "/t"], R.LP_WEIGHTS)
    assert abs(loss - META[tag]["loss"]) <= 1e-6 * META[tag]["loss"]
    dW, db, g, gskip, stats = R.tail_backward_np(t, tc, v, w, dl, 8)
    gw, gb = k[tag + "/grad/classifier.weight"].reshape(5, 16), k[tag + "/grad/classifier.bias"]
    assert np.abs(dW - gw).max() <= 1e-5 * np.abs(gw).max() and np.abs(db - gb).max() <= 1e-5 * np.abs(gb).max()
    assert gskip.shape == (2, 16, 16, 8) and np.array_equal(gskip, g[..., :8])
    # the BatchNorm-backward sums are upConv3's affine gradients: d beta = sum g*m, d gamma = istd * sum g*m*(t - mean)
    dbeta, dgamma = k[tag + "/grad/upConv3.bn.bias"], k[tag + "/grad/upConv3.bn.weight"]
    assert np.abs(stats[0] - dbeta).max() <= 1e-4 * np.abs(dbeta).max()
    assert np.abs(stats[1] / np.sqrt(var + 1e-5) - dgamma).max() <= 1e-4 * np.abs(dgamma).max()


@pytest.mark.parametrize("rch", [4, 8, 12, 16])
@pytest.mark.parametrize("mode", [0, 1, 5])
def test_restatement_of_the_tail_equals_float64_autograd(rch, mode):
    """tail_forward_np / load_np / tail_backward_np at every skip width the launcher accepts, on a 2x5x7 plane, against torch float64
    autograd of  logits = W (cat(relu(t c0 + c1)[:rch] + f(r), relu(t c0 + c1)[rch:])) + b:  logits, dW, db, the gradient of the
    decoder output, the skip gradient, and the statistics rows as the gradients of the shift (row 0) and of the scale (row 1 + mean
    times row 0)."""
    rng = np.random.default_rng(100 * rch + mode)
    N, H, W, nC = 2, 5, 7, 5
    t, r = rng.standard_normal((N, H, W, 16)), rng.standard_normal((N, H, W, rch))
    tc, rc = rng.standard_normal((5, 16)), rng.standard_normal((5, rch))
    w, b, dl = rng.standard_normal((nC, 16)), rng.standard_normal(nC), rng.standard_normal((N, nC, H, W))
    top = R.load_np(r, rc, mode)
    v, logits = R.tail_forward_np(t, tc, top, w, b)
    dW, db, g, gskip, stats = R.tail_backward_np(t, tc, v, w, dl, rch)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    c0, c1 = T(tc[0]).requires_grad_(True), T(tc[1]).requires_grad_(True)
    wt, bt, rt = T(w).requires_grad_(True), T(b).requires_grad_(True), T(r)
    ft = rt if mode == 0 else rt * T(rc[0]) + T(rc[1])
    ft = (torch.relu(ft) if mode == 5 else ft).detach().requires_grad_(True)
    u = torch.relu(T(t) * c0 + c1)
    u.retain_grad()
    vt = torch.cat([u[..., :rch] + ft, u[..., rch:]], -1)
    lt = torch.einsum("nhwk,ck->nchw", vt, wt) + bt[None, :, None, None]
    (lt * T(dl)).sum().backward()
    near = lambda a, x: float(np.abs(a - x.detach().numpy()).max()) <= 1e-12 * max(1.0, float(x.detach().abs().max()))
    assert near(top, ft) and near(v, vt) and near(logits, lt)
    assert near(dW, wt.grad) and near(db, bt.grad) and near(g, u.grad) and near(gskip, ft.grad)
    assert gskip.shape == (N, H, W, rch) and np.array_equal(gskip, g[..., :rch])
    assert near(stats[0], c1.grad) and near(stats[1] + tc[2] * stats[0], c0.grad)


def test_exact_tail_cases_hold_their_preconditions():
    """The integer-grid cases of tests/test_gpu_labelprop_train.py, sized for 256 CUs here (on the device by rcv_num_cus): every class
    count, skip width and load mode on the small planes, every skip width on both planes beyond one grid pass; R.check_tail."""
    cases = R.tail_exact_cases(256)
    small = [k for k in cases if not k[4]]
    big = [k for k in cases if k[4]]
    assert {k[1:4] for k in small if k[0] == (2, 9, 11)} == {(nC, rch, m) for nC in (1, 5, 8) for rch in (4, 8, 12, 16) for m in (0, 1, 5)}
    assert {k[0] for k in small} == {(2, 9, 11), (1, 1, 1)} and len(big) == 8
    assert {(k[0], k[2]) for k in big} == {(pl, rch) for pl in [(1, 1025, 256), (3, 299, 293)] for rch in (4, 8, 12, 16)}
    assert {k[1] for k in big} == {1, 5, 8} and {k[3] for k in big} == {0, 1, 5}
    h = L.planner_handle(256)
    for plane, nC, rch, mode, second in cases:
        npix = plane[0] * plane[1] * plane[2]
        assert (second == 4 * 256 * 256 and npix > second) if second else npix <= 256
        op = _rec(L.OP_LP_TAIL_BWD, n=plane[0], h=plane[1], w=plane[2], cout=nC, aux0=mode, aux1=rch)
        L.op_workspace(h, op)
        assert op.i[L.RCV_I_NPART] == (1024 if second else 1)          # the capped grid: one pass is short of a big plane
        c = R.build_tail(plane, nC, rch, mode, second)
        full = R.check_tail(c)
        if plane == (2, 9, 11) or (rch, second) == (16, 4 * 256 * 256):
            # what check_tail's per-pixel terms stand for: the restatement without either pixel differs in EVERY reduced entry
            idx, masks = S.drop_masks(npix, second)
            assert idx == [npix - 1, second or npix // 2]
            for keep in masks:
                part = R.tail_reference(c, keep)
                assert all(np.all(full[j] != part[j]) for j in (1, 2, 5)) and np.array_equal(full[0], part[0])


def test_twin_equals_the_reference_at_init():
    """The plain-torch twin (the yardstick of the five-step GPU test and of the benchmark) has the reference's parameters, in its
    order, from the same seed, and its training step is the goldens' step."""
    tag = "lp_2x16x16"
    k = kats(tag)
    torch.manual_seed(12345678)
    twin = R.LabelPropTwin()
    assert sd_hash(twin.state_dict()) == META[tag]["sd_hash_init"]
    torch.manual_seed(12345678)
    assert sd_hash(M.LabelProp(5, 32).state_dict()) == META[tag]["sd_hash_init"]
    x, t = torch.from_numpy(k[tag + "/x"]), torch.from_numpy(k[tag + "/t"])
    twin.train()
    logits = twin(x)
    loss = torch.nn.CrossEntropyLoss(torch.tensor(R.LP_WEIGHTS))(logits, t)
    loss.backward()
    assert abs(float(loss.detach()) - META[tag]["loss"]) <= 1e-5 * META[tag]["loss"]
    for name, p in twin.named_parameters():
        ref = torch.from_numpy(k["%s/grad/%s" % (tag, name)])
        assert float((p.grad - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-7, name
    xx, tt = R.loop_assembly(torch.from_numpy(k[tag + "/images"]), torch.from_numpy(k[tag + "/labels"]))
    assert torch.equal(xx, x) and torch.equal(tt, t)


def test_near_tie_sets_respect_the_cap():
    for tag, (P, H, W, _) in R.CONFIGS.items():
        k = kats(tag)
        n = 2 * P * H * W
        near = np.unpackbits(k[tag + "/near_tie"])[:n]
        assert int(near.sum()) == META[tag]["near_ties"] <= max(1, int(R.NEAR_TIE_CAP * n))
        assert k[tag + "/argmax"].shape == (2 * P, H, W) and k[tag + "/argmax"].dtype == np.uint8
    for f in os.listdir(GOLDEN):
        if f.startswith("labelprop_train"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f


# ------------------------------------------------------------------------------------------ Python-level refusals
def test_python_level_refusals():
    assert robocupvision_amd.labelprop_batch is M.labelprop_batch
    im, lab = torch.zeros(2, 2, 3, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_class must be 5"):
        M.labelprop_batch(im, lab, num_class=4)
    with pytest.raises(TypeError):
        M.labelprop_batch(im.double(), lab)
    with pytest.raises(TypeError):
        M.labelprop_batch(im, lab.int())
    with pytest.raises(ValueError):
        M.labelprop_batch(im[:, :1], lab)
    with pytest.raises(ValueError):
        M.labelprop_batch(im, lab[:, :, :4])
    with pytest.raises(ValueError):
        M.labelprop_batch(im, lab[:1])
    with pytest.raises(L.RcvError, match="HIP device only"):
        M.labelprop_batch(im, lab)                                   # CPU tensors: there is no CPU path
    model = M.LabelProp(5, 32)
    with pytest.raises(L.RcvError, match="There is no CPU path"):    # (training mode no longer raises "inference only")
        model.train()(torch.zeros(2, 8, 16, 16).contiguous(memory_format=torch.channels_last))
    with pytest.raises(L.RcvError, match="reads its input as NHWC memory"):      # no hidden re-layout pass in the training step
        model.train()(torch.zeros(2, 8, 16, 16))
    with pytest.raises(L.RcvError, match="There is no CPU path"):    # eval mode takes any layout (and then meets the device check)
        model.eval()(torch.zeros(2, 8, 16, 16))
    model.train()
    with pytest.raises(ValueError, match="multiples of 8"):
        model(torch.zeros(2, 8, 12, 16))
    with pytest.raises(L.RcvError, match="requires_grad=False"):
        model(torch.zeros(2, 8, 16, 16, requires_grad=True).contiguous(memory_format=torch.channels_last))
    eng = model._get_engine()
    assert model._get_engine() is eng
    # a batch that leaves one value per channel at the bottom: torch's own refusal (the engine has the check)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _lower(model, (1, 8, 8, 8), training=True)


def test_distributed_labelprop_is_refused():
    with pytest.raises(L.RcvError, match="data-parallel training of LabelProp is not built"):
        Trainer(M.LabelProp(5, 32), class_weights=R.LP_WEIGHTS, optimizer=object(), distributed=True)
