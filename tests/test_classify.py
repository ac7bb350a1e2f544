"""The patch-classification stage (classTrainer.py:83,118-140): PB_FCN(classify=1) and PB_FCN_2(classify=True) train through the
pooled head (RCV_OP_POOL_CLS_FWD / _BWD, csrc/pool_cls.hip).  Goldens: ``tests/golden/classify.{npz,json}`` from the imported
reference (``make_golden_classify.py``).

  * CPU: both classify models plan in training and eval mode through the planner handle; the graph reads exactly the parameters the
    reference's autograd reaches; init and state_dict keys match the reference; unsupported heads are refused when the plan is built;
  * GPU: the whole classTrainer.py step against the goldens, the dropout draw, the classify -> segmentation checkpoint hand-over
    (trainer.py:149-151) and a 5-step trajectory against a torch-CPU twin on the box."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, sd_hash
from oracle import cpu_reference as O
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd.engine import Engine

DEV = "cuda:0"
TAGS = ["pb_c5_8x32x32", "pb_c3_8x32x32", "pbl_c5_8x32x32", "pb_c5_4x48x64", "pb2_c5_8x32x32", "pb2_c5_2x120x160"]


@pytest.fixture(scope="module")
def cl_kats():
    return np.load(os.path.join(GOLDEN, "classify.npz"))


@pytest.fixture(scope="module")
def cl_meta():
    with open(os.path.join(GOLDEN, "classify.json")) as f:
        return json.load(f)


def _t(a):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(a.shape)


def _make(m):
    return M.PB_FCN_2(True, nClass=m["nC"]) if m["v2"] else M.PB_FCN(32, m["nC"], 1, m["noScale"], 1)


def _input(m):
    """make_golden_classify.make_input, checked against the stored hash."""
    x = torch.randn(m["B"], 3, m["H"], m["W"], generator=torch.Generator().manual_seed(3))
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest()[:16] == m["x_sha"], "the seeded input differs from the golden's"
    return x


def _sample_index(numel, name, n):
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    return torch.randperm(numel, generator=torch.Generator().manual_seed(seed))[:n].sort()[0]


def _lower(model, shape, training=True):
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    plan = eng._plan_for([torch.zeros(shape)], training)
    return eng, plan


def _unread(model, v2):
    prefixes = ("segmenter.", "upPart.") if v2 else ("segmenter.", "up")
    return sorted(n for n, _ in model.named_parameters() if n.startswith(prefixes))


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("training", [True, False])
def test_classify_models_plan(cl_meta, tag, training):
    m = cl_meta[tag]
    model = _make(m)
    eng, plan = _lower(model, (m["B"], 3, m["H"], m["W"]), training)
    assert tuple(plan.logits.shape) == tuple(m["logits_shape"])
    lists = [plan.fwd] + ([plan.bwd] if training else [])
    for lst in lists:
        labels = lst.labels(eng.handle)
        for k in range(lst.n):           # every record answers its query again, as it stands
            op = L.RcvOp.from_buffer_copy(lst.arr[k])
            L.op_workspace(eng.handle, op)
        assert any(s.startswith("pool_cls_fwd<" if lst is plan.fwd else "pool_cls_bwd<") for s in labels), labels
    fwd = plan.fwd.labels(eng.handle)
    pool = "avg" if m["v2"] else ("max2" if m["noScale"] else "max4")
    assert [s for s in fwd if s.startswith("pool_cls")] == ["pool_cls_fwd<%s,%s>" % (pool, (
        "affine" if m["v2"] else ("affine_relu" if training else "plain")))]
    if training:
        # the producer's BatchNorm backward: PB_FCN_2's Conv = bn(relu(conv)) (encoder sums), PB_FCN's ConvPoolSimple = relu(bn(conv))
        bwd = [s for s in plan.bwd.labels(eng.handle) if s.startswith("pool_cls")]
        assert bwd == ["pool_cls_bwd<%s,%s,%s>" % (pool, "affine" if m["v2"] else "affine_relu", "enc" if m["v2"] else "dec")]
        assert plan.dropout is not None if m["v2"] else plan.dropout is None
    else:
        assert plan.dropout is None and plan.bwd.n == 0


@pytest.mark.parametrize("tag", TAGS)
def test_graph_reads_what_the_reference_autograd_reaches(cl_meta, tag):
    m = cl_meta[tag]
    model = _make(m)
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    unread = sorted(n for (n, _), used in zip(model.named_parameters(), eng.param_used) if not used)
    assert unread == _unread(model, m["v2"]) == sorted(m["none_grads"])


@pytest.mark.parametrize("tag", TAGS)
def test_init_matches_the_reference(cl_meta, tag):
    m = cl_meta[tag]
    torch.manual_seed(12345678)
    assert sd_hash(_make(m).state_dict()) == m["sd_hash_init"]


@pytest.mark.parametrize("make_cls,make_seg", [
    (lambda: M.PB_FCN(32, 5, 1, False, 1), lambda: M.PB_FCN(32, 5, 1, False, 0)),
    (lambda: M.PB_FCN(32, 5, 1, True, 1), lambda: M.PB_FCN(32, 5, 1, True, 0)),
    (lambda: M.PB_FCN_2(True), lambda: M.PB_FCN_2(False))])
def test_state_dict_keys_are_those_of_the_segmentation_mode(make_cls, make_seg):
    torch.manual_seed(12345678)
    a = make_cls()
    torch.manual_seed(12345678)
    b = make_seg()
    assert list(a.state_dict()) == list(b.state_dict())
    assert sd_hash(a.state_dict()) == sd_hash(b.state_dict())        # same init draws in both modes
    b.load_state_dict(a.state_dict())                                 # trainer.py:149-151


def test_unsupported_heads_are_refused_when_the_plan_is_built():
    with pytest.raises(L.RcvError, match="1x1"):
        _lower(M.PB_FCN(32, 5, 3, False, 1), (2, 3, 32, 32))
    with pytest.raises(L.RcvError, match="classes"):
        _lower(M.PB_FCN(32, 9, 1, False, 1), (2, 3, 32, 32))
    with pytest.raises(L.RcvError, match="classes"):
        _lower(M.PB_FCN_2(True, nClass=9), (2, 3, 32, 32))
    with pytest.raises(ValueError, match="empty"):
        _lower(M.PB_FCN(32, 5, 1, True, 1), (2, 3, 16, 16))          # f4 is 1x1: MaxPool2d(2) leaves nothing


def _rec(kind, **kw):
    base = dict(n=2, h=8, w=8, cin=64, cout=5, ho=2, wo=2, aux0=4, inmode=L.LOAD_AFFINE_RELU)
    base.update(kw)
    flags = base.pop("flags", 0)
    return L.make_op(kind, flags, **base)


def test_the_query_refuses_what_the_launch_would_refuse():
    h = L.planner_handle(256)
    for kind in (L.OP_POOL_CLS_FWD, L.OP_POOL_CLS_BWD):
        L.op_workspace(h, _rec(kind))
        L.op_workspace(h, _rec(kind, cin=512, cout=8, aux0=0, ho=1, wo=1, inmode=L.LOAD_AFFINE))
        L.op_workspace(h, _rec(kind, cout=1, h=9, w=11, aux0=2, ho=4, wo=5, inmode=L.LOAD_PLAIN))
        for bad in (dict(cin=62), dict(cin=516), dict(cin=0), dict(cout=9), dict(cout=0), dict(aux0=3), dict(aux0=8),
                    dict(inmode=L.LOAD_GRAD_ENC), dict(inmode=L.LOAD_NCHW), dict(ho=1), dict(h=3, w=3, ho=0, wo=0),
                    dict(flags=L.F_BIAS), dict(flags=L.F_RELU)):
            with pytest.raises(L.RcvError):
                L.op_workspace(h, _rec(kind, **bad))
            with pytest.raises(L.RcvError):
                L.OpList([_rec(kind, **bad)]).labels(h)
    with pytest.raises(L.RcvError):
        L.op_workspace(h, _rec(L.OP_POOL_CLS_FWD, flags=L.F_RESID))       # the skip gradient belongs to the backward
    for st in (L.STATS_FWD, 7):
        with pytest.raises(L.RcvError):
            L.op_workspace(h, _rec(L.OP_POOL_CLS_BWD, stats=st))
    # workspace: partial rows of the statistics, then d loss / d pooled
    op = _rec(L.OP_POOL_CLS_BWD, stats=L.STATS_BWD_DEC, flags=L.F_RESID)
    nbytes = L.op_workspace(h, op)
    assert op.i[L.RCV_I_NPART] >= 1 and nbytes == 4 * (op.i[L.RCV_I_NPART] * 2 * 64 + 2 * 2 * 2 * 64)
    op = _rec(L.OP_POOL_CLS_BWD)
    assert L.op_workspace(h, op) == 4 * 8 * 64 and op.i[L.RCV_I_NPART] == 0


def test_heads_called_on_their_own_still_raise():
    with pytest.raises(L.RcvError):
        M.Classifier(64, 5, poolSize=4)(torch.zeros(1, 64, 4, 4))
    with pytest.raises(L.RcvError):
        M.UltClassifier(64, 5, True)(torch.zeros(1, 64, 4, 4))


@pytest.mark.parametrize("make", [lambda c: M.PB_FCN(32, 5, 1, False, c), lambda c: M.PB_FCN_2(c)])
def test_a_change_of_classify_reaches_the_next_forward(make):
    model = make(1)
    assert model._get_engine().graph["nodes"][-1]["op"] == "pool_cls"
    model.classify = 0
    assert model._get_engine().graph["nodes"][-1]["op"] == "cls"
    model.classify = True
    eng = model._get_engine()
    assert eng.graph["nodes"][-1]["op"] == "pool_cls" and model._get_engine() is eng


# ------------------------------------------------------------------------------------------ GPU
def _close(a, b, what, rtol=1e-3, floor=1e-2):
    from test_gpu_blocks import close
    close(a, b, what, rtol=rtol, floor=floor)


def _rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cls_step(model, x, t, weights, opt, keep=None):
    """classTrainer.py:118-131: forward, squeeze, stock CrossEntropyLoss(weights), backward, optimizer step."""
    crit = torch.nn.CrossEntropyLoss(torch.tensor(weights, dtype=torch.float32, device=x.device))
    model.train()
    if keep is not None:
        model._get_engine()._impose_dropout(keep)
    opt.zero_grad()
    logits = model(x)
    pred = torch.squeeze(logits)
    loss = crit(pred, t)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    opt.step()
    return logits.detach().clone(), pred.detach(), float(loss.detach()), grads


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_gpu_classify_step_vs_golden(cl_kats, cl_meta, tag):
    from test_gpu_net import check_mask
    from test_gpu_pbfcn import _check_after
    m = cl_meta[tag]
    torch.manual_seed(12345678)
    model = _make(m)
    assert sd_hash(model.state_dict()) == m["sd_hash_init"]
    model = model.to(DEV)
    x, t = _input(m).to(DEV), _t(cl_kats[tag + "/t"]).to(DEV)
    keep = None
    if m["v2"]:
        keep = _t(cl_kats[tag + "/drop_keep"]).float() / (1.0 - m["dropout_p"])
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-1, momentum=0.5, weight_decay=1e-3)
    logits, pred, loss, grads = _cls_step(model, x, t, m["weights"], opt, keep)
    if keep is not None:
        assert torch.equal(model._get_engine()._last_dropout_scale().cpu(), keep)
        model._get_engine()._impose_dropout(None)
    _close(logits, _t(cl_kats[tag + "/logits"]), tag + " logits")
    check_mask(torch.max(pred, 1)[1], cl_kats[tag + "/argmax"], cl_kats[tag + "/near_tie_idx"], tag)
    assert abs(loss - m["loss"]) <= 1e-4 * abs(m["loss"]), (loss, m["loss"])
    assert sorted(k for k, g in grads.items() if g is None) == m["none_grads"]
    for k, g in grads.items():
        if g is None:
            continue
        n_ref = m["grad_norm"][k]
        if (tag + "/grad/" + k) in cl_kats.files:
            rel = _rel_l2(g, _t(cl_kats[tag + "/grad/" + k]))
        else:
            ref = _t(cl_kats[tag + "/grad_sample/" + k])
            rel = _rel_l2(g.reshape(-1).cpu()[_sample_index(g.numel(), k, ref.numel())], ref)
            assert abs(float(g.double().norm()) - n_ref) <= 5e-3 * n_ref + 1e-12, (k, float(g.double().norm()), n_ref)
        assert rel <= 5e-3 or n_ref < 1e-7, "%s grad %s: relative L2 error %.3e" % (tag, k, rel)
    sd = model.state_dict()
    for k in cl_kats.files:
        if k.startswith(tag + "/after/"):
            _close(sd[k[len(tag) + 7:]], _t(cl_kats[k]), k)
    _check_after(sd, m["param_after_step_sum"], 0.1)
    model.eval()
    with torch.no_grad():
        pe = model(x)
    _close(pe, _t(cl_kats[tag + "/eval_logits"]), tag + " eval logits")


def _pb2_twin_logits(sd, x, keep_scale):
    """torch-CPU restatement of PB_FCN_2(classify=True) (model.py:444-453) with a given Dropout2d keep-scale (None: eval)."""
    training = keep_scale is not None
    v = O.level_down(x, sd, "downPart.Level0", 1, False, False, training)
    for i in range(3):
        v = O.level_down(v, sd, "downPart.Level%d" % (i + 1), 2, True, False, training)
    v = O.level_down(v, sd, "PB.PB_1", 4, False, False, training)
    v = O.level_down(v, sd, "PB.PB_2", 1, False, False, training)
    v = F.adaptive_avg_pool2d(v, 1)
    if training:
        v = v * keep_scale.reshape(v.shape)
    return F.conv2d(v, sd["classifier.layers.Class.weight"], sd["classifier.layers.Class.bias"])


@pytest.mark.gpu
def test_gpu_dropout_draw():
    torch.manual_seed(12345678)
    model = M.PB_FCN_2(True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    eng = model._get_engine()
    x = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(11))
    xd = x.to(DEV)
    torch.manual_seed(5)
    with torch.no_grad():
        y1 = model(xd).clone()
    s1 = eng._last_dropout_scale().cpu()
    assert tuple(s1.shape) == (64, 64) and set(torch.unique(s1).tolist()) <= {0.0, 2.0}
    # the module's logits are those of a torch-CPU restatement fed the mask it drew
    _close(y1, _pb2_twin_logits({k: v.clone() for k, v in sd.items()}, x, s1), "logits with the drawn mask")
    # torch.manual_seed governs the draw: the same seed gives the same mask
    torch.manual_seed(5)
    with torch.no_grad():
        model(xd)
    assert torch.equal(eng._last_dropout_scale().cpu(), s1)
    with torch.no_grad():
        model(xd)
    assert not torch.equal(eng._last_dropout_scale().cpu(), s1)
    # kept fraction: 64 x 64 Bernoulli(1 - p) draws
    kept = float((s1 != 0).double().mean())
    sigma = (0.5 * 0.5 / s1.numel()) ** 0.5
    assert abs(kept - 0.5) <= 4 * sigma, kept
    # eval mode drops nothing
    model.eval()
    with torch.no_grad():
        ye = model(xd)
    assert eng._last_dropout_scale() is None
    sd_now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    _close(ye, _pb2_twin_logits(sd_now, x, None), "eval logits")


@pytest.mark.gpu
def test_gpu_classify_checkpoint_starts_the_segmentation_stage(tmp_path):
    """classTrainer.py saves bestModel*.pth; trainer.py:149-151 loads it into the segmentation net and trains on."""
    torch.manual_seed(12345678)
    cls = M.PB_FCN(32, 5, 1, False, 1).to(DEV)
    opt = torch.optim.SGD([{"params": cls.parameters()}], lr=1e-2, momentum=0.9, weight_decay=1e-5)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        x = torch.randn(16, 3, 32, 32, generator=g).to(DEV)
        t = torch.randint(0, 5, (16,), generator=g).to(DEV)
        _, _, loss, _ = _cls_step(cls, x, t, [1.0] * 5, opt)
        assert np.isfinite(loss)
    path = str(tmp_path / "bestModel.pth")
    torch.save(cls.state_dict(), path)
    seg = M.PB_FCN(32, 5, 1, False, 0)
    seg.load_state_dict(torch.load(path, map_location="cpu"))
    seg = seg.to(DEV)
    for k, v in cls.state_dict().items():
        if k.startswith("FCN."):
            assert torch.equal(seg.state_dict()[k], v), k
    from test_gpu_pbfcn import pb_step
    xs, ts = O.synthetic_batch(2, 48, 64)
    res = pb_step(seg, xs.to(DEV), ts.to(DEV))
    assert np.isfinite(res["loss"]) and bool(torch.isfinite(res["pred"]).all())
    assert all(bool(torch.isfinite(gr).all()) for gr in res["grads"].values() if gr is not None)


def _pb_twin_f3(sd, x):
    v = O._cps(x, sd, "FCN.conv0", 1, 2, 2, True)
    v = O._cps(v, sd, "FCN.conv1", 2, 1, 1, True)
    v = O.conv_pool(v, sd, "FCN.conv2", True)
    v = O.conv_pool(v, sd, "FCN.conv3", True)
    for name in ("conv4", "conv5", "conv6", "conv7", "conv8"):
        v = O._cps(v, sd, "FCN." + name, 1, 2, 2, True)
    return v


def _pb_twin_logits(sd, x):
    """torch-CPU restatement of PB_FCN(classify=1) without noScale (model.py:221-229, 294-298) from the oracle's pieces."""
    v = F.max_pool2d(_pb_twin_f3(sd, x), 4)
    return F.conv2d(v, sd["classifier.classifier.weight"], sd["classifier.classifier.bias"])


def _near_tie(sd, x, rel=2e-6):
    """True when the float64 forward of the twin puts a pre-ReLU value of the small planes (10x10 and below), or the top two values of a
    pooled window, within rel * (the tensor's standard deviation) of a tie: there fp32 rounding alone decides a ReLU mask or an
    arg-max, and the gradients of two correct fp32 implementations differ by a whole element's share (on the 5x5 plane: several 1e-3
    of a BatchNorm gradient; measured: one such value at 1e-6 sigma moves conv3.bn.bias by 5e-3)."""
    sd64 = {k: (v.detach().double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    hits, relu = [], F.relu

    def spy(z, *a, **k):
        if z.shape[-2] * z.shape[-1] <= 100:
            hits.append(bool((z.abs() < rel * float(z.std())).any()))
        return relu(z, *a, **k)
    F.relu = spy
    try:
        f3 = _pb_twin_f3(sd64, x.double())
    finally:
        F.relu = relu
    win = f3[:, :, :4, :4].reshape(f3.shape[0], f3.shape[1], 16)
    top = torch.topk(win, 2, dim=2)[0]
    gap = top[:, :, 0] - top[:, :, 1]
    return any(hits) or bool(((gap < rel * float(f3.std())) & (top[:, :, 0] > 0)).any())


@pytest.mark.gpu
def test_gpu_classify_trajectory_vs_cpu_twin():
    torch.manual_seed(12345678)
    model = M.PB_FCN(32, 5, 1, False, 1)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in model.named_parameters()]
    used = [n for n in names if n.startswith(("FCN.", "classifier."))]
    for n in used:
        sd[n].requires_grad_(True)
    topt = torch.optim.SGD([{"params": [sd[n] for n in used]}], lr=1e-2, momentum=0.9, weight_decay=1e-5)
    model = model.to(DEV)
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-2, momentum=0.9, weight_decay=1e-5)
    w = [1.0, 2.0, 0.5, 3.0, 1.5]
    g = torch.Generator().manual_seed(9)
    for step in range(5):
        for _ in range(20):          # (batches on a fp32 knife edge of the current parameters are redrawn, see _near_tie)
            x = torch.randn(12, 3, 40, 40, generator=g)          # 40x40: f3 is 5x5, the last row and column lie outside the 4x4 window
            t = torch.randint(0, 5, (12,), generator=g)
            if not _near_tie(sd, x):
                break
        else:
            pytest.fail("no batch without a near tie in 20 draws")
        topt.zero_grad()
        ref = _pb_twin_logits(sd, x)
        rloss = torch.nn.CrossEntropyLoss(torch.tensor(w))(torch.squeeze(ref), t)
        rloss.backward()
        logits, _, loss, grads = _cls_step(model, x.to(DEV), t.to(DEV), w, opt)
        _close(logits, ref.detach(), "step %d logits vs twin" % step)
        assert abs(loss - float(rloss)) <= 1e-3 * abs(float(rloss)), (step, loss, float(rloss))
        for n in names:
            if n not in used:
                assert grads[n] is None, n
                continue
            rel = _rel_l2(grads[n], sd[n].grad)
            assert rel <= 5e-3, "step %d grad %s vs twin: relative L2 error %.3e" % (step, n, rel)
        topt.step()


def test_an_imposed_dropout_mask_must_fit_the_plan():
    model = M.PB_FCN_2(True)
    eng, plan = _lower(model, (4, 3, 32, 32))
    eng._impose_dropout(torch.full((4, 64), 2.0))
    eng._fill_dropout(plan)
    assert torch.equal(plan.dropout[0], torch.full((4, 64), 2.0))
    eng._impose_dropout(torch.ones(8, 64))
    with pytest.raises(L.RcvError, match="imposed dropout"):
        eng._fill_dropout(plan)
