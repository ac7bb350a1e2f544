"""CPU: the module surface of BNN-L / BNN-M-C (reference model.py:569-619), their restatement against the goldens, the float64
stage / head forms against torch's float64 autograd, plan-time refusals through the planner handle, PatchMetrics arithmetic."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnn_restatement as R
from conftest import GOLDEN, sd_hash
from robocupvision_amd import _lib as L

TAGS = ["bnnl_3x32x32", "bnnl_2x40x36", "bnnmc_3x32x32", "bnnmc_2x40x36"]


@pytest.fixture(scope="module")
def bnn_golden():
    with open(os.path.join(GOLDEN, "bnn.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "bnn.npz")), meta


def golden_masks(kats, tag, net):
    """The reference's keep masks as keep-scales in the restatement's layout: [N,C] x 3 (1/(1-p) in fp32), BNN-L's dof [N,512,h,w] (2)."""
    out = [torch.from_numpy(kats["%s/keep%d" % (tag, i)]).float() / torch.tensor(0.75) for i in range(3)]
    if net == "BNNL":
        out.append(torch.from_numpy(kats["%s/keep3" % tag]).float() * 2)
    return out


def golden_input(e):
    x = torch.randn(e["B"], 3, e["H"], e["W"], generator=torch.Generator().manual_seed(e["input_seed"]))
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest()[:16] == e["x_sha"]
    return x


def sample_index(numel, name, sample):
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    return torch.randperm(numel, generator=torch.Generator().manual_seed(seed))[:sample].sort()[0]


def golden_grad(kats, meta, tag, name, g):
    """(ours, golden) restricted to what the golden stores of this gradient."""
    key = "%s/grad/%s" % (tag, name)
    if key in kats.files:
        return g, torch.from_numpy(kats[key])
    idx = sample_index(g.numel(), name, meta["_sample"]["sample"])
    return g.reshape(-1)[idx], torch.from_numpy(kats["%s/grad_sample/%s" % (tag, name)])


@pytest.mark.parametrize("net", ["BNNL", "BNNMC"])
def test_modules_are_exported_with_the_reference_surface(net, bnn_golden):
    import robocupvision_amd.model as M
    kats, meta = bnn_golden
    assert net in M.__all__
    torch.manual_seed(12345678)
    m = getattr(M, net)()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == R.state_keys(net)
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in R.state_keys(net)]
    assert all(p.is_leaf and isinstance(p, torch.nn.Parameter) for p in m.parameters())
    children = ["conv1", "conv2", "conv3"] + (["fc"] if net == "BNNL" else []) + ["classifier", "relu", "pool1", "pool2", "pool3", "do1", "do2", "do3"] + \
        (["dof"] if net == "BNNL" else [])
    assert [k for k, _ in m.named_children()] == children
    tag = [t for t in TAGS if meta[t]["net"] == net][0]
    assert sd_hash(m.state_dict()) == meta[tag]["sd_hash_init"]
    with pytest.raises(L.RcvError, match="no CPU path"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(L.RcvError, match="training mode"):
        m.predict(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_goldens_bit_for_bit(tag, bnn_golden):
    import robocupvision_amd.model as M
    kats, meta = bnn_golden
    e = meta[tag]
    net = e["net"]
    prev = torch.get_num_threads()
    torch.set_num_threads(e["threads"])
    try:
        torch.manual_seed(12345678)
        sd = {k: v.clone() for k, v in getattr(M, net)().state_dict().items()}
        x = golden_input(e)
        masks = golden_masks(kats, tag, net)
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        logits = R.forward(net, params, x, masks)
        assert torch.equal(logits.detach(), torch.from_numpy(kats[tag + "/logits"]))
        t = torch.from_numpy(kats[tag + "/t"])
        loss = torch.nn.CrossEntropyLoss(torch.tensor(e["weights"]))(torch.squeeze(logits), t)
        assert float(loss.detach()) == e["loss"]
        loss.backward()
        for k, p in params.items():
            a, b = golden_grad(kats, meta, tag, k, p.grad)
            assert torch.equal(a, b), k
            assert float(p.grad.double().norm()) == pytest.approx(e["grad_norm"][k], rel=1e-12)
        losses, after = R.train_steps(net, sd, x, t, [masks])
        assert losses[0] == e["loss"]
        for k, v in after.items():
            assert float(v.double().sum()) == pytest.approx(e["param_after_step_sum"][k], rel=1e-12, abs=1e-12)
        with torch.no_grad():
            assert torch.equal(R.forward(net, after, x), torch.from_numpy(kats[tag + "/eval_logits"]))
        assert min(e["near_tie_ratios"].values()) >= e["margin"] == 8.0
    finally:
        torch.set_num_threads(prev)


def _autograd64(x, w, b, keep, pad, k, relu, dout):
    x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    cv = F.conv2d(x, w, b, padding=pad)
    if keep is not None:
        cv = cv * keep.reshape(keep.shape[0], keep.shape[1], 1, 1)
    if k:
        cv = F.max_pool2d(cv, k, 2)
    out = F.relu(cv) if relu else cv
    out.backward(dout)
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("ci", range(len(R.STAGE_CASES)))
def test_float64_stage_form_agrees_with_autograd_on_ties(ci):
    """Integer operands: every window is full of exact ties, pixels win several overlapping windows, all sums are exact -- the
    hand-written first-maximum backward must equal aten's bit for bit."""
    N, H, W, Cin, Cout, K, pad, k, drop = R.STAGE_CASES[ci]
    relu = k != 0
    x, w, b, keep, dout = R.exact_case(300 + ci, N, H, W, Cin, Cout, K, pad, k, drop)
    out, arg = R.stage_fwd64(x, w, b, keep, pad, k, relu)
    dx, dW, db, dconv = R.stage_bwd64(x, w, keep, pad, k, relu, out, arg, dout)
    o2, dx2, dW2, db2 = _autograd64(x, w, b, keep, pad, k, relu, dout)
    assert torch.equal(out, o2) and torch.equal(dx, dx2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    if k and out.numel() >= 200:                        # the case really has tied windows, and pixels that won more than one of them
        win = R._windows(F.conv2d(x, w, b, padding=pad) * (1 if keep is None else keep.reshape(N, Cout, 1, 1)), k)
        assert int(((win == win.max(-1, keepdim=True)[0]).sum(-1) > 1).sum()) > 0
        if k == 4:
            hits = torch.zeros_like(dconv)
            for j in range(16):
                hits[:, :, j // 4:j // 4 + 2 * out.shape[2]:2, j % 4:j % 4 + 2 * out.shape[3]:2][:, :, :out.shape[2], :out.shape[3]] += (arg == j).double()
            assert float(hits.max()) >= 2


@pytest.mark.parametrize("ci", sorted(R.NORMAL_CASES))
def test_float64_stage_form_agrees_with_autograd_on_normal_operands_and_the_seed_has_few_near_ties(ci):
    N, H, W, Cin, Cout, K, pad, k, drop = R.STAGE_CASES[ci]
    x, w, b, keep, dout = [None if v is None else v.double() for v in R.normal_case(R.NORMAL_CASES[ci], N, H, W, Cin, Cout, K, pad, k, drop)]
    out, arg = R.stage_fwd64(x, w, b, keep, pad, k, True)
    dx, dW, db, _ = R.stage_bwd64(x, w, keep, pad, k, True, out, arg, dout)
    o2, dx2, dW2, db2 = _autograd64(x, w, b, keep, pad, k, True, dout)
    for a, c in ((out, o2), (dx, dx2), (dW, dW2), (db, db2)):
        assert float((a - c).abs().max()) <= 1e-12 * float(c.abs().max())
    near = R.near_tie_windows(x, w, b, keep, pad, k)
    assert int(near.sum()) < 1e-3 * near.numel()


@pytest.mark.parametrize("keep_on", [False, True])
def test_float64_head_form_agrees_with_autograd(keep_on):
    g = torch.Generator().manual_seed(5)
    M_ = 6
    x = torch.randn(M_, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    wfc = torch.randn(512, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    bfc = torch.randn(512, generator=g, dtype=torch.float64).requires_grad_(True)
    wc = torch.randn(4, 512, generator=g, dtype=torch.float64).requires_grad_(True)
    bc = torch.randn(4, generator=g, dtype=torch.float64).requires_grad_(True)
    keep = (torch.randint(0, 2, (M_, 512), generator=g).double() * 2) if keep_on else None
    dl = torch.randn(M_, 4, generator=g, dtype=torch.float64)
    z = F.linear(x, wfc, bfc)
    logits = F.linear(F.relu(z if keep is None else z * keep), wc, bc)
    logits.backward(dl)
    with torch.no_grad():
        l2, z2 = R.head_fwd64(x, wfc, bfc, keep, wc, bc)
        got = R.head_bwd64(x, wfc, keep, wc, z2, dl)
    assert float((l2 - logits.detach()).abs().max()) < 1e-12
    for a, c in zip(got, (x.grad, wfc.grad, bfc.grad, wc.grad, bc.grad)):
        assert float((a - c).abs().max()) <= 1e-12 * float(c.abs().max())


def test_planner_refuses_what_the_launch_would_refuse():
    import robocupvision_amd.model as M
    h = L.planner_handle(256)
    mc, bl = M.BNNMC(), M.BNNL()
    with pytest.raises(L.RcvError, match="rcv_op_workspace.*bnn stage forward: a 2x3 plane is too small for a 3x3 filter"):
        mc._plan_records(2, 3, 31, 32, h)
    fwd, bwd = mc._plan_records(2, 3, 32, 32, h)
    assert len(fwd) == 4 and len(bwd) == 4 and fwd[-1].i[L.RCV_I_HO] == 1 and fwd[-1].i[L.RCV_I_WO] == 1
    fwd, bwd = bl._plan_records(2, 3, 30, 30, h)          # BNN-L accepts 30x30
    assert len(fwd) == 4 and len(bwd) == 4 and (fwd[2].i[L.RCV_I_HO], fwd[2].i[L.RCV_I_WO]) == (1, 1)
    with pytest.raises(L.RcvError, match="too small"):
        bl._plan_records(2, 3, 20, 32, h)
    for m in (mc, bl):
        with pytest.raises(L.RcvError, match="2 input channels unsupported"):
            m._plan_records(2, 2, 32, 32, h)
        fwd, _ = m._plan_records(1, 3, 256, 256, h)
        assert fwd[0].i[L.RCV_I_H] == 256
    base = dict(n=2, h=15, w=15, cin=8, cout=16, ho=6, wo=6, aux0=8, aux1=4, count=3, inmode=L.LOAD_PLAIN)
    for kind, what in ((L.OP_BNN_STAGE_FWD, "forward"), (L.OP_BNN_STAGE_BWD, "backward")):
        ok = L.make_op(kind, L.F_RELU, **base)
        nbytes = L.op_workspace(h, ok)
        assert (nbytes > 0) == (kind == L.OP_BNN_STAGE_BWD)
        assert L.OpList([ok]).labels(h)[0].startswith("bnn_stage_%s<8,4," % ("fwd" if what == "forward" else "bwd"))
        for change, msg in ((dict(aux0=7), "filter size 7 unsupported"), (dict(aux1=3), "pool size 3 unsupported"),
                            (dict(cin=2), "2 input channels unsupported"), (dict(cout=5), "5 output channels unsupported"),
                            (dict(count=2), "padding 2 unsupported"), (dict(ho=7), "output plane 7x6 given, 6x6 expected"),
                            (dict(h=4), "too small")):
            bad = L.make_op(kind, L.F_RELU, **dict(base, **change))
            with pytest.raises(L.RcvError, match="bnn stage %s: .*%s" % (what, msg)):
                L.op_workspace(h, bad)
            with pytest.raises(L.RcvError, match="planning-only|%s" % msg):       # the launch path: the planner cannot enqueue at all
                L.OpList([bad]).run(h, 0)
    for kind in (L.OP_BNN_HEAD_FWD, L.OP_BNN_HEAD_BWD):
        L.op_workspace(h, L.make_op(kind, 0, n=3, h=1, w=1, cin=16, cout=4, count=512))
        for change, msg in ((dict(cin=8), "8 input channels unsupported"), (dict(count=256), "256 hidden units unsupported"),
                            (dict(cout=9), "9 classes unsupported")):
            with pytest.raises(L.RcvError, match=msg):
                L.op_workspace(h, L.make_op(kind, 0, **dict(dict(n=3, h=1, w=1, cin=16, cout=4, count=512), **change)))


def test_an_imposed_dropout_list_of_the_wrong_shape_is_refused():
    import robocupvision_amd.model as M
    bl, mc = M.BNNL(), M.BNNMC()
    good = [torch.ones(3, 8), torch.ones(3, 16), torch.ones(3, 16), torch.ones(3, 1, 1, 512)]
    bl._impose_dropout(good)
    bl._impose_dropout(None)
    mc._impose_dropout(good[:3])
    for bad in (good[:3], [torch.ones(3, 8), torch.ones(3, 8), torch.ones(3, 16), torch.ones(3, 1, 1, 512)],
                good[:3] + [torch.ones(3, 512, 1, 1)], good[:3] + [torch.ones(2, 1, 1, 512)]):
        with pytest.raises(L.RcvError, match="keep-scales"):
            bl._impose_dropout(bad)
    with pytest.raises(L.RcvError, match="keep-scales"):
        mc._impose_dropout(good)
    assert bl._last_dropout_scales() is None


def test_patch_metrics_arithmetic_against_the_reference_loop():
    from robocupvision_amd.metrics import PatchMetrics, patch_scores
    g = torch.Generator().manual_seed(9)
    pred = torch.randint(0, 4, (200,), generator=g)
    lab = torch.randint(0, 4, (200,), generator=g)
    conf = torch.zeros(4, 4).long()
    for j in range(200):                                   # objDetEval.py:128-129
        conf[(pred[j], lab[j])] += 1
    running_acc = torch.sum(pred == lab).item() * 100      # objDetEval.py:156
    total = torch.sum(conf[:, 1:4]).item()                 # objDetEval.py:171-179
    totAcc = conf[1, 1] + conf[2, 2] + conf[3, 3]
    fp = torch.sum(conf[1:4, :]).item() - totAcc
    want = {"acc": running_acc / 200, "obj_acc": float(totAcc / total * 100), "false_neg": float(100 - totAcc / total * 100),
            "false_pos": float(fp / total * 100)}
    got = patch_scores(conf)
    pm = PatchMetrics(4, device="cpu")
    pm.conf = conf.clone()
    for res in (got, pm.compute()):
        for k, v in want.items():      # the reference divides an int64 TENSOR by a Python int: its three figures are fp32 (2^-23 per operation)
            assert res[k] == pytest.approx(v, rel=1e-12 if k == "acc" else 1e-6), k
        assert torch.equal(res["confusion"], conf)
    with pytest.raises(L.RcvError):
        pm.update(pred.to(torch.uint8), lab)               # no CPU path
