"""GPU: the BNN-L / BNN-M-C kernels (csrc/bnn.hip) through the C ABI, one record per test where possible, against the float64
restatement (tests/bnn_restatement.py); then whole training steps of the modules against the reference's goldens (tests/golden/bnn.npz),
determinism, dropout, a short trajectory against the CPU restatement, ``predict`` and ``PatchMetrics``."""
import math

import numpy as np
import pytest
import torch

import bnn_restatement as R
from robocupvision_amd import _lib as L
from test_bnn import TAGS, bnn_golden, golden_grad, golden_input, golden_masks      # noqa: F401  (bnn_golden is a fixture)
from test_gpu_blocks import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t, dtype=torch.float32):
    return t.detach().to(dtype).contiguous().to(DEV)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _run_stage(case, x, w, b, keep, dout, with_arg=True):
    """One forward record and one backward record (run twice) on fp32 copies of the operands.  Activations are handed over as the
    network would: the 3-channel case NCHW, the others NHWC; the pool-less classifier case writes / reads NCHW logits."""
    N, H, W, Cin, Cout, K, pad, k, drop = case
    relu, nchw_in, nchw_out = k != 0, Cin == 3, k == 0
    Hc, Wc = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    Ho, Wo = ((Hc - k) // 2 + 1, (Wc - k) // 2 + 1) if k else (Hc, Wc)
    h = L.handle(0)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    x_d = _dev(x if nchw_in else _nhwc(x))
    w_d, b_d = _dev(w), _dev(b)
    keep_d = _dev(keep) if keep is not None else None
    out_d = torch.full((N, Cout, Ho, Wo) if nchw_out else (N, Ho, Wo, Cout), 7.0, device=DEV)
    arg_d = torch.full((N, Ho, Wo, Cout), 99, dtype=torch.uint8, device=DEV) if k else None
    flags = (L.F_RELU if relu else 0) | (L.F_OUT_NCHW if nchw_out else 0)
    common = dict(n=N, h=H, w=W, cin=Cin, cout=Cout, ho=Ho, wo=Wo, aux0=K, aux1=k, count=pad, inmode=L.LOAD_NCHW if nchw_in else L.LOAD_PLAIN,
                  p_w=w_d.data_ptr(), p_x0=(keep_d.data_ptr() if keep_d is not None else 0), p_x1=(arg_d.data_ptr() if arg_d is not None else 0))
    fop = L.make_op(L.OP_BNN_STAGE_FWD, flags, p_in=x_d.data_ptr(), p_bias=b_d.data_ptr(), p_out=out_d.data_ptr(), **common)
    assert L.op_workspace(h, fop) == 0 and L.OpList([fop]).labels(h)[0].startswith("bnn_stage_fwd<%d,%d," % (K, k))
    L.OpList([fop]).run(h, stream)
    torch.cuda.synchronize()
    dout_d = _dev(dout if nchw_out else _nhwc(dout))
    dx_d = None if nchw_in else torch.full((N, H, W, Cin), 7.0, device=DEV)
    dw_d, db_d = torch.full_like(w_d, 7.0), torch.full_like(b_d, 7.0)
    bop = L.make_op(L.OP_BNN_STAGE_BWD, flags, p_in=dout_d.data_ptr(), p_in_aux=out_d.data_ptr(), p_epi_aux=x_d.data_ptr(),
                    p_out=(dx_d.data_ptr() if dx_d is not None else 0), p_x2=dw_d.data_ptr(), p_x3=db_d.data_ptr(), **common)
    nbytes = L.op_workspace(h, bop)
    rows = bop.i[L.RCV_I_NPART]
    assert nbytes == 4 * rows * (Cout * Cin * K * K + Cout) and rows >= N
    part_d = torch.zeros(nbytes // 4, device=DEV)
    bop.p[L.RCV_P_PART] = part_d.data_ptr()
    assert L.OpList([bop]).labels(h)[0].startswith("bnn_stage_bwd<%d,%d," % (K, k))
    runs = []
    for _ in range(2):
        for t in (dx_d, dw_d, db_d, part_d):
            if t is not None:
                t.fill_(7.0)
        L.OpList([bop]).run(h, stream)
        torch.cuda.synchronize()
        runs.append([None if t is None else t.cpu().clone() for t in (dx_d, dw_d, db_d)])
    for a, c in zip(*runs):
        assert a is None or torch.equal(a, c), "two backward runs differ"
    out = out_d.cpu() if nchw_out else out_d.cpu().permute(0, 3, 1, 2)
    arg = arg_d.cpu().permute(0, 3, 1, 2) if k else None
    dx = None if dx_d is None else runs[0][0].permute(0, 3, 1, 2)
    return out, arg, dx, runs[0][1], runs[0][2], rows


@pytest.mark.parametrize("ci", range(len(R.STAGE_CASES)))
def test_stage_kernels_exact_on_integer_operands(ci):
    """Every sum is exact in fp32 whatever its order, so forward, arg-max bytes, dx, dW and db must equal the float64 restatement bit
    for bit -- through windows full of exact ties and pixels that win several overlapping windows."""
    case = R.STAGE_CASES[ci]
    N, H, W, Cin, Cout, K, pad, k, drop = case
    x, w, b, keep, dout = R.exact_case(300 + ci, *case)
    out, arg, dx, dW, db, rows = _run_stage(case, x, w, b, keep, dout)
    r_out, r_arg = R.stage_fwd64(x, w, b, keep, pad, k, k != 0)
    r_dx, r_dW, r_db, _ = R.stage_bwd64(x, w, keep, pad, k, k != 0, r_out, r_arg, dout)
    assert torch.equal(out.double(), r_out), "forward"
    if k:
        assert torch.equal(arg, r_arg), "arg-max bytes"
    if dx is not None:
        assert torch.equal(dx.double(), r_dx), "dx"
    assert torch.equal(dW.double(), r_dW), "dW"
    assert torch.equal(db.double(), r_db), "db"
    if ci == 6:
        assert rows == 9            # 41x37 conv plane in 16x16 tiles: more than one tile per plane


@pytest.mark.parametrize("ci", sorted(R.NORMAL_CASES))
def test_stage_kernels_vs_float64_on_normal_operands(ci):
    """The bars of tests/test_gpu_kernels.py: max error relative to the largest entry of the float64 result, 3e-6 for forward and
    data gradient, 5e-7 for the filter gradients.  Windows whose float64 top-2 gap is below 1e-5 are set apart: their arg-max may fall
    either way, and the float64 backward takes the device's choice there (and only there)."""
    case = R.STAGE_CASES[ci]
    N, H, W, Cin, Cout, K, pad, k, drop = case
    x, w, b, keep, dout = R.normal_case(R.NORMAL_CASES[ci], *case)
    out, arg, dx, dW, db, _ = _run_stage(case, x, w, b, keep, dout)
    x6, w6, b6, d6 = x.double(), w.double(), b.double(), dout.double()
    k6 = keep.double() if keep is not None else None
    r_out, r_arg = R.stage_fwd64(x6, w6, b6, k6, pad, k, True)
    near = R.near_tie_windows(x6, w6, b6, k6, pad, k)
    print("case %d: %d of %d windows within 1e-5 of a tie" % (ci, int(near.sum()), near.numel()))
    assert int(near.sum()) < 1e-3 * near.numel()
    differs = arg != r_arg
    if keep is not None:
        differs = differs & (keep.reshape(N, Cout, 1, 1) != 0)      # (a dropped channel is all +-0: any offset is a maximum; it carries no gradient)
    assert not bool((differs & ~near).any()), "arg-max differs outside the near-tie windows"
    use_arg = torch.where(near, arg, r_arg)
    r_dx, r_dW, r_db, _ = R.stage_bwd64(x6, w6, k6, pad, k, True, r_out, use_arg, d6)

    def rel(a, r):
        return float((a.double() - r).abs().max()) / float(r.abs().max())
    errs = {"out": rel(out, r_out), "dW": rel(dW, r_dW), "db": rel(db, r_db)}
    if dx is not None:
        errs["dx"] = rel(dx, r_dx)
    print("case %d: relative errors %s" % (ci, errs))
    assert errs["out"] <= 3e-6 and errs.get("dx", 0.0) <= 3e-6 and errs["dW"] <= 5e-7 and errs["db"] <= 5e-7, errs


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 2, 2), (70, 1, 1)])
@pytest.mark.parametrize("keep_on", [False, True])
def test_head_kernels_vs_float64(shape, keep_on):
    N, hh, ww = shape
    M_, nC = N * hh * ww, 4
    g = torch.Generator().manual_seed(40 + N + (1 if keep_on else 0))
    x = torch.randn(M_, 16, generator=g).abs()                     # (the head's input is a ReLU output)
    wfc = torch.randn(512, 16, generator=g) * 0.25
    bfc = torch.randn(512, generator=g)
    wc = torch.randn(nC, 512, generator=g) * 0.05
    bc = torch.randn(nC, generator=g)
    wc[2], bc[2] = wc[1], bc[1]                                     # a constructed tie: classes 1 and 2 always get the same logit
    keep = (torch.randint(0, 2, (M_, 512), generator=g).float() * 2) if keep_on else None
    dl = torch.randn(N, nC, hh, ww, generator=g)
    h = L.handle(0)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    x_d, wfc_d, bfc_d, wc_d, bc_d, dl_d = [_dev(t) for t in (x, wfc, bfc, wc, bc, dl)]
    keep_d = _dev(keep) if keep is not None else None
    logits_d = torch.full((N, nC, hh, ww), 7.0, device=DEV)
    am_d = torch.full((N, hh, ww), 99, dtype=torch.uint8, device=DEV)
    common = dict(n=N, h=hh, w=ww, cin=16, cout=nC, count=512, p_w=wfc_d.data_ptr(), p_bias=bfc_d.data_ptr(),
                  p_x0=(keep_d.data_ptr() if keep_d is not None else 0), p_x1=wc_d.data_ptr())
    fop = L.make_op(L.OP_BNN_HEAD_FWD, 0, p_in=x_d.data_ptr(), p_x2=bc_d.data_ptr(), p_out=logits_d.data_ptr(), p_x3=am_d.data_ptr(), **common)
    assert L.OpList([fop]).labels(h)[0] == "bnn_head_fwd<4>"
    L.OpList([fop]).run(h, stream)
    am2_d = torch.full((N, hh, ww), 99, dtype=torch.uint8, device=DEV)      # the labels-only form (predict): no logits are written
    fop2 = L.make_op(L.OP_BNN_HEAD_FWD, 0, p_in=x_d.data_ptr(), p_x2=bc_d.data_ptr(), p_x3=am2_d.data_ptr(), **common)
    L.OpList([fop2]).run(h, stream)
    torch.cuda.synchronize()
    x6, k6 = x.double(), (keep.double() if keep is not None else None)
    r_logits, z = R.head_fwd64(x6, wfc.double(), bfc.double(), k6, wc.double(), bc.double())
    r_nchw = r_logits.reshape(N, hh, ww, nC).permute(0, 3, 1, 2)
    close(logits_d, r_nchw, "logits", rtol=1e-4)
    lc = logits_d.cpu()
    assert torch.equal(lc[:, 1], lc[:, 2])
    want = torch.max(lc, 1)[1]
    assert torch.equal(am_d.cpu().long(), want) and torch.equal(am2_d.cpu().long(), want) and not bool((want == 2).any())
    dx_d = torch.full((N, hh, ww, 16), 7.0, device=DEV)
    outs_d = [torch.full(s, 7.0, device=DEV) for s in ((512, 16), (512,), (nC, 512), (nC,))]
    bop = L.make_op(L.OP_BNN_HEAD_BWD, 0, p_in=dl_d.data_ptr(), p_epi_aux=x_d.data_ptr(), p_out=dx_d.data_ptr(), p_x2=outs_d[0].data_ptr(),
                    p_x3=outs_d[1].data_ptr(), p_x4=outs_d[2].data_ptr(), p_x5=outs_d[3].data_ptr(), **common)
    nbytes = L.op_workspace(h, bop)
    assert nbytes > 0 and bop.i[L.RCV_I_NPART] == M_
    part_d = torch.zeros(nbytes // 4, device=DEV)
    bop.p[L.RCV_P_PART] = part_d.data_ptr()
    runs = []
    for _ in range(2):
        for t in [dx_d] + outs_d:
            t.fill_(7.0)
        L.OpList([bop]).run(h, stream)
        torch.cuda.synchronize()
        runs.append([t.cpu().clone() for t in [dx_d] + outs_d])
    for a, c in zip(*runs):
        assert torch.equal(a, c), "two backward runs differ"
    dl6 = dl.double().permute(0, 2, 3, 1).reshape(M_, nC)
    ref = R.head_bwd64(x6, wfc.double(), k6, wc.double(), z, dl6)
    close(runs[0][0].reshape(M_, 16), ref[0], "dx", rtol=1e-4)
    for got, r, name in zip(runs[0][1:], ref[1:], ("dWfc", "dbfc", "dWc", "dbc")):
        close(got, r, name, rtol=1e-4, floor=1.0)


def test_stage_class_byte_takes_the_first_maximum_on_a_tie():
    """The class byte of the stage record (p[X2]: BNN-M-C's ``predict``) with two pairs of equal classifier filters: classes 0 / 1 and
    2 / 3 get bitwise-equal logits at every pixel, so only the first of a pair may ever be named; with and without the logits beside."""
    N, H, W, Cin, Cout, K = 3, 6, 7, 16, 4, 3
    g = torch.Generator().manual_seed(51)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g)
    b = torch.randn(Cout, generator=g)
    w[1], b[1], w[3], b[3] = w[0], b[0], w[2], b[2]
    h = L.handle(0)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    x_d, w_d, b_d = _dev(x), _dev(w), _dev(b)
    Ho, Wo = H - K + 1, W - K + 1
    logits_d = torch.full((N, Cout, Ho, Wo), 7.0, device=DEV)
    labels = [torch.full((N, Ho, Wo), 99, dtype=torch.uint8, device=DEV) for _ in range(2)]
    common = dict(n=N, h=H, w=W, cin=Cin, cout=Cout, ho=Ho, wo=Wo, aux0=K, aux1=0, count=0, inmode=L.LOAD_PLAIN, p_in=x_d.data_ptr(),
                  p_w=w_d.data_ptr(), p_bias=b_d.data_ptr())
    both = L.make_op(L.OP_BNN_STAGE_FWD, L.F_OUT_NCHW, p_out=logits_d.data_ptr(), p_x2=labels[0].data_ptr(), **common)
    only = L.make_op(L.OP_BNN_STAGE_FWD, L.F_OUT_NCHW, p_x2=labels[1].data_ptr(), **common)
    L.OpList([both, only]).run(h, stream)
    torch.cuda.synchronize()
    lc = logits_d.cpu()
    assert torch.equal(lc[:, 0], lc[:, 1]) and torch.equal(lc[:, 2], lc[:, 3])
    top = torch.maximum(lc[:, 0], lc[:, 2])
    want = torch.where(lc[:, 0] == top, 0, 2)              # the first maximum in class order, written out
    assert torch.equal(want, torch.max(lc, 1)[1])
    for lab in labels:
        assert torch.equal(lab.cpu().long(), want)
    assert bool((want == 0).any()) and bool((want == 2).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(net):
    import robocupvision_amd.model as M
    torch.manual_seed(12345678)
    return getattr(M, net)()


def _device_masks(masks, net):
    out = [m.to(DEV) for m in masks[:3]]
    if net == "BNNL":
        out.append(masks[3].permute(0, 2, 3, 1).contiguous().to(DEV))      # the modules take dof as [N][h][w][512]
    return out


def _step(model, x, t, weights, opt=None):
    """The body of objDetEval.py:113-119 with stock torch loss and optimiser."""
    crit = torch.nn.CrossEntropyLoss(torch.tensor(weights, device=DEV))
    if opt is not None:
        opt.zero_grad()
    else:
        model.zero_grad()
    logits = model(x)
    pred = torch.squeeze(logits)
    loss = crit(pred, t)
    loss.backward()
    if opt is not None:
        opt.step()
    return logits.detach(), float(loss.detach())


@pytest.mark.parametrize("tag", TAGS)
def test_whole_step_vs_golden(tag, bnn_golden):
    kats, meta = bnn_golden
    e = meta[tag]
    net = e["net"]
    model = _model(net).to(DEV).train()
    x = golden_input(e).to(DEV)
    t = torch.from_numpy(kats[tag + "/t"]).to(DEV)
    model._impose_dropout(_device_masks(golden_masks(kats, tag, net), net))
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=e["sgd"]["lr"], momentum=e["sgd"]["momentum"], weight_decay=e["sgd"]["weight_decay"])
    logits, loss = _step(model, x, t, e["weights"])
    assert list(logits.shape) == e["logits_shape"]
    close(logits, torch.from_numpy(kats[tag + "/logits"]), "logits", rtol=1e-3)
    assert abs(loss - e["loss"]) <= 1e-4 * abs(e["loss"]), (loss, e["loss"])
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        a, b = golden_grad(kats, meta, tag, name, p.grad.cpu())
        close(a, b, "grad " + name, rtol=1e-3, floor=1.0)
    opt.step()
    for name, p in model.named_parameters():
        # the bar of tests/test_gpu_pbfcn.py::_check_after (tests/test_classify.py, smoke()): SGD moves an element by lr |g| per step;
        # the sums must agree to a small fraction of that scale
        got, ref = float(p.detach().double().sum()), e["param_after_step_sum"][name]
        print("%s %s: sum after the step %.9f, golden %.9f" % (tag, name, got, ref))
        assert abs(got - ref) <= 1e-3 * max(1.0, abs(ref)) + 1e-4 * p.numel() ** 0.5 * e["sgd"]["lr"], (name, got, ref)
    model.eval()
    with torch.no_grad():
        close(model(x), torch.from_numpy(kats[tag + "/eval_logits"]), "eval logits after the step", rtol=1e-3)


@pytest.mark.parametrize("net", ["BNNL", "BNNMC"])
def test_two_steps_from_the_same_state_are_bitwise_equal(net):
    x = torch.randn(5, 3, 40, 36, generator=torch.Generator().manual_seed(21)).to(DEV)
    hh, ww = R.out_plane(net, 40, 36)
    tshape = [5] + [d for d in (hh, ww) if d != 1]          # the caller's torch.squeeze drops the unit axes of the logit plane
    t = torch.randint(0, 4, tshape, generator=torch.Generator().manual_seed(22)).to(DEV)
    model = _model(net).to(DEV).train()
    _step(model, x, t, R.CE_WEIGHTS)
    model._impose_dropout(model._last_dropout_scales())
    grads = []
    for _ in range(2):
        logits, loss = _step(model, x, t, R.CE_WEIGHTS)
        grads.append([logits.cpu()] + [p.grad.cpu().clone() for p in model.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert all(float(g.abs().max()) > 0 for g in grads[0][1:])


def test_dropout_draws_and_refusals():
    model = _model("BNNL").to(DEV).train()
    x = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(23)).to(DEV)
    with torch.no_grad():
        model(x)
    a = model._last_dropout_scales()
    with torch.no_grad():
        model(x)
    b = model._last_dropout_scales()
    assert [tuple(s.shape) for s in a] == [(64, 8), (64, 16), (64, 16), (64, 1, 1, 512)]
    legal = float(torch.tensor(1.0) / torch.tensor(0.75))
    for s in a[:3]:
        assert bool(((s == 0) | (s == legal)).all())
    assert bool(((a[3] == 0) | (a[3] == 2)).all())
    assert abs(float((a[1] != 0).float().mean()) - 0.75) <= 4 * math.sqrt(0.75 * 0.25 / 1024)      # a 64 x 16 draw
    assert abs(float((a[3] != 0).float().mean()) - 0.5) <= 4 * math.sqrt(0.25 / (64 * 512))
    assert any(not torch.equal(p, q) for p, q in zip(a, b)), "no new draw per forward"
    model._impose_dropout(a)
    with torch.no_grad():
        model(x)
    assert all(torch.equal(p, q) for p, q in zip(a, model._last_dropout_scales()))
    with pytest.raises(L.RcvError, match="do not fit this batch"):
        with torch.no_grad():
            model(x[:32])
    # eval mode ignores an imposed list
    model.eval()
    with torch.no_grad():
        e1 = model(x[:32]).cpu()
        model._impose_dropout(None)
        e2 = model(x[:32]).cpu()
    assert torch.equal(e1, e2)
    # refusals of the module surface, before any launch
    model.train()
    with pytest.raises(L.RcvError, match="gradient for its input"):
        model(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        model(x.double())
    with pytest.raises(ValueError):
        model(x[0])
    with pytest.raises(L.RcvError, match="2 input channels"):
        model(x[:, :2])
    with pytest.raises(L.RcvError, match="too small"):
        model(x[:, :, :20])
    with pytest.raises(L.RcvError, match="training mode"):
        model.predict(x)


def test_trajectory_vs_cpu_restatement_and_loss_goes_down():
    """Three steps of BNN-L at B = 8 with the same keep-scales on both sides: losses within 1e-3 relative (the bar of
    tests/test_classify.py's trajectory); then the eval-mode loss of the fixed batch after 20 training steps is below the start's."""
    B = 8
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, 3, 32, 32, generator=g)
    t = torch.randint(0, 4, (B,), generator=g)
    masks = []
    for _ in range(3):
        ms = [(torch.rand(B, c, generator=g) < 0.75).float() / torch.tensor(0.75) for c in (8, 16, 16)]
        ms.append((torch.rand(B, 512, 1, 1, generator=g) < 0.5).float() * 2)
        masks.append(ms)
    model = _model("BNNL")
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ref_losses, _ = R.train_steps("BNNL", sd, x, t, masks)
    model = model.to(DEV).train()
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-2, momentum=0.9, weight_decay=5e-4)
    xd, td = x.to(DEV), t.to(DEV)

    def eval_loss():
        model.eval()
        with torch.no_grad():
            v = float(torch.nn.CrossEntropyLoss(torch.tensor(R.CE_WEIGHTS, device=DEV))(torch.squeeze(model(xd)), td))
        model.train()
        return v
    start = eval_loss()
    for step in range(3):
        model._impose_dropout(_device_masks(masks[step], "BNNL"))
        _, loss = _step(model, xd, td, R.CE_WEIGHTS, opt)
        print("step %d: loss %.7f, restatement %.7f" % (step, loss, ref_losses[step]))
        assert abs(loss - ref_losses[step]) <= 1e-3 * abs(ref_losses[step]), (step, loss, ref_losses[step])
    model._impose_dropout(None)
    for _ in range(17):
        _step(model, xd, td, R.CE_WEIGHTS, opt)
    end = eval_loss()
    assert end < start, (start, end)


@pytest.mark.parametrize("net", ["BNNL", "BNNMC"])
def test_a_plane_of_many_tiles_runs(net):
    """120x160 (eval mode, gradients on): logits against the fp32 CPU restatement at the golden bar; gradients at the relative-L2 bar of
    tests/test_classify.py's trajectory (5e-3), which a single pool arg-max that falls the other way in fp32 does not break."""
    model = _model(net)
    sd = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()}
    x = torch.randn(1, 3, 120, 160, generator=torch.Generator().manual_seed(33))
    ref = R.forward(net, sd, x)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(34))
    ref.backward(gout)
    model = model.to(DEV).eval()
    out = model(x.to(DEV))
    assert tuple(out.shape) == tuple(ref.shape) == (1, 4) + R.out_plane(net, 120, 160)
    close(out, ref.detach(), "logits", rtol=1e-3)
    out.backward(gout.to(DEV))
    for name, p in model.named_parameters():
        r = sd[name].grad
        err = float((p.grad.cpu().double() - r.double()).norm() / r.double().norm())
        assert err <= 5e-3, (name, err)


@pytest.mark.parametrize("net", ["BNNL", "BNNMC"])
def test_predict_and_patch_metrics_match_torch_max_and_the_host_loop(net):
    from robocupvision_amd.metrics import PatchMetrics
    g = torch.Generator().manual_seed(35)
    x = torch.randn(64, 3, 32, 32, generator=g).to(DEV)
    labels = torch.randint(0, 4, (64,), generator=g)
    model = _model(net).to(DEV).eval()
    with torch.no_grad():
        logits = model(x)
    pred = model.predict(x)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (64, 1, 1)
    want = torch.max(torch.squeeze(logits).cpu(), 1)[1]
    assert torch.equal(pred.cpu().reshape(64).long(), want)
    with torch.no_grad():
        assert torch.equal(model(x), logits)               # predict left the plan's logits slot usable
    big = model.predict(x[:2, :, :, :].repeat(1, 1, 2, 2)[:, :, :40, :36])
    with torch.no_grad():
        lb = model(x[:2].repeat(1, 1, 2, 2)[:, :, :40, :36].contiguous())
    assert torch.equal(big.cpu().long(), torch.max(lb.cpu(), 1)[1])
    pm = PatchMetrics(4)
    pm.update(pred, labels.to(DEV))
    pm.update(pred.reshape(64), labels.to(DEV))
    conf = torch.zeros(4, 4).long()
    for j in range(64):                                    # objDetEval.py:158-159
        conf[(want[j], labels[j])] += 2
    res = pm.compute()
    assert torch.equal(res["confusion"], conf)
    assert res["acc"] == pytest.approx(float(torch.sum(want == labels)) * 100 / 64, rel=1e-12)
    total = torch.sum(conf[:, 1:4]).item()
    totAcc = int(conf[1, 1] + conf[2, 2] + conf[3, 3])
    assert res["obj_acc"] == pytest.approx(totAcc / total * 100, rel=1e-12)
    assert res["false_pos"] == pytest.approx((torch.sum(conf[1:4, :]).item() - totAcc) / total * 100, rel=1e-12)
