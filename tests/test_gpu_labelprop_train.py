"""GPU: LabelProp's training step (labelPropTrain.py:162-215) -- the tail kernels through rcv_run against the float64 restatement,
the batch assembly against its fixture, the whole step against the reference's goldens (tests/golden/make_golden_labelprop_train.py)
with the bars of tests/test_gpu_pbfcn.py, fused-loss against autograd path, five steps against a torch-CPU twin, the prune mask."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, sd_hash
import labelprop_restatement as R
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer
from test_gpu_blocks import close, _t
from test_gpu_net import check_mask
from test_gpu_pbfcn import _check_after
from test_gpu_small_ops import _exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = R.LP_SGD["lr"]

with open(os.path.join(GOLDEN, "labelprop_train.json")) as _f:
    META = json.load(_f)


def kats(tag):
    return np.load(os.path.join(GOLDEN, "labelprop_train_%s.npz" % tag[3:]))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _run(op):
    L.OpList([op]).run(L.handle(0), torch.cuda.current_stream(DEV).cuda_stream)


def _with_workspace(op):
    nbytes = L.op_workspace(L.handle(0), op)
    ws = _nan(max(nbytes // 4, 1))
    op.p[L.RCV_P_PART] = ws.data_ptr()
    return ws


# ------------------------------------------------------------------------------------------ tail kernels
# (N, H, W, classes, skip load mode): pixel counts that are no multiple of 256 (and of 64), every class-count extreme
TAIL_CASES = [(2, 9, 11, 5, L.LOAD_AFFINE_RELU), (1, 7, 5, 1, L.LOAD_AFFINE_RELU), (3, 13, 17, 8, L.LOAD_AFFINE_RELU),
              (2, 24, 40, 5, L.LOAD_AFFINE), (1, 33, 31, 3, L.LOAD_PLAIN), (5, 120, 160, 5, L.LOAD_AFFINE_RELU)]


@pytest.mark.parametrize("ci", range(len(TAIL_CASES)))
def test_tail_kernels_vs_float64(ci):
    N, H, W, nC, mode = TAIL_CASES[ci]
    _tail_randn_case(ci, N, H, W, nC, mode, 8)


def _tail_randn_case(ci, N, H, W, nC, mode, rch):
    """Random operands through all forms of the tail: the fused-loss, the plain and the eval-mode forward give the same logits bit for
    bit, the loss row equals RCV_OP_CE_FWD's on the same logits, the fused-loss backward equals the logits-gradient one, two runs are
    equal; all of it against float64 at the project's bars."""
    rng = np.random.default_rng(300 + ci)
    t = rng.standard_normal((N, H, W, 16)).astype(np.float32)
    r = rng.standard_normal((N, H, W, rch)).astype(np.float32)
    tc = np.zeros((5, 16), np.float32)
    tc[0], tc[1], tc[2] = rng.uniform(0.5, 1.5, 16), rng.standard_normal(16) * 0.3, rng.standard_normal(16) * 0.2
    rc = np.zeros((5, rch), np.float32)
    rc[0], rc[1] = rng.uniform(0.5, 1.5, rch), rng.standard_normal(rch) * 0.3
    w = (rng.standard_normal((nC, 16)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(nC) * 0.1).astype(np.float32)
    tgt = rng.integers(0, nC, (N, H, W)).astype(np.int64)
    tgt.reshape(-1)[::37] = -100                          # ignored pixels, as NLLLoss's ignore_index
    cw = rng.uniform(0.5, 6.0, nC).astype(np.float32)
    t_d, r_d, tc_d, rc_d, w_d, b_d, cw_d = (_dev(a) for a in (t, r, tc, rc, w, b, cw))
    tgt_d = _dev(tgt, torch.int64)
    common = dict(n=N, h=H, w=W, cin=16, cout=nC, aux0=mode, aux1=rch, p_w=w_d.data_ptr(), p_x3=r_d.data_ptr(), p_x4=rc_d.data_ptr())

    # forward: the fused-loss launch, the plain launch and the eval-mode classifier record give the same logits, bit for bit
    logits_d, logits2_d, loss_d = _nan(N, nC, H, W), _nan(N, nC, H, W), _nan(4)
    am_d = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
    fkw = dict(p_in=t_d.data_ptr(), p_in_c=tc_d.data_ptr(), p_bias=b_d.data_ptr(), **common)
    fop = L.make_op(L.OP_LP_TAIL_FWD, L.F_FUSED_UP | L.F_FUSED_CE, p_out=logits_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_x0=cw_d.data_ptr(),
                    p_x1=loss_d.data_ptr(), p_x2=am_d.data_ptr(), **fkw)
    ws_f = _with_workspace(fop)
    assert L.OpList([fop]).labels(L.handle(0))[0] == "lp_tail_fwd<1>"
    _run(fop)
    logits3_d = _nan(N, nC, H, W)
    _run(L.make_op(L.OP_LP_TAIL_FWD, L.F_FUSED_UP, p_out=logits2_d.data_ptr(), **fkw))
    _run(L.make_op(L.OP_CLS_FWD, L.F_FUSED_UP, p_out=logits3_d.data_ptr(), **fkw))          # the record inference uses
    torch.cuda.synchronize()
    assert torch.equal(logits_d, logits2_d) and torch.equal(logits_d, logits3_d)
    top = R.load_np(r, rc, mode)
    v, logits = R.tail_forward_np(t, tc, top, w, b)
    close(logits_d, torch.from_numpy(logits), "logits", rtol=1e-4)
    loss, dl = R.ce_np(logits, tgt, cw)
    got = loss_d.cpu().double()
    print("case %d: loss %.8f vs %.8f" % (ci, float(got[0]), loss))
    assert abs(float(got[0]) - loss) <= 1e-5 * abs(loss)
    am = logits_d.argmax(1)
    margin = np.sort(logits, 1)
    clear = torch.from_numpy((margin[:, -1] - margin[:, -2]) > 1e-4) if nC > 1 else torch.ones(N, H, W, dtype=torch.bool)
    assert torch.equal(am_d.cpu()[clear].long(), torch.from_numpy(logits.argmax(1))[clear])
    assert torch.equal(am_d.long(), am) and int(got[2]) == int((am.cpu() == torch.from_numpy(tgt)).sum())
    # the loss of the separate kernels on the same logits: same partial rows, same bits
    loss2_d, am2_d = _nan(4), torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
    cop = L.make_op(L.OP_CE_FWD, L.F_ARGMAX, n=N, h=H, w=W, cout=nC, p_in=logits_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(),
                    p_out=loss2_d.data_ptr(), p_x0=am2_d.data_ptr())
    ws_c = _with_workspace(cop)
    _run(cop)
    torch.cuda.synchronize()
    assert torch.equal(loss_d, loss2_d) and torch.equal(am_d, am2_d), (loss_d, loss2_d)

    # backward, both forms
    one_d = torch.ones(1, device=DEV)
    dl_d = _nan(N, nC, H, W)
    _run(L.make_op(L.OP_CE_BWD, 0, n=N, h=H, w=W, cout=nC, p_in=logits_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(),
                   p_x0=loss_d.data_ptr(), p_x1=one_d.data_ptr(), p_out=dl_d.data_ptr()))
    outs = []
    for with_ce in (False, True, True):
        dup_d, dskip_d, dw_d, db_d = _nan(N, H, W, 16), _nan(N, H, W, rch), _nan(nC, 16), _nan(nC)
        bop = L.make_op(L.OP_LP_TAIL_BWD, L.F_FUSED_UP | (L.F_FUSED_CE if with_ce else 0), stats=L.STATS_BWD_DEC, p_out=dup_d.data_ptr(),
                        p_in_aux=dskip_d.data_ptr(), p_epi_aux=t_d.data_ptr(), p_epi_c=tc_d.data_ptr(), p_x1=dw_d.data_ptr(),
                        p_x2=db_d.data_ptr(), p_in2=(tgt_d if with_ce else dl_d).data_ptr(), **common)
        if with_ce:
            bop.p[L.RCV_P_X0], bop.p[L.RCV_P_BIAS] = cw_d.data_ptr(), b_d.data_ptr()
            bop.p[L.RCV_P_X5], bop.p[L.RCV_P_IN2_AUX] = loss_d.data_ptr(), one_d.data_ptr()
        ws_b = _with_workspace(bop)
        n_part = bop.i[L.RCV_I_NPART]
        assert L.OpList([bop]).labels(L.handle(0))[0] == "lp_tail_bwd<%d,%d>" % (nC, int(with_ce))
        _run(bop)
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (dup_d, dskip_d, dw_d, db_d, ws_b[:n_part * 32])])
    for a, c, e in zip(*outs):
        assert torch.equal(a, c), "fused-loss and logits-gradient forms differ"
        assert torch.equal(c, e), "two runs differ"
    gup, gskip, gw, gb, gpart = outs[0]
    dW, db, g, gs, stats = R.tail_backward_np(t, tc, v, w, dl, rch)
    close(dl_d, torch.from_numpy(dl), "dlogits", rtol=1e-4)
    close(gw, torch.from_numpy(dW), "dW", rtol=1e-4, floor=1.0)
    close(gb, torch.from_numpy(db), "db", rtol=1e-4, floor=1.0)
    close(gup, torch.from_numpy(g), "d upConv3", rtol=1e-4)
    assert torch.equal(gskip, gup[..., :rch].contiguous()), "the skip gradient is the first rch channels of the data gradient"
    rows = gpart.reshape(n_part, 2, 16).double().sum(0)
    close(rows, torch.from_numpy(stats), "statistics rows", rtol=1e-4, floor=1.0)
    del ws_f, ws_c


def _cus():
    return int(L.load().rcv_num_cus(L.handle(0)))


GUARD = 64      # floats behind a buffer that no lane may touch


def _guarded(a):
    """The array on the device with GUARD zeros behind it (the skip tensor: nothing behind its N*H*W*rch floats belongs to it)."""
    return _dev(np.concatenate([np.asarray(a, np.float32).reshape(-1), np.zeros(GUARD, np.float32)]))


def _tail_exact_case(plane, nC, rch, mode, second):
    """lp_tail_fwd<0> and lp_tail_bwd<nC,0> on integer-grid operands: logits, d upConv3, the skip gradient, dW, db and the float64 fold
    of the partial statistics rows equal the restatement bit for bit; the skip gradient is the first rch channels of the data
    gradient and nothing is stored behind its N*H*W*rch floats."""
    N, H, W = plane
    npix = N * H * W
    c = R.build_tail(plane, nC, rch, mode, second)
    logits, dW, db, g, gskip, stats = R.check_tail(c)
    t_d, tc_d, rc_d, w_d, b_d, dl_d = (_dev(c[k]) for k in ("t", "tc", "rc", "w", "b", "dl"))
    r_d = _guarded(c["r"])
    common = dict(n=N, h=H, w=W, cin=16, cout=nC, aux0=mode, aux1=rch, p_w=w_d.data_ptr(), p_x3=r_d.data_ptr(), p_x4=rc_d.data_ptr())
    logits_d, dup_d, dskip_d, dw_d, db_d = _nan(N, nC, H, W), _nan(N, H, W, 16), _nan(npix * rch + GUARD), _nan(nC, 16), _nan(nC)
    fop = L.make_op(L.OP_LP_TAIL_FWD, L.F_FUSED_UP, p_in=t_d.data_ptr(), p_in_c=tc_d.data_ptr(), p_bias=b_d.data_ptr(),
                    p_out=logits_d.data_ptr(), **common)
    bop = L.make_op(L.OP_LP_TAIL_BWD, L.F_FUSED_UP, stats=L.STATS_BWD_DEC, p_out=dup_d.data_ptr(), p_in_aux=dskip_d.data_ptr(),
                    p_epi_aux=t_d.data_ptr(), p_epi_c=tc_d.data_ptr(), p_x1=dw_d.data_ptr(), p_x2=db_d.data_ptr(), p_in2=dl_d.data_ptr(), **common)
    ws = _with_workspace(bop)
    n_part = bop.i[L.RCV_I_NPART]
    labels = L.OpList([fop, bop]).labels(L.handle(0))
    assert labels == ["lp_tail_fwd<0>", "lp_tail_bwd<%d,0>" % nC], labels
    assert n_part == min(-(-npix // 256), 4 * _cus())
    _run(fop)
    _run(bop)
    torch.cuda.synchronize()
    what = "lp tail %s %d classes rch %d mode %d: " % (plane, nC, rch, mode)
    _exact(logits_d, logits, what + "logits")
    _exact(dup_d, g, what + "d upConv3")
    _exact(dskip_d[:npix * rch].reshape(N, H, W, rch), gskip, what + "skip gradient")
    assert torch.equal(dskip_d[:npix * rch].reshape(N, H, W, rch), dup_d[..., :rch].contiguous())
    assert bool(torch.isnan(dskip_d[npix * rch:]).all()), what + "a lane without a skip stored behind the skip gradient"
    _exact(dw_d, dW, what + "dW")
    _exact(db_d, db, what + "db")
    _exact(ws[:n_part * 32].reshape(n_part, 2, 16).double().sum(0), stats, what + "statistics rows")
    return n_part


@pytest.mark.parametrize("rch", R.TAIL_RCH)
def test_tail_kernels_exact(rch):
    """Every class count in {1, 5, 8} and skip load mode on 2x9x11 and 1x1x1; both planes beyond one grid pass (a multiple of 256
    pixels and an odd count, sized from the device's CU count): the backward's COUT*16 + COUT + 8 register sums per lane carried into
    a second chunk.  The first pixel of the second pass and the last pixel add a non-zero term to every reduced entry
    (R.check_tail), so a lost pixel, chunk or accumulator cannot go unseen."""
    cus = _cus()
    cap = 4 * cus * 256
    big = 0
    for plane, nC, rch_, mode, second in R.tail_exact_cases(cus):
        if rch_ != rch:
            continue
        npix = plane[0] * plane[1] * plane[2]
        n_part = _tail_exact_case(plane, nC, rch, mode, second)
        if second:
            print("lp tail %s: %d pixels, one grid pass covers %d (%d CUs x 4 workgroups x 256)" % (plane, npix, cap, cus))
            assert npix > cap and n_part == 4 * cus and n_part * 256 < npix
            big += 1
    assert big == 2


@pytest.mark.parametrize("rch", [4, 16])
def test_tail_fused_loss_forms_beyond_one_grid_pass(rch):
    """The fused cross-entropy forms (lp_tail_fwd<1>, lp_tail_bwd<5,1>) past one grid pass at the narrowest and the widest skip, random
    operands: the assertions and bars of test_tail_kernels_vs_float64."""
    cus = _cus()
    N, H, W = R.tail_big_planes(cus)[1]
    print("lp tail fused forms %s: %d pixels, one grid pass covers %d" % ((N, H, W), N * H * W, 4 * cus * 256))
    assert N * H * W > 4 * cus * 256
    _tail_randn_case(40 + rch, N, H, W, 5, L.LOAD_AFFINE_RELU if rch == 4 else L.LOAD_AFFINE, rch)


# ------------------------------------------------------------------------------------------ batch assembly
@pytest.mark.parametrize("tag", R.SMALL)
def test_batch_assembly_equals_the_fixture_exactly(tag):
    k = kats(tag)
    im, lab = _t(k[tag + "/images"]).to(DEV), _t(k[tag + "/labels"]).to(DEV)
    x, t = M.labelprop_batch(im, lab)
    B, _, _, H, W = im.shape
    assert x.shape == (2 * B, 8, H, W) and x.stride() == (H * W * 8, 1, W * 8, 8) and x.dtype == torch.float32
    assert x.permute(0, 2, 3, 1).is_contiguous() and t.is_contiguous() and t.dtype == torch.int64
    assert torch.equal(x.cpu(), _t(k[tag + "/x"])) and torch.equal(t.cpu(), _t(k[tag + "/t"]))
    # out-of-range labels: all five class channels -1, the label itself passed through to the targets
    lab2 = lab.clone()
    lab2[0, 0, 0, 0], lab2[0, 1, 1, 1] = 5, -100
    x2, t2 = M.labelprop_batch(im, lab2)
    xr, tr_ = R.assemble_np(im.cpu().numpy(), lab2.cpu().numpy())
    assert torch.equal(x2.cpu(), torch.from_numpy(xr)) and torch.equal(t2.cpu(), torch.from_numpy(tr_))
    assert float(x2[1, 3:, 0, 0].max()) == -1.0 and float(x2[0, 3:, 1, 1].max()) == -1.0
    # more channels per frame than the script's loader gives: only channel 0 is read
    im5 = torch.cat([im, torch.full_like(im[:, :, :2], 9.0)], 2)
    x5, _ = M.labelprop_batch(im5, lab)
    assert torch.equal(x5, x)


def test_batch_assembly_beyond_the_grid_cap():
    """RCV_OP_LP_BATCH is capped at 8 workgroups per CU: an odd pixel count beyond 8 * CUs * 256 (3x419x421 on 256 CUs), three
    channels per frame, bitwise against the restatement; labels 5, -1, -100 and 1 << 40 sit in the second pass."""
    cus = _cus()
    cap = 8 * cus * 256
    B, W = 3, 421
    H = cap // (B * W) + 1
    H += 1 - H % 2
    while B * H * W - cap < 16:
        H += 2
    print("lp batch %dx%dx%d: %d pixels, one grid pass covers %d" % (B, H, W, B * H * W, cap))
    assert B * H * W > cap and (B * H * W) % 2 == 1
    rng = np.random.default_rng(77)
    im = rng.standard_normal((B, 2, 3, H, W)).astype(np.float32)
    lab = rng.integers(0, 5, (B, 2, H, W)).astype(np.int64)
    b2, hw = cap // (H * W), cap % (H * W)                       # element `cap` = (pair b2, pixel hw): the first of the second pass
    assert b2 == B - 1 and hw + 8 < H * W
    flat = lab.reshape(B, 2, H * W)
    flat[b2, 0, hw:hw + 4] = [5, -1, -100, 1 << 40]
    flat[b2, 1, hw + 2:hw + 6] = [1 << 40, 5, -1, -100]
    flat[b2, :, -1] = [-100, 1 << 40]
    x, t = M.labelprop_batch(_t(im).to(DEV), _t(lab).to(DEV))
    xr, tr_ = R.assemble_np(im, lab)
    assert torch.equal(x.cpu(), torch.from_numpy(xr)) and torch.equal(t.cpu(), torch.from_numpy(tr_))
    assert float(x[2 * b2 + 1, 3:].reshape(5, -1)[:, hw:hw + 4].max()) == -1.0 and int(t[2 * b2].reshape(-1)[hw + 3]) == 1 << 40


# ------------------------------------------------------------------------------------------ whole step
def _model():
    torch.manual_seed(12345678)
    model = M.LabelProp(5, 32, 0.0)
    return model


def _batch(tag):
    m = META[tag]
    if tag in R.SMALL:
        k = kats(tag)
        im, lab = _t(k[tag + "/images"]), _t(k[tag + "/labels"])
    else:
        im, lab = R.synthetic_pairs(m["P"], m["H"], m["W"], m["seed"])
        assert abs(float(im.double().sum()) - m["images_sum"]) < 1e-6 and int(lab.sum()) == m["labels_sum"]
    return M.labelprop_batch(im.to(DEV), lab.to(DEV))


def _near(tag):
    P, H, W, _ = R.CONFIGS[tag]
    near = np.nonzero(np.unpackbits(kats(tag)[tag + "/near_tie"])[:2 * P * H * W])[0]
    assert near.size <= max(1, int(R.NEAR_TIE_CAP * 2 * P * H * W))
    return near


def _autograd_step(model, opt, x, t):
    crit = M.CrossEntropyLoss2d(torch.tensor(R.LP_WEIGHTS)).to(DEV)
    model.train()
    opt.zero_grad()
    pred = model(x)
    loss = crit(pred, t)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    return pred.detach().clone(), float(loss.detach()), grads, crit.last_argmax.clone()


def _trainer_step(tr, x, t):
    pred = tr.step(x, t).clone()
    grads = {k: p.grad.detach().clone() for k, p in tr.model.named_parameters()}
    return pred, tr.pop_metrics()["loss"], grads, tr.criterion.last_argmax.clone()


def _check_grads(tag, grads, k, m):
    assert len(grads) == 35
    for name, g in grads.items():
        if name.startswith("upConv") and name.endswith("conv.bias"):
            assert float(g.abs().max()) == 0.0          # a bias ahead of a BatchNorm: exactly zero here, rounding noise in the reference
            continue
        bn = name.endswith("bn.weight") or name.endswith("bn.bias")
        key = "%s/grad/%s" % (tag, name)
        if key in k.files:
            ref = _t(k[key])
            err = float((g.cpu().double() - ref.double()).norm())
            print("%s grad %-22s L2 error / norm %.2e (reference fp32 vs float64 %.2e)" % (tag, name, err / float(ref.double().norm()),
                                                                                         m["grad_fp32_vs_fp64_rel"][name]))
            if bn:
                assert err <= 1e-2 * float(ref.double().norm()), (name, err)
            else:
                close(g, ref, "%s grad %s" % (tag, name), rtol=1e-3, floor=1.0)
        else:
            n_ = m["grad_norm"][name]
            gn = float(g.double().norm())
            print("%s grad %-22s norm %.6e vs %.6e" % (tag, name, gn, n_))
            assert abs(gn - n_) <= (1e-2 if bn else 1e-3) * n_ + 1e-7, (name, gn, n_)
            idx = R.sample_index(g.numel(), name, META["_sample"]["grad"]).to(DEV)
            close(g.reshape(-1)[idx], _t(k["%s/grad_sample/%s" % (tag, name)]), "%s grad sample %s" % (tag, name), rtol=1e-3, floor=1.0)


@pytest.mark.parametrize("tag,fused", [(t_, f_) for t_ in R.SMALL for f_ in (False, True)])
def test_step_vs_golden_small(tag, fused):
    m, k = META[tag], kats(tag)
    model = _model()
    assert sd_hash(model.state_dict()) == m["sd_hash_init"]
    model = model.to(DEV)
    x, t = _batch(tag)
    opt = SGD(model, **R.LP_SGD)
    tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=opt) if fused else None
    step = (lambda: _trainer_step(tr, x, t)) if fused else (lambda: _autograd_step(model, opt, x, t))
    pred, loss, grads, am = step()
    print("%s loss %.8f vs %.8f" % (tag, loss, m["loss"]))
    close(pred, _t(k[tag + "/logits"]), tag + " logits", rtol=1e-3)
    assert abs(loss - m["loss"]) <= 1e-3 * abs(m["loss"])
    check_mask(am, k[tag + "/argmax"], _near(tag), tag)
    assert torch.equal(am.long(), pred.argmax(1))
    _check_grads(tag, grads, k, m)
    sd = model.state_dict()
    for key in k.files:
        if key.startswith(tag + "/after/"):
            close(sd[key[len(tag) + 7:]], _t(k[key]), key)
    assert int(sd["pre.bn.num_batches_tracked"]) == 1 and int(sd["upConv3.bn.num_batches_tracked"]) == 1
    _check_after(sd, m["param_after_step_sum"], LR)
    model.eval()
    with torch.no_grad():
        pe = model(x)
    close(pe, _t(k[tag + "/eval_logits"]), tag + " eval logits after the step (a stale eval cache would not pass)", rtol=5e-3)
    _, loss2, _, _ = step()
    print("%s step-2 loss %.8f vs %.8f" % (tag, loss2, m["loss_step2"]))
    assert abs(loss2 - m["loss_step2"]) <= 2e-3 * abs(m["loss_step2"])
    _check_after(model.state_dict(), m["param_after_2_steps_sum"], 2 * LR)
    assert int(model.state_dict()["pre.bn.num_batches_tracked"]) == m["num_batches_tracked"] == 2


def test_step_vs_golden_script_shape():
    """The script's batch: 8 frame pairs at 120x160 (16 images), assembled on the device, through the Trainer."""
    tag = "lp_16x120x160"
    m, k = META[tag], kats(tag)
    model = _model().to(DEV)
    x, t = _batch(tag)
    assert abs(float(x.double().sum()) - m["x_sum"]) < 1e-6
    tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=SGD(model, **R.LP_SGD))
    pred, loss, grads, am = _trainer_step(tr, x, t)
    print("%s loss %.8f vs %.8f" % (tag, loss, m["loss"]))
    assert abs(loss - m["loss"]) <= 1e-3 * abs(m["loss"])
    assert abs(float(pred.double().abs().sum()) - m["logits_abs_sum"]) <= 1e-3 * m["logits_abs_sum"]
    assert abs(float(pred.double().sum()) - m["logits_sum"]) <= 1e-3 * m["logits_abs_sum"]
    idx = R.sample_index(pred.numel(), tag + "/logits", META["_sample"]["logits"]).to(DEV)
    close(pred.reshape(-1)[idx], _t(k[tag + "/logits_sample"]), tag + " logits sample", rtol=1e-3)
    ndiff = check_mask(am, k[tag + "/argmax"], _near(tag), tag)
    assert abs(int(tr.criterion.last_stats[2]) - m["correct"]) <= ndiff
    _check_grads(tag, grads, k, m)
    sd = model.state_dict()
    for key in k.files:
        if key.startswith(tag + "/after/"):
            close(sd[key[len(tag) + 7:]], _t(k[key]), key)
    _check_after(sd, m["param_after_step_sum"], LR)
    pe, _, _ = tr.evaluate(x, t)
    close(pe.reshape(-1)[idx], _t(k[tag + "/eval_logits_sample"]), tag + " eval logits sample", rtol=5e-3)
    assert abs(float(pe.double().abs().sum()) - m["eval_logits_abs_sum"]) <= 5e-3 * m["eval_logits_abs_sum"]
    _, loss2, _, _ = _trainer_step(tr, x, t)
    assert abs(loss2 - m["loss_step2"]) <= 2e-3 * abs(m["loss_step2"])
    _check_after(model.state_dict(), m["param_after_2_steps_sum"], 2 * LR)


def _two_steps(fused, tag="lp_4x24x32"):
    model = _model().to(DEV)
    x, t = _batch(tag)
    opt = SGD(model, **R.LP_SGD)
    if fused:
        tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=opt)
        _trainer_step(tr, x, t)
        pred, loss, _, am = _trainer_step(tr, x, t)
        assert model._get_engine()._last[0].ce not in (None, False)          # the fast path really ran
    else:
        _autograd_step(model, opt, x, t)
        pred, loss, _, am = _autograd_step(model, opt, x, t)
        assert not model._get_engine()._last[0].ce
    return pred, loss, am, {k: v.clone() for k, v in model.state_dict().items()}


def test_fused_step_equals_autograd_step_bit_for_bit():
    (pa, la, aa, sa), (pb, lb, ab, sb), (pc, lc, ac, sc) = _two_steps(True), _two_steps(False), _two_steps(True)
    assert torch.equal(pa, pb) and torch.equal(aa, ab) and la == lb
    for k in sa:
        assert torch.equal(sa[k], sb[k]), "fused vs autograd: " + k
        assert torch.equal(sa[k], sc[k]), "two fresh runs: " + k
    assert torch.equal(pa, pc)


def test_training_forward_takes_nhwc_memory_only():
    """A batch assembled the script's way (NCHW memory) trains after ``contiguous(memory_format=torch.channels_last)`` with the bits
    of the ``labelprop_batch`` batch; as it is, the training forward refuses it (no hidden re-layout pass); eval mode takes it."""
    tag = "lp_2x16x16"
    k = kats(tag)
    x_nchw, t = _t(k[tag + "/x"]).to(DEV), _t(k[tag + "/t"]).to(DEV)
    xb, tb = _batch(tag)
    assert torch.equal(xb, x_nchw) and torch.equal(tb, t) and x_nchw.is_contiguous() and not xb.is_contiguous()
    res = []
    for x in (xb, x_nchw.contiguous(memory_format=torch.channels_last)):
        model = _model().to(DEV)
        pred, loss, grads, _ = _autograd_step(model, SGD(model, **R.LP_SGD), x, t)
        res.append((pred, loss, model.state_dict()))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    for name in res[0][2]:
        assert torch.equal(res[0][2][name], res[1][2][name]), name
    model.train()
    with pytest.raises(L.RcvError, match="reads its input as NHWC memory"):
        model(x_nchw)
    tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=SGD(model, **R.LP_SGD))
    with pytest.raises(L.RcvError, match="reads its input as NHWC memory"):
        tr.step(x_nchw, t)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x_nchw), model(xb))


def test_five_steps_vs_torch_cpu_twin():
    tag = "lp_2x40x24"
    k = kats(tag)
    torch.manual_seed(12345678)
    twin = R.LabelPropTwin()
    model = _model()
    twin.load_state_dict(model.state_dict())
    model = model.to(DEV)
    im, lab = _t(k[tag + "/images"]), _t(k[tag + "/labels"])
    xc, tc_ = R.loop_assembly(im, lab)
    x, t = M.labelprop_batch(im.to(DEV), lab.to(DEV))
    assert torch.equal(x.cpu(), xc) and torch.equal(t.cpu(), tc_)
    tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=SGD(model, **R.LP_SGD))
    topt = torch.optim.SGD(twin.parameters(), **R.LP_SGD)
    crit = torch.nn.CrossEntropyLoss(torch.tensor(R.LP_WEIGHTS))
    twin.train()
    losses, ref_losses = [], []
    for _ in range(5):
        tr.step(x, t)
        losses.append(tr.pop_metrics()["loss"])
        topt.zero_grad()
        loss = crit(twin(xc), tc_)
        loss.backward()
        topt.step()
        ref_losses.append(float(loss.detach()))
    print("HIP  ", losses, "\ntwin ", ref_losses)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-2 * abs(b), (losses, ref_losses)
    assert abs(losses[0] - ref_losses[0]) <= 1e-3 * ref_losses[0]
    assert losses[-1] < 0.9 * losses[0], "the loss must fall"
    sd, ref = model.state_dict(), twin.state_dict()
    for name in ref:
        if ref[name].dtype.is_floating_point:
            err = float((sd[name].cpu().double() - ref[name].double()).norm() / (ref[name].double().norm() + 1e-30))
            assert err <= 2e-2, (name, err)
    assert int(sd["conv2.bn.num_batches_tracked"]) == 5


def test_prune_mask_step_vs_golden():
    tag = R.PRUNE_TAG
    m = META[tag]["prune"]
    model = _model().to(DEV)
    masks = R.prune_masks(list(model.parameters()))
    assert sum(int(q.sum()) for q in masks) == m["masked"]
    x, t = _batch(tag)
    for fused_opt in (True, False):
        model = _model().to(DEV)
        opt = SGD(model, **R.LP_SGD) if fused_opt else torch.optim.SGD(model.parameters(), **R.LP_SGD)
        tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=opt, prune_indices=masks)
        tr.step(x, t)
        assert abs(tr.pop_metrics()["loss"] - m["loss"]) <= 1e-3 * m["loss"]
        big = [p for p in model.parameters() if p.dim() > 1]
        if not fused_opt:          # the stock optimizer path zeroes the gradient views themselves (labelPropTrain.py:201-206)
            for p, q in zip(big, masks):
                assert float(p.grad[q.to(DEV)].abs().max()) == 0.0
            for name, p in model.named_parameters():
                if not (name.startswith("upConv") and name.endswith("conv.bias")):
                    n_ = m["grad_norm"][name]
                    tol = 1e-2 if (name.endswith("bn.weight") or name.endswith("bn.bias")) else 1e-3
                    assert abs(float(p.grad.double().norm()) - n_) <= tol * n_ + 1e-7, name
        _check_after(model.state_dict(), m["param_after_step_sum"], LR)
        # a masked weight moves by weight decay alone: p1 = p0 - lr * wd * p0
        torch.manual_seed(12345678)
        p0 = [p for p in M.LabelProp(5, 32, 0.0).parameters() if p.dim() > 1]
        for a, b0, q in zip(big, p0, masks):
            want = b0[q] * (1.0 - LR * R.LP_SGD["weight_decay"])
            assert float((a.detach().cpu()[q] - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9
