"""GPU: the training-step form of the fused 1x1 classifier -- RCV_OP_CE_NORM + RCV_OP_CLS_STEP (cls_bwd_kernel<8, 1..8, true, true, ClsStepArgs>, ce_norm_kernel,
cls_step_tail_kernel; csrc/small_kernels.hip) -- against the two records it replaces, RCV_OP_CLS_FWD and RCV_OP_CLS_BWD with
RCV_F_FUSED_UP | RCV_F_FUSED_CE, run on the same operands in the same process.  Those two are pinned against float64 and the goldens
by test_gpu_small_ops.py, test_gpu_blocks.py and test_gpu_net.py; here everything is `torch.equal`: logits, arg-max, the four
loss_out values, d_up, dW, db, the statistics rows, the filter rows and the loss rows.

Shapes: 1x5x7 (35 pixels: one partial wave, the per-pixel store path), 2x8x16 (256 pixels: the whole-line store path, one
workgroup), 1x480x640 (307 200 pixels on a grid of 4 workgroups per CU: on 256 CUs some threads take two grid-stride passes and the
last pass re-requests its own pixel).  Targets hold -100 and, below 8 classes, a label in [C, 8)."""
import numpy as np
import pytest
import torch

from oracle import cpu_reference as O
from robocupvision_amd import _lib as L
from test_gpu_blocks import _t
from test_gpu_net import CE_W, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (L.LOAD_PLAIN, L.LOAD_AFFINE, L.LOAD_AFFINE_RELU)


def _h():
    return L.handle(0)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _ws(op):
    ws = _nan(max(L.op_workspace(_h(), op) // 4, 1))
    op.p[L.RCV_P_PART] = ws.data_ptr()
    return ws


def _run(*ops):
    L.OpList(list(ops)).run(_h(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


def _operands(plane, nC, seed):
    N, H, W = plane
    rng = np.random.default_rng(seed)
    t, r = (rng.standard_normal((N, H, W, 8)).astype(np.float32) for _ in range(2))
    tc, rc = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    tc[0], tc[1], tc[2] = rng.uniform(0.5, 1.5, 8) * rng.choice([-1, 1], 8), rng.standard_normal(8) * 0.3, rng.standard_normal(8) * 0.2
    rc[0], rc[1] = rng.uniform(0.5, 1.5, 8), rng.standard_normal(8) * 0.3
    w, b = (rng.standard_normal((nC, 8)) * 0.5).astype(np.float32), (rng.standard_normal(nC) * 0.1).astype(np.float32)
    tgt = rng.integers(0, nC, (N, H, W)).astype(np.int64)
    flat = tgt.reshape(-1)
    flat[::37] = -100
    if nC < 8:
        flat[5::41] = nC + (seed % (8 - nC))
    flat[1] = 0                                              # at least one valid label: the normaliser is not zero
    assert (flat == -100).any() and ((flat >= 0) & (flat < nC)).any() and (nC == 8 or ((flat >= nC) & (flat < 8)).any())
    cw = rng.uniform(0.5, 6.0, nC).astype(np.float32)
    d = {k: _dev(v) for k, v in dict(t=t, r=r, tc=tc, rc=rc, w=w, b=b, cw=cw).items()}
    d["tgt"], d["one"] = _dev(tgt, torch.int64), torch.ones(1, device=DEV)
    return d


def _both_paths(plane, nC, mode2, d, weights, bias):
    """Outputs of (CLS_FWD, CLS_BWD) and of (CE_NORM, CLS_STEP) on the operands `d`, as two dicts of tensors."""
    N, H, W = plane
    cw = d["cw"].data_ptr() if weights else 0
    b = d["b"].data_ptr() if bias else 0
    kw = dict(n=N, h=H, w=W, cin=8, cout=nC, aux0=mode2, p_w=d["w"].data_ptr(), p_x3=d["r"].data_ptr(), p_x4=d["rc"].data_ptr(), p_bias=b,
              p_in2=d["tgt"].data_ptr(), p_x0=cw)
    both = L.F_FUSED_UP | L.F_FUSED_CE
    res = []
    for fused in (False, True):
        o = dict(logits=_nan(N, nC, H, W), argmax=torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV), loss=_nan(4),
                 d_up=_nan(N, H, W, 8), dW=_nan(nC, 8), db=_nan(nC))
        bkw = dict(stats=L.STATS_BWD_DEC, p_out=o["d_up"].data_ptr(), p_epi_aux=d["t"].data_ptr(), p_epi_c=d["tc"].data_ptr(),
                   p_x1=o["dW"].data_ptr(), p_x2=o["db"].data_ptr(), p_x5=o["loss"].data_ptr(), p_in2_aux=d["one"].data_ptr(), **kw)
        if not fused:
            f = L.make_op(L.OP_CLS_FWD, both, p_in=d["t"].data_ptr(), p_in_c=d["tc"].data_ptr(), p_out=o["logits"].data_ptr(),
                          p_x1=o["loss"].data_ptr(), p_x2=o["argmax"].data_ptr(), **kw)
            ce_rows = _ws(f)
            bop = L.make_op(L.OP_CLS_BWD, both, **bkw)
            ws = _ws(bop)
            assert f.i[L.RCV_I_NPART] == bop.i[L.RCV_I_NPART]
            _run(f, bop)
        else:
            norm = L.make_op(L.OP_CE_NORM, 0, n=N, h=H, w=W, cout=nC, p_in2=d["tgt"].data_ptr(), p_x0=cw)
            norm_rows = _ws(norm)
            bop = L.make_op(L.OP_CLS_STEP, both, p_resid=o["logits"].data_ptr(), p_in_aux=o["argmax"].data_ptr(), **bkw)
            ws = _ws(bop)
            ce_rows = _nan(bop.i[L.RCV_I_NPART] * 3)
            bop.p[L.RCV_P_IN2_C], bop.p[L.RCV_P_IN_C] = ce_rows.data_ptr(), norm_rows.data_ptr()
            assert norm.i[L.RCV_I_NPART] == bop.i[L.RCV_I_NPART]
            assert L.OpList([norm, bop]).labels(_h()) == ["ce_norm", "cls_step"]
            _run(norm, bop)
            o["norm_rows"] = norm_rows[:norm.i[L.RCV_I_NPART]]
        g, wrow = bop.i[L.RCV_I_NPART], nC * 8 + nC
        o["stat_rows"], o["w_rows"], o["ce_rows"] = ws[:g * 16], ws[g * 16:g * (16 + wrow)], ce_rows[:g * 3]
        assert ws.numel() == g * (16 + wrow)
        res.append(o)
    return res


def _assert_same(two, fused, what):
    for k in ("logits", "argmax", "loss", "d_up", "dW", "db", "stat_rows", "w_rows", "ce_rows"):
        a, b = two[k], fused[k]
        assert not bool(torch.isnan(a.float()).any()), what + k + ": the two-record path left a value unwritten"
        assert a.shape == b.shape and torch.equal(a, b), "%s%s differs: %d of %d entries" % (what, k, int((a != b).sum()), a.numel())
    assert torch.equal(fused["norm_rows"], two["ce_rows"].reshape(-1, 3)[:, 1]), what + "normaliser rows are not the forward's a_w column"
    assert float(two["loss"][1]) > 0


@pytest.mark.parametrize("plane", [(1, 5, 7), (2, 8, 16)])
@pytest.mark.parametrize("nC", [1, 5, 8])
def test_step_record_equals_the_two_records(plane, nC):
    d = _operands(plane, nC, seed=900 + 10 * nC + plane[0])
    for mode2 in MODES:
        for weights in (False, True):
            for bias in (False, True):
                two, fused = _both_paths(plane, nC, mode2, d, weights, bias)
                _assert_same(two, fused, "cls_step %s %d classes mode %d weights %d bias %d: " % (plane, nC, mode2, weights, bias))


def test_step_record_equals_the_two_records_beyond_one_grid_pass():
    plane, nC = (1, 480, 640), 5
    d = _operands(plane, nC, seed=77)
    two, fused = _both_paths(plane, nC, L.LOAD_AFFINE, d, True, True)
    _assert_same(two, fused, "cls_step %s: " % (plane,))


# ------------------------------------------------------------------------------------------ whole steps
def _two_steps(x, t, monkeypatch, off):
    from robocupvision_amd.train import Trainer
    if off:
        monkeypatch.setenv("RCV_NO_FUSED_CLS_STEP", "1")
    else:
        monkeypatch.delenv("RCV_NO_FUSED_CLS_STEP", raising=False)
    model = build(dict(noScale=True)).to(DEV)
    tr = Trainer(model, class_weights=CE_W, lr=1e-3, decay=1e-6)
    tr.step(x, t)
    pred = tr.step(x, t).clone()
    eng = model._get_engine()
    ce = eng._last[0].ce
    assert ce and ce["step"] is not None
    ran = ce["ran"]
    assert (ran is ce["step"]) == (not off) and (ran is ce) == off          # the fused record really ran / really did not
    labels = ran["fwd"].labels(eng.handle) + ran["bwd"].labels(eng.handle)
    assert ("cls_step" in labels and "ce_norm" in labels and "cls_bwd" not in labels and "cls_fwd" not in labels) == (not off)
    assert ("cls_bwd" in labels and "cls_fwd" in labels and "cls_step" not in labels) == off
    torch.cuda.synchronize()
    return (tr.pop_metrics(), pred, tr.criterion.last_argmax.clone(), tr.criterion.last_stats.clone(),
            {k: v.clone() for k, v in model.state_dict().items()})


@pytest.mark.parametrize("batch", ["golden_1x48x64", "seeded_2x48x64"])
def test_trainer_step_is_bitwise_the_two_record_step(batch, net_kats, monkeypatch):
    """Two Trainer steps with RCV_NO_FUSED_CLS_STEP=1 and without: equal metrics, logits, arg-max, loss row, every parameter and
    every BatchNorm buffer."""
    if batch.startswith("golden"):
        x, t = _t(net_kats["robo_l_1x48x64/x"]), _t(net_kats["robo_l_1x48x64/t"])
    else:
        x, t = O.synthetic_batch(2, 48, 64, seed=3)
    x, t = x.to(DEV), t.to(DEV)
    (ma, pa, aa, la, sa), (mb, pb, ab, lb, sb) = (_two_steps(x, t, monkeypatch, off) for off in (True, False))
    assert ma == mb, (ma, mb)
    assert torch.equal(pa, pb) and torch.equal(aa, ab) and torch.equal(la, lb)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_captured_step_with_the_fused_record_equals_an_eager_step(monkeypatch):
    from robocupvision_amd.train import Trainer
    monkeypatch.delenv("RCV_NO_FUSED_CLS_STEP", raising=False)
    x, t = O.synthetic_batch(2, 48, 64, seed=3)
    x, t = x.to(DEV), t.to(DEV)
    out = []
    for graph in (False, True):
        model = build(dict(noScale=True)).to(DEV)
        tr = Trainer(model, class_weights=CE_W, lr=1e-3, decay=1e-6)
        for _ in range(2):
            tr.step(x, t)
        tr.optimizer.use_device_step()                 # (both runs read the step number from the device: same arithmetic)
        if graph:
            step = tr.capture(x, t)
        else:
            tr.step(x, t)                              # capture() runs one eager step itself: the eager run takes it here
            step = tr.step
        tr.pop_metrics()
        pred = step(x, t).clone()
        torch.cuda.synchronize()
        ce = model._get_engine()._last[0].ce
        assert ce["ran"] is ce["step"]
        out.append((tr.pop_metrics(), pred, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (ma, pa, sa), (mb, pb, sb) = out
    assert ma == mb, (ma, mb)
    assert torch.equal(pa, pb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
