"""No GPU: tests/small_ops_restatement.py (the float64 yardstick of tests/test_gpu_small_ops.py and of the epilogue-statistics tests
of tests/test_gpu_kernels.py) against torch float64 autograd on ragged shapes, the integer-grid preconditions and the single-pixel
sensitivity of every exact GPU case (small_ops_cases), the plan-time refusal of RCV_OP_CONV1X1 (in the header, no kernel); the Adam
+ L1 restatement against torch.optim.Adam in float64, its rounding bound against an fp32 emulation of the kernel (inside) and against
seven wrong kernels (outside, each on a recorded share of the elements), the preconditions of the reduction and confusion cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_cases as K
import small_ops_restatement as R
from oracle import cpu_reference as O

T64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(T64)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert float(np.abs(a - b).max()) <= tol * (float(np.abs(b).max()) + 1.0), float(np.abs(a - b).max())


def _rows(cols, n_part, rng):
    """Column sums [2][C] spread over n_part partial rows that add up to them (the kernels' workspace)."""
    w = rng.random((n_part, 1, 1))
    return cols[None] * (w / w.sum())


@pytest.mark.parametrize("N,C,H,W", [(3, 8, 5, 7), (2, 16, 9, 11), (1, 4, 3, 5)])
@pytest.mark.parametrize("decoder", [False, True])
def test_batchnorm_statistics_finalize_backward_vs_autograd(N, C, H, W, decoder):
    """Encoder block conv -> ReLU -> BN (the BN input r is the ReLU output; BWD_ENC sums, GRAD_ENC load) and decoder block
    convT -> BN -> ReLU (BWD_DEC sums with the ReLU mask, GRAD_DEC load): batch statistics, normalisation constants, running
    statistics, dgamma / dbeta and the input gradient dx = A g + B + C r rebuilt from the bn_backward constants."""
    rng = np.random.default_rng(N * 100 + C + H)
    count = N * H * W
    x = rng.standard_normal((N, H, W, C)) * 1.5 + rng.standard_normal(C)
    gamma, beta = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C), rng.standard_normal(C)
    rm0, rv0 = rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
    gout = rng.standard_normal((N, H, W, C))
    eps, mom = 1e-5, 0.1
    xt = _t(x).permute(0, 3, 1, 2).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).to(T64)
    with torch.no_grad():
        bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta)); bn.running_mean.copy_(_t(rm0)); bn.running_var.copy_(_t(rv0))
    r_in = xt if decoder else torch.relu(xt)                 # the tensor the BatchNorm reads
    y = bn(r_in)
    out = torch.relu(y) if decoder else y
    out.backward(_t(gout).permute(0, 3, 1, 2))
    r = r_in.detach().permute(0, 2, 3, 1).numpy()
    fin = R.bn_finalize(_rows(R.stats(R.STATS_FWD, r), 7, rng), count, gamma, beta, rm0, rv0, mom, eps, True)
    _close(R.load(r, fin["consts"], R.LOAD_AFFINE), y.detach().permute(0, 2, 3, 1).numpy())
    _close(fin["consts"][2], r.reshape(-1, C).mean(0))
    _close(fin["running_mean"], bn.running_mean.numpy()); _close(fin["running_var"], bn.running_var.numpy())
    ev = F.batch_norm(_t(r).permute(0, 3, 1, 2), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, eps)
    ec = R.bn_eval(gamma, beta, fin["running_mean"], fin["running_var"], eps)
    _close(R.load(r, ec, R.LOAD_AFFINE), ev.detach().permute(0, 2, 3, 1).numpy())
    kind = R.STATS_BWD_DEC if decoder else R.STATS_BWD_ENC
    rows = _rows(R.stats(kind, gout, r, fin["consts"]), 5, rng)
    bwd = R.bn_backward(rows, count, gamma, fin["mean"], fin["istd"], fin["consts"])
    _close(bwd["dgamma"], bn.weight.grad.numpy(), 1e-10); _close(bwd["dbeta"], bn.bias.grad.numpy(), 1e-10)
    _close(bwd["consts"][3:], fin["consts"][:2], 0.0)
    if decoder:     # ReLU backward, then dx = A gm + B + C t
        dx = R.load(gout, bwd["consts"], R.LOAD_GRAD_DEC, aux=r)
        A, B, Cc = bwd["consts"][:3]
        _close(dx, A * np.where(r * fin["consts"][0] + fin["consts"][1] > 0, gout, 0.0) + B + Cc * r, 1e-13)
    else:           # dr = A g + B + C r, then the ReLU ahead of the BatchNorm
        dx = R.load(gout, bwd["consts"], R.LOAD_GRAD_ENC, aux=r)
    _close(dx, xt.grad.permute(0, 2, 3, 1).numpy(), 1e-10)


def test_bn_finalize_edges():
    """The variance clamp, eval mode / a missing running buffer (nothing updated), the folded bias row of bn_eval."""
    rows = np.zeros((3, 2, 2))
    rows[:, 0] = [[2.0, 1.0]] * 3              # mean 2 / 1 over count 3
    rows[:, 1] = [[3.0, 1.5]] * 3              # E[x^2] = 3 < 4: negative variance in exact arithmetic; 1.5 > 1: positive
    f = R.bn_finalize(rows, 3, [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0], 0.1, 1e-5, True)
    assert f["var"][0] == 0.0 and f["istd"][0] == 1.0 / np.sqrt(np.float64(1e-5)) and f["var"][1] == 0.5
    for kw in (dict(training=False), dict(training=True, running_mean=None)):
        args = dict(running_mean=np.ones(2), running_var=np.ones(2), momentum=0.1, eps=1e-5)
        args.update(kw)
        g = R.bn_finalize(rows, 3, [1.0, 1.0], [0.0, 0.0], **args)
        assert g["running_mean"] is args["running_mean"]
    # count == 1 (torch refuses a single value per channel in training): the running variance takes the biased value, 0
    one = R.bn_finalize(np.array([[[3.0], [9.0]]]), 1, [1.0], [0.0], [1.0], [2.0], 0.25, 1e-5, True)
    assert one["var"][0] == 0.0 and one["running_var"][0] == 1.5 and one["running_mean"][0] == 1.5
    e = R.bn_eval([2.0], [1.0], [3.0], [4.0 - 1e-5], 1e-5, [5.0])
    _close(e[:, 0], [1.0, -2.0, 0.0, 3.0, 0.0], 1e-15)
    assert R.bn_eval([2.0], [1.0], [3.0], [4.0 - 1e-5], 1e-5)[3, 0] == e[1, 0]


@pytest.mark.parametrize("C", [1, 2, 5, 8])
def test_cross_entropy_vs_torch(C):
    rng = np.random.default_rng(C)
    lg = rng.standard_normal((3, C, 5, 7)) * 2
    t = rng.integers(0, C, (3, 5, 7))
    t.reshape(-1)[::6] = -100
    w = rng.uniform(0.5, 4.0, C)
    lt = _t(lg).requires_grad_(True)
    loss = F.cross_entropy(lt, torch.from_numpy(t), weight=_t(w), ignore_index=-100)
    (3.0 * loss).backward()
    got = R.cross_entropy(lg, t, w, grad_out=3.0)
    _close(got["loss"], loss.item()); _close(got["dlogits"], lt.grad.numpy())
    assert np.array_equal(got["argmax"], lg.argmax(1)) and got["correct"] == int((lg.argmax(1) == t).sum())
    t2 = t.copy()
    t2[t == -100] = C + 3                     # any label outside [0, C) is ignored alike
    got2 = R.cross_entropy(lg, t2, w, grad_out=3.0)
    assert got2["loss"] == got["loss"] and np.array_equal(got2["dlogits"], got["dlogits"])
    un = R.cross_entropy(lg, t, None)
    _close(un["loss"], F.cross_entropy(_t(lg), torch.from_numpy(t), ignore_index=-100).item())


@pytest.mark.parametrize("C", [2, 3, 5, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_dice_vs_oracle(C, weighted):
    """The reference's DiceLoss (oracle.cpu_reference.dice_loss, float64).  For a label outside [0, C) the reference's
    torch.eye(C)[label] raises (label >= C or < -C) or wraps (-C..-1); the kernels give such a pixel an all-zero one-hot row, which
    is what the restatement states and what this test pins: equal to the oracle on a target whose one-hot rows are zeroed there."""
    rng = np.random.default_rng(10 + C)
    lg = rng.standard_normal((2, C, 7, 5)) * 2
    t = rng.integers(0, C, (2, 7, 5))
    w = O.dice_weights(_t(rng.uniform(0.5, 4.0, C))) if weighted else torch.ones(C, dtype=T64)
    lt = _t(lg).requires_grad_(True)
    loss = O.dice_loss(lt, torch.from_numpy(t), w, 1e-7)
    (2.0 * loss).backward()
    got = R.dice(lg, t, w.numpy(), 1e-7, grad_out=2.0)
    _close(got["loss"], loss.item()); _close(got["dlogits"], lt.grad.numpy())
    # A_c, B_c: d loss / d P = A_c [t == c] + B_c, against autograd through the probabilities
    p = torch.softmax(_t(lg), 1).requires_grad_(True)
    hot = F.one_hot(torch.from_numpy(t), C).permute(0, 3, 1, 2).to(T64)
    l2 = 1 - (2.0 * w * (p * hot).sum((0, 2, 3)) / ((p + hot).sum((0, 2, 3)) + 1e-7)).mean()
    l2.backward()
    _close(got["A"][None, :, None, None] * hot.numpy() + got["B"][None, :, None, None], p.grad.numpy())
    # labels outside [0, C)
    t2 = t.copy()
    out = np.zeros(t.shape, bool)
    out.reshape(-1)[::5] = True
    t2[out] = np.where(np.arange(out.sum()) % 2 == 0, -100, C + 1)
    hot2 = hot * _t(~out)[:, None]
    lt2 = _t(lg).requires_grad_(True)
    p2 = torch.softmax(lt2, 1)
    l3 = 1 - (2.0 * w * (p2 * hot2).sum((0, 2, 3)) / ((p2 + hot2).sum((0, 2, 3)) + 1e-7)).mean()
    l3.backward()
    got3 = R.dice(lg, t2, w.numpy(), 1e-7)
    _close(got3["loss"], l3.item()); _close(got3["dlogits"], lt2.grad.numpy())


@pytest.mark.parametrize("mode2", [None, R.LOAD_PLAIN, R.LOAD_AFFINE, R.LOAD_AFFINE_RELU])
def test_classifier_vs_conv2d(mode2):
    rng = np.random.default_rng(5)
    N, H, W, K, C = 2, 5, 7, 8, 5
    t, r = rng.standard_normal((N, H, W, K)), rng.standard_normal((N, H, W, K))
    tc, rc = rng.standard_normal((5, K)), rng.standard_normal((5, K))
    w, b, dl = rng.standard_normal((C, K)), rng.standard_normal(C), rng.standard_normal((N, C, H, W))
    tt, rt = _t(t).requires_grad_(True), _t(r)
    if mode2 is None:
        up_t = tt
        up = t
    else:
        fr = rt if mode2 == R.LOAD_PLAIN else rt * _t(rc[0]) + _t(rc[1])
        up_t = torch.relu(tt * _t(tc[0]) + _t(tc[1])) + (torch.relu(fr) if mode2 == R.LOAD_AFFINE_RELU else fr)
        up = R.fused_up(t, tc, r, rc, mode2)
        _close(up, up_t.detach().numpy())
    up_t = up_t.permute(0, 3, 1, 2)
    up_t.retain_grad()
    wt, bt = _t(w).requires_grad_(True), _t(b).requires_grad_(True)
    lg = F.conv2d(up_t, wt[:, :, None, None], bt)
    lg.backward(_t(dl))
    _close(R.cls_forward(up, w, b), lg.detach().numpy())
    d_up, dW, db = R.cls_backward(up, dl, w)
    _close(d_up, up_t.grad.permute(0, 2, 3, 1).numpy()); _close(dW, wt.grad.numpy()); _close(db, bt.grad.numpy())
    keep = np.ones(N * H * W, bool)
    keep[-1] = False
    assert np.all(R.cls_backward(up, dl, w, keep)[2] != db)


@pytest.mark.parametrize("affine", [False, True])
def test_maxpool_vs_torch(affine):
    rng = np.random.default_rng(3)
    N, H, W, C = 2, 6, 10, 8
    r = R.grid(rng, (N, H, W, C), 2)                       # ties in most windows
    c = R.grid_consts(rng, C, scales=(0.5, -0.5, 2.0, -2.0))
    mode = R.LOAD_AFFINE if affine else R.LOAD_PLAIN
    dp, res = rng.standard_normal((N, H // 2, W // 2, C)), rng.standard_normal((N, H, W, C))
    v = _t(R.load(r, c, mode)).permute(0, 3, 1, 2).requires_grad_(True)
    y = F.max_pool2d(v, 2, 2)
    y.backward(_t(dp).permute(0, 3, 1, 2))
    _close(R.pool_forward(r, c, mode), y.detach().permute(0, 2, 3, 1).numpy(), 0.0)
    _close(R.pool_backward(dp, r, c, mode, res), v.grad.permute(0, 2, 3, 1).numpy() + res, 0.0)


def test_sgd_vs_torch():
    rng = np.random.default_rng(9)
    n = 1001
    p0 = rng.standard_normal(n)
    ref = torch.nn.Parameter(_t(p0).clone())
    opt = torch.optim.SGD([ref], lr=0.2, momentum=0.5, weight_decay=1e-3)
    p, buf = p0.copy(), np.zeros(n)
    lre = np.full(n, 0.2)
    lre[::7] = 0.0
    q, qbuf = p0.copy(), np.full(n, 7.0)
    for step in (1, 2, 3):
        g = rng.standard_normal(n)
        ref.grad = _t(g) * 0.25
        opt.step()
        p, buf = R.sgd_step(p, g, buf, step, 0.2, 0.5, 1e-3, grad_scale=0.25)
        _close(p, ref.detach().numpy(), 1e-14)
        q, qbuf = R.sgd_step(q, g, qbuf, step, 0.2, 0.5, 1e-3, grad_scale=0.25, lr_elem=lre)
    assert np.array_equal(q[::7], p0[::7]) and np.all(qbuf[::7] == 7.0)
    live = lre != 0
    _close(q[live], p[live], 1e-14)


def test_load_modes_and_statistics_definitions():
    rng = np.random.default_rng(1)
    x, a, c = rng.standard_normal((2, 3, 4, 8)), rng.standard_normal((2, 3, 4, 8)), rng.standard_normal((5, 8))
    assert np.array_equal(R.load(x, c, R.LOAD_GRAD_ENC, a), np.where(a > 0, c[0] * x + c[1] + c[2] * a, 0.0))
    assert np.array_equal(R.load(x, c, R.LOAD_AFFINE_RELU), np.maximum(x * c[0] + c[1], 0))
    v, e, ec = R.grid(rng, (2, 3, 4, 8)), R.grid(rng, (2, 3, 4, 8)), R.grid_consts(rng, 8, rows=3)
    m = (e * ec[0] + ec[1]) > 0
    assert ((e * ec[0] + ec[1]) == 0).any()
    s = R.stats(R.STATS_BWD_DEC, v, e, ec)
    assert np.array_equal(s[0], (v * m).sum((0, 1, 2))) and np.array_equal(s[1], (v * m * (e - ec[2])).sum((0, 1, 2)))
    s = R.stats(R.STATS_BWD_ENC, v, e, ec)
    assert np.array_equal(s[1], (v * (e - ec[2])).sum((0, 1, 2)))
    assert np.array_equal(R.stats(R.STATS_FWD, v)[1], (v.astype(np.float64) ** 2).sum((0, 1, 2)))


# ------------------------------------------------------------------------------------------ preconditions of the exact GPU cases
CUS = 256       # the planes beyond one grid pass are sized by rcv_num_cus on the device; the preconditions are asserted for 256 CUs here


def test_big_planes_for_256_cus():
    b = K.big_planes(CUS)
    assert b["reducing"] == [(2, 360, 368), (3, 297, 295)] and b["streaming"][0] == (2, 520, 512)
    for name, per_cu in (("reducing", 4), ("streaming", 8)):
        for n, h, w in b[name]:
            assert n * h * w > 256 * per_cu * CUS


@pytest.mark.parametrize("nC", range(1, 9))
def test_classifier_cases_are_exact_and_sensitive(nC):
    cases = [c for c in K.cls_case_list(CUS) if c[1] == nC]
    assert len(cases) >= 20
    for case in cases:
        K.check_cls(K.build_cls(*case))


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("resid", [False, True])
def test_pool_cases_are_exact_and_sensitive(affine, resid):
    small, big, cap = K.pool_cases(CUS)
    for N, H, W, C in small:
        K.check_pool(K.build_pool(N, H, W, C, affine, resid))
    for N, H, W, C in big:
        assert N * (H // 2) * (W // 2) * (C // 4) > cap
        K.check_pool(K.build_pool(N, H, W, C, affine, resid, second_item=cap))


def test_bwd_stats_cases_are_exact_and_sensitive():
    cap = 256 * 4 * CUS
    for Csrc, coff, C in K.BWD_STATS_SLICES:
        for plane in K.PLANES:
            K.check_bwd_stats(K.build_bwd_stats(plane, Csrc, coff, C))
    plane = K.big_planes(CUS)["reducing"][1]
    assert plane[0] * plane[1] * plane[2] * 2 > cap
    K.check_bwd_stats(K.build_bwd_stats(plane, 16, 8, 8, second_item=cap))


@pytest.mark.parametrize("family", ["conv", "tconv", "image", "tiny", "dilated"])
def test_conv_statistics_cases_are_exact(family):
    shapes = dict(conv=K.CONV_STATS_SHAPES, tconv=K.TCONV_STATS_SHAPES, image=K.IMAGE_STATS_SHAPES, tiny=K.TINY_STATS_SHAPES,
                  dilated=K.DILATED_STATS_SHAPES)[family]
    for shape in shapes:
        K.check_conv_stats(K.build_conv_stats(shape, transposed=family == "tconv", nchw=family == "image"))


@pytest.mark.parametrize("k", range(len(K.MULTI_ROUND_STATS_CASES)))
def test_multi_round_statistics_cases_are_exact_row_by_row(k):
    """The multi-round planes are too large for check_conv_stats' bound on the whole sum; each partial row stays exact."""
    case = K.MULTI_ROUND_STATS_CASES[k]
    K.check_multi_round_stats(K.build_conv_stats(case[1], transposed=case[0] == "tconv", nchw=case[0] == "image"), case)


def test_conv1x1_is_refused_when_planned():
    """RCV_OP_CONV1X1 is in the header and has no kernel: rcv_op_workspace refuses it with a message; nothing is launched."""
    from robocupvision_amd import _lib as L
    h = L.planner_handle(CUS)
    op = L.make_op(L.OP_CONV1X1, L.F_OUT_NCHW, n=1, h=4, w=4, cin=16, cout=5)
    with pytest.raises(L.RcvError) as ei:
        L.op_workspace(h, op)
    assert "(-1)" in str(ei.value) and "18" in str(ei.value), str(ei.value)
    with pytest.raises(L.RcvError):
        L.OpList([op]).labels(h)


# ------------------------------------------------------------------------------------------ Adam + L1
def _adam_case(case):
    if case not in _adam_case.cache:
        c = K.build_adam(*case)
        _adam_case.cache[case] = (c, {form: K.adam_reference(c, form) for form in K.ADAM_FORMS})
    return _adam_case.cache[case]


_adam_case.cache = {}


def test_adam_cases_cover_every_step_scale_and_size():
    cases = K.adam_cases(CUS)
    big = K.adam_big_n(CUS)
    assert big == 529291 and big % 4 == 3 and big > 2 * CUS * 256 * 4
    assert {c[0] for c in cases} == {1, 3, 4, 5, 255, 1027, 100003, big} and {c[1] for c in cases} == set(K.ADAM_T)
    assert {c[2] for c in cases if c[0] == big} == set(K.ADAM_GS)
    c = K.build_adam(big, 1000, 0.125)
    z = (c["g"] == 0) & (c["m"] == 0) & (c["v"] == 0)
    assert (z & (c["p"] == 0) & np.signbit(c["p"])).any() and (z & (c["p"] == 0) & ~np.signbit(c["p"])).any() and (z & (c["p"] != 0)).any()
    assert set(np.unique(c["lr_elem"]).tolist()) == {0.0, float(c["lr"]), float(np.float32(10) * c["lr"])}
    assert 0.2 < c["prune"].mean() < 0.3 and np.abs(c["g"][c["g"] != 0]).min() < 1e-9 and np.abs(c["g"]).max() > 0.5
    quad = c["lr_elem"][:big // 4 * 4].reshape(-1, 4)
    assert ((quad == 0).any(1) & (quad != 0).any(1)).any(), "a float4 must straddle a stepped and an unstepped stretch"


def test_adam_restatement_vs_torch_adam():
    """(a) R.adam_l1_step = torch.optim.Adam in float64 on the gradient g gs + decay sign(p), betas and eps the fp32-rounded values,
    steps 1..3, to a few float64 ulps once bc1 / bc2_sqrt are left unrounded; a pruned element is one whose whole gradient is 0;
    lr_elem == 0 leaves the element alone with a zero bound."""
    rng = np.random.default_rng(77)
    n = 2003
    c = K.build_adam(n, 2, 1.0 / 3)
    h = {k: float(c[k]) for k in ("lr", "b1", "b2", "eps", "decay", "gs")}
    for pruned in (False, True):
        ref = torch.nn.Parameter(_t(c["p"]).clone())
        opt = torch.optim.Adam([ref], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"])
        p, m, v = c["p"].astype(np.float64), np.zeros(n), np.zeros(n)
        worst = 0.0
        for step in (1, 2, 3):
            g = (K._logu(rng, n, 1e-10, 1.0) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
            grad = _t(g) * h["gs"] + h["decay"] * torch.sign(ref.detach())
            ref.grad = torch.where(torch.from_numpy(c["prune"] != 0), torch.zeros_like(grad), grad) if pruned else grad
            p_prev, m_prev = p, m
            opt.step()
            (p, m, v), _ = R.adam_l1_step(p, g, m, v, step, c["lr"], c["b1"], c["b2"], c["eps"], c["decay"], c["gs"],
                                          prune=c["prune"] if pruned else None, round_bc=False)
            st = opt.state[ref]
            # scales: the sums of |terms| (m' may cancel; what it loses goes into p' through step / denom)
            sm = np.abs(m_prev) + np.abs(g.astype(np.float64) * h["gs"]) + h["decay"]
            sp = np.abs(p_prev) + h["lr"] / (1 - h["b1"] ** step) * sm / (np.sqrt(v) / np.sqrt(1 - h["b2"] ** step) + h["eps"])
            for got, want, scale in ((p, ref.detach().numpy(), sp), (m, st["exp_avg"].numpy(), sm), (v, st["exp_avg_sq"].numpy(), np.abs(v))):
                err = np.abs(got - want)
                worst = max(worst, float((err / np.maximum(scale, 1e-300)).max()))
                assert np.all(err <= 1e-14 * scale), float((err / np.maximum(scale, 1e-300)).max())
        print("adam restatement vs torch.optim.Adam (pruned=%d): largest relative difference %.2e" % (pruned, worst))
    # rounding bc1 / bc2_sqrt to fp32 moves the step by at most 2^-24 relative each
    a, _ = R.adam_l1_step(c["p"], c["g"], c["m"], c["v"], 2, c["lr"], c["b1"], c["b2"], c["eps"], c["decay"], c["gs"])
    b, _ = R.adam_l1_step(c["p"], c["g"], c["m"], c["v"], 2, c["lr"], c["b1"], c["b2"], c["eps"], c["decay"], c["gs"], round_bc=False)
    assert np.all(np.abs(a[0] - b[0]) <= 2.1 * 2.0 ** -24 * np.abs(b[0] - c["p"])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # lr_elem == 0
    (p1, m1, v1), (ep, em, ev) = K.adam_reference(c, "lr_elem")
    dead = c["lr_elem"] == 0
    assert dead.any() and np.array_equal(p1[dead], c["p"][dead]) and np.array_equal(np.signbit(p1[dead]), np.signbit(c["p"][dead]))
    assert np.array_equal(m1[dead], c["m"][dead]) and np.array_equal(v1[dead], c["v"][dead])
    assert not ep[dead].any() and not em[dead].any() and not ev[dead].any() and (ep[~dead & (c["p"] != 0)] > 0).all()
    # a pruned element: gr = 0 exactly, the moments only decay
    (_, m2, v2), _ = K.adam_reference(c, "lr_elem+prune")
    pr = (c["prune"] != 0) & ~dead
    assert np.array_equal(m2[pr], np.float64(c["b1"]) * c["m"][pr]) and np.array_equal(v2[pr], np.float64(c["b2"]) * c["v"][pr])


def test_adam_fp32_emulation_stays_inside_the_bound():
    """(b) the kernel's expression order in fp32 numpy, uncontracted and with either contraction of a b + c d (and of p - step r),
    stays inside the running bound on every case and record form.  The p bound is mostly the final rounding of p itself."""
    worst = np.zeros(3)
    for case in K.adam_cases(CUS):
        c, refs = _adam_case(case)
        for form in K.ADAM_FORMS:
            ref, bound = refs[form]
            for contract in (0, 1, 2):
                got = K.adam_emulate(c, form, contract)
                rat = K.adam_ratios(got, ref, bound)
                for k, name in enumerate("pmv"):
                    assert np.all(rat[k] <= 1.0), "%s %s contraction %d: %s leaves the bound (%.3f)" % (case, form, contract, name, rat[k].max())
                worst = np.maximum(worst, [r.max() for r in rat])
                if form != "plain":
                    dead = c["lr_elem"] == 0
                    assert all(np.array_equal(a[dead], c[k][dead]) for a, k in zip(got, "pmv"))
    print("adam fp32 emulation: largest error / bound p %.3f m %.3f v %.3f" % tuple(worst))
    assert worst.min() > 0.3, "a bound nothing comes near is no bound"


@pytest.mark.parametrize("mutant", sorted(K.ADAM_MUTANTS))
def test_adam_wrong_variants_leave_the_bound(mutant):
    """(c) every wrong kernel of K.ADAM_MUTANTS puts its recorded share of the live elements outside TWICE the bound in at least one
    case (whichever way the compiler contracts), so the GPU test would see it."""
    form, best = "lr_elem+prune", 0.0
    for case in K.adam_cases(CUS):
        if case[0] < 1027:
            continue
        c, refs = _adam_case(case)
        ref, bound = refs[form]
        live = c["lr_elem"] != 0
        share = 1.0
        for contract in (0, 1, 2):
            rat = K.adam_ratios(K.adam_emulate(c, form, contract, mutant), ref, bound)
            out = ~(rat[0] <= 2.0) | ~(rat[1] <= 2.0) | ~(rat[2] <= 2.0)           # NaN and inf count as outside
            share = min(share, float(out[live].mean()))
        print("adam mutant %s, case %s: %.3f of the live elements outside twice the bound" % (mutant, case, share))
        best = max(best, share)
    assert best >= K.ADAM_MUTANTS[mutant], (mutant, best)


# ------------------------------------------------------------------------------------------ filter-gradient reductions
def test_wgrad_reduce_restatement_layout():
    rng = np.random.default_rng(4)
    ns, CB, CA = 3, 5, 3
    CBP, CAP = K.reduce_pads(CB, CA)
    assert (CBP, CAP) == (16, 4) and K.reduce_pads(16, 8) == (16, 16) and K.reduce_pads(64, 32) == (64, 32) and K.reduce_pads(8, 4) == (16, 4)
    part, bias = rng.standard_normal((ns, 9, CBP, CAP)), rng.standard_normal((ns, CBP))
    dw, db = R.wgrad_reduce(part, bias, CB, CA)
    assert dw.shape == (CB, CA, 3, 3) and db.shape == (CB,)
    for cb in range(CB):
        assert db[cb] == bias[:, cb].sum()
        for ca in range(CA):
            for tap in range(9):
                assert dw[cb, ca, tap // 3, tap % 3] == part[:, tap, cb, ca].sum()
    assert R.wgrad_reduce(part, None, CB, CA)[1] is None
    assert K.reduce_blocks(16, 8, True) == 37 and K.reduce_blocks(8, 3, False) == 9 and K.reduce_blocks(64, 32, True) == 289
    c = K.build_reduce(2, CB, CA, "weights")
    buf = K.reduce_buffer(c, True)
    assert buf.size == 3 * (9 * CBP * CAP + CBP) and np.isnan(buf[2 * (9 * CBP * CAP + CBP):]).all()
    assert np.array_equal(buf[2 * 9 * CBP * CAP:2 * 9 * CBP * CAP + 2 * CBP], c["bias"].reshape(-1), equal_nan=True)


@pytest.mark.parametrize("CB,CA", K.REDUCE_SHAPES + (K.REDUCE_WIDE[0],))
def test_wgrad_reduce_cases_are_exact_sensitive_and_out_of_fp32_reach(CB, CA):
    """Both exact kinds: integer sums below 2^24; "weights": every split moves every entry; "cancel": the kernel's own order of
    additions, done in fp32, misses at least the recorded share of the entries (so only a double accumulation passes)."""
    for ns in (K.REDUCE_NSPLIT if (CB, CA) != K.REDUCE_WIDE[0] else K.REDUCE_WIDE[1]):
        w = K.build_reduce(ns, CB, CA, "weights")
        K.check_reduce(w)
        dw, db = K.reduce_reference(w)
        assert np.array_equal(K.reduce_fixed_order_fp32(w["part"][:, :, :CB, :CA]).transpose(1, 2, 0).reshape(dw.shape), dw)
        assert np.array_equal(K.reduce_fixed_order_fp32(w["bias"][:, :CB]), db), "the emulated order must add every split once"
        c = K.build_reduce(ns, CB, CA, "cancel")
        K.check_reduce(c)
        miss = K.reduce_fp32_miss(c)
        print("wgrad_reduce (%d, %d) nsplit %d: an fp32 accumulation misses %.3f of the entries" % (CB, CA, ns, miss))
        assert miss >= K.REDUCE_FP32_MISS[ns], (ns, miss)


# ------------------------------------------------------------------------------------------ confusion counts
@pytest.mark.parametrize("C", K.CONF_CLASSES)
def test_confusion_restatement_and_cases(C):
    for N, H, W in K.confusion_planes():
        pred, tgt = K.build_confusion(N, H, W, C)
        ref = R.confusion(pred, tgt, C)
        slow = np.zeros((N, C, C), np.int64)
        for n in range(min(N, 2)):
            for p, t in zip(pred[n].reshape(-1).tolist()[:3000], tgt[n].reshape(-1).tolist()[:3000]):
                if p < C and 0 <= t < C:
                    slow[n, p, t] += 1
        if H * W <= 3000:
            assert np.array_equal(ref[:2], slow[:2])
        ok = (pred < C) & (tgt >= 0) & (tgt < C)
        assert np.array_equal(ref.sum((1, 2)), ok.reshape(N, -1).sum(1))
        if N * H * W >= 6:
            assert {int(x) for x in tgt.reshape(-1)[~ok.reshape(-1)]} >= {C if x is None else x for x in K.CONF_ODD_LABELS}
            assert (pred >= C).any()
            # a 32-bit truncation of the labels would count 2^32 + 1 as class 1 and -2^32 + 2 as class 2
            if C > 1:
                assert not np.array_equal(R.confusion(pred, tgt.astype(np.int32), C), ref)
        if C > 1 and H * W > 1:
            assert ref[-1, C - 1, 0] == 1 and pred[-1, -1, -1] == C - 1 and tgt[-1, -1, -1] == 0
    one = R.confusion(np.array([[[0]], [[1]]], np.uint8), np.array([[[2 ** 32]], [[1]]], np.int64), 2)
    assert one.tolist() == [[[0, 0], [0, 0]], [[0, 0], [0, 1]]]
