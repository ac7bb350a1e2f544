"""GPU: the kernels around the 3x3 contractions, one op record at a time through rcv_run, against the float64 restatement
(tests/small_ops_restatement.py; cases and their CPU-side preconditions in tests/small_ops_cases.py).

Exact cases draw their operands from a small integer grid (values in {-2..2}, scales +-2^k, integer shifts and means): every
product and partial sum is an integer multiple of a power of two below 2^24 of it, exact in fp32 in any summation order, so stored
tensors and the float64 sums of the (NaN-prefilled) partial rows are compared with `==`; one dropped, doubled or wrongly masked pixel
fails.  Each reduction also has a randn case at the project's bars (statistics rows, dW, db: close(rtol=1e-4, floor=1); loss 1e-5
relative; dlogits close(rtol=1e-4); arg-max equal where the float64 margin exceeds 1e-4).  Planes: 35, 192, 576, 663 pixels and, per
grid cap (reducing kernels 4 workgroups per CU, streaming kernels 8), a multiple of 64 and an odd plane beyond one grid pass
(small_ops_cases.big_planes(rcv_num_cus)), so that the grid-stride loops make a second pass.

Kernel labels covered (rcv_op_kernel_label): bn_finalize, bn_bwd, bn_eval, pool_fwd, pool_bwd, pool_bwd_rows, bwd_stats, cls_fwd
(cls_fwd_kernel<8, FUSED, CE>, cls_fwd16_kernel; beyond a streaming grid pass too), cls_bwd (cls_bwd_kernel<8, 1..8, FUSED, CE>: 24 instantiations, both store paths;
<16, {1,5,8}, false, false>), ce_fwd, ce_bwd, dice_fwd, dice_bwd, sgd, adam_l1 (both instantiations), combine, materialize, add_slice,
nhwc_to_nchw, nchw_to_nhwc, wgrad_reduce, wgrad_reduce_batch; RCV_OP_CONFUSION (no label of its own).

BatchNorm bookkeeping: bound = (roundings + 1) * 2^-24 * sum|terms| against the restatement on the same fp32 rows.  The rows are
accumulated in double (error <= n_part 2^-53 sum|rows|, covered by the +1 as long as the sums are not cancelled: asserted), so the
fp32 roundings on each output's path are
  bn_finalize  mean (consts row 2, save_mean)   1   (float) of the double quotient
               istd                             1   (float) of 1 / sqrt(var + eps) in double; clamped variance: exactly fl(1/sqrt(eps))
               scale = gamma * istd             2
               shift = beta - mean * scale      5   mean 1, scale 2, product 1, difference 1
               running_mean                     5   1 - momentum 1, product 1, mean 1, product 1, sum 1
               running_var                      5   the same with (float) unbiased
  bn_bwd       A, B, C, dgamma, dbeta           1   each a (float) of a double expression; rows 3, 4 are copies (exact)
  bn_eval      istd = 1 / sqrtf(rv + eps)       3   sum, root, quotient
               scale                            4
               shift = beta - rm * scale        6
               row 3 = fma(bias, scale, shift)  7
SGD (one step from the device's own state): p 5 (g * grad_scale, fma, fma, lr * buf, difference), momentum buffer 3.
Adam + L1 (one step from the uploaded state; R.adam_l1_step carries the bound alongside every intermediate, each rounding weighted by
its OWN result and passed on through the later operations by their derivatives, so the count is per path, not one common factor):
  gr = fmaf(decay, sign p, g * grad_scale)        2   product, fma (0 and exact where pruned)
  m' = b1 m + (1 - b1) gr                         3 + gr's 2 = 5   two products, sum (1 - b exact for b >= 1/2)
  v' = b2 v + ((1 - b2) gr) gr                    4 + gr's 2 twice over (gr enters as a square) = 6 distinct roundings
  denom = sqrtf(v') / bc2_sqrt + eps              4   root (ev passed on as sqrt(v' + ev) - sqrt(v')), bc2_sqrt's own, quotient, sum
  step = lr_elem / bc1                            2   bc1's own, quotient
  p' = p - step * (m' / denom)                    3   quotient, product, difference
  => p' 20 roundings in all (m' 5, v' 6, 9 of its own), dominated by the last one, 2^-24 |p'|.
An fma contraction removes roundings only.  tests/test_small_ops.py: an fp32 emulation of this order stays inside (largest error / bound
p 0.990, m 0.972, v 0.992 over the cases) and each of seven wrong kernels leaves TWICE the bound on its recorded share of the elements.

Filter-gradient reduction: exact (==) on integer partials -- distinct weights per split; values of magnitude 2^23 that cancel across
splits, which the kernel's order of additions done in fp32 gets wrong on 4 - 43 % of the entries (measured per nsplit on the CPU) --
and for randn partials |got - ref| <= 2^-24 |ref| + nsplit 2^-53 sum|partials|: one fp32 rounding of a sum accumulated in double.

Largest error / bound measured on the MI355X (printed by every test; reported, not used as bars): Adam + L1 p 0.993, m 0.817, v 0.897
over the 13 cases x 3 record forms and the decay = 0 launch (the p bound is all but the final rounding of p, so a value just above a
power of two comes close to it); second metrics launch 2.1e-16 relative against the float64 sum (bar 1e-12); filter-gradient
reduction, randn partials, 0.998 (a correctly rounded fp32 of the double sum: the bound is that rounding).

A label outside [0, C) in the Dice loss: the reference's torch.eye(C)[label] raises (or wraps for -C..-1); the kernels treat the pixel
as belonging to no class (it adds to the cardinality through its probabilities only), which tests/test_small_ops.py pins."""
import numpy as np
import pytest
import torch

import small_ops_cases as K
import small_ops_restatement as R
from robocupvision_amd import _lib as L
from test_gpu_blocks import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _h():
    return L.handle(0)


def _cus():
    return int(L.load().rcv_num_cus(_h()))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _run(*ops):
    L.OpList(list(ops)).run(_h(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


def _label(op):
    return L.OpList([op]).labels(_h())[0]


def _ws(op):
    """NaN-filled workspace of an op (rows no workgroup writes show up in the sums); fills i[NPART]."""
    nbytes = L.op_workspace(_h(), op)
    ws = _nan(max(nbytes // 4, 1))
    op.p[L.RCV_P_PART] = ws.data_ptr()
    return ws


def _rowsum(ws, n_part, width):
    """Float64 host sum of ALL n_part partial rows of `width` floats."""
    return _np(ws[:n_part * width]).reshape(n_part, width).sum(0)


def _exact(got, ref, what):
    g, r = _np(got), np.asarray(ref, np.float64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.nonzero(~(g == r))
    assert bad[0].size == 0, "%s: %d / %d entries differ, first at %s: got %r, expected %r" % (
        what, bad[0].size, g.size, tuple(int(b[0]) for b in bad), g[tuple(b[0] for b in bad)], r[tuple(b[0] for b in bad)])


def _within(got, ref, roundings, terms, what):
    g, r, t = _np(got), np.asarray(ref, np.float64), np.asarray(terms, np.float64)
    err, bound = np.abs(g - r), (roundings + 1) * U * np.abs(t)
    print("%s: max error / bound %.3f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), "%s: error %.3e over the bound %.3e" % (what, float((err - bound).max()), float(bound[np.argmax(err - bound)]))


# ------------------------------------------------------------------------------------------ BatchNorm bookkeeping
def _stat_rows(rng, n_part, C, count):
    """Random fp32 partial rows of a plausible batch: sum v ~ count * mean, sum v^2 ~ count * (var + mean^2); channel 0's second
    sums are too small for its mean (negative variance in double)."""
    mean, var = rng.standard_normal(C) * 2, rng.uniform(0.5, 3.0, C)
    share, share2 = (rng.dirichlet(np.ones(n_part), C).T for _ in range(2))      # [n_part][C], every column sums to 1
    rows = np.empty((n_part, 2, C), np.float32)
    rows[:, 0] = share * count * mean
    rows[:, 1] = share2 * count * (var + mean ** 2)
    m0 = rows[:, 0, 0].astype(np.float64).sum() / count
    rows[:, 1, 0] = share2[:, 0] * count * 0.5 * m0 * m0
    return rows


@pytest.mark.parametrize("C", [8, 16, 64, 128])
@pytest.mark.parametrize("n_part", [1, 63, 257, 1000])
def test_bn_finalize_vs_float64(C, n_part):
    rng = np.random.default_rng(C * 7 + n_part)
    count = 4 * 37 * 53
    rows = _stat_rows(rng, n_part, C, count)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta, rm0 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rv0 = rng.uniform(0.5, 2.0, C).astype(np.float32)
    mom, eps = np.float32(0.1), np.float32(1e-5)
    S = np.abs(rows.astype(np.float64)).sum(0)                          # sum |rows|
    for training, with_running in ((True, True), (False, True), (True, False)):
        ref = R.bn_finalize(rows, count, gamma, beta, rm0, rv0, mom, eps, training and with_running)
        assert ref["var"][0] == 0.0 and np.all(ref["var"][1:] > 1e-3 * S[1, 1:] / count), "the sums must not be cancelled"
        rows_d, g_d, b_d = _dev(rows), _dev(gamma), _dev(beta)
        rm_d, rv_d = _dev(rm0), _dev(rv0)
        consts, sm, si = _nan(5, C), _nan(C), _nan(C)
        op = L.make_op(L.OP_BN_FINALIZE, L.F_TRAINING if training else 0, n=count, ho=1, wo=1, cout=C, npart=n_part, f0=mom, f1=eps,
                       p_part=rows_d.data_ptr(), p_x0=g_d.data_ptr(), p_x1=b_d.data_ptr(), p_x2=rm_d.data_ptr() if with_running else 0,
                       p_x3=rv_d.data_ptr() if with_running else 0, p_out=consts.data_ptr(), p_x4=sm.data_ptr(), p_x5=si.data_ptr())
        assert _label(op) == "bn_finalize"
        _run(op)
        mean, istd, sc = ref["mean"], ref["istd"], ref["consts"][0]
        what = "bn_finalize C=%d n_part=%d training=%d running=%d " % (C, n_part, training, with_running)
        _within(sm, mean, 1, S[0] / count, what + "mean")
        assert torch.equal(consts[2], sm) and torch.equal(consts[3:], torch.zeros(2, C, device=DEV))
        _within(si, istd, 1, istd, what + "istd")
        assert float(si[0]) == float(np.float32(1.0 / np.sqrt(np.float64(eps)))), "clamped variance: istd = fl(1 / sqrt(eps))"
        _within(consts[0], sc, 2, sc, what + "scale")
        _within(consts[1], ref["consts"][1], 5, np.abs(beta) + np.abs(S[0] / count * sc), what + "shift")
        if training and with_running:
            unb = ref["var"] * count / (count - 1.0)
            _within(rm_d, ref["running_mean"], 5, np.abs((1 - np.float64(mom)) * rm0) + np.abs(mom * S[0] / count), what + "running_mean")
            _within(rv_d, ref["running_var"], 5, np.abs((1 - np.float64(mom)) * rv0) + np.abs(mom * unb), what + "running_var")
        else:
            assert torch.equal(rm_d.cpu(), torch.from_numpy(rm0)) and torch.equal(rv_d.cpu(), torch.from_numpy(rv0))


def test_bn_finalize_count_one():
    """count == 1: the running variance takes the biased variance (no division by count - 1 = 0)."""
    C = 8
    rng = np.random.default_rng(1)
    x = rng.standard_normal(C).astype(np.float32)
    rows = np.stack([x, np.float32(1.5) * x * x])[None].astype(np.float32)           # variance 0.5 x^2 > 0
    gamma, beta, rm0, rv0 = (rng.uniform(0.5, 1.5, C).astype(np.float32) for _ in range(4))
    mom, eps = np.float32(0.25), np.float32(1e-5)
    ref = R.bn_finalize(rows, 1, gamma, beta, rm0, rv0, mom, eps, True)
    rows_d, g_d, b_d, rm_d, rv_d = (_dev(a) for a in (rows, gamma, beta, rm0, rv0))
    consts, sm, si = _nan(5, C), _nan(C), _nan(C)
    _run(L.make_op(L.OP_BN_FINALIZE, L.F_TRAINING, n=1, ho=1, wo=1, cout=C, npart=1, f0=mom, f1=eps, p_part=rows_d.data_ptr(),
                   p_x0=g_d.data_ptr(), p_x1=b_d.data_ptr(), p_x2=rm_d.data_ptr(), p_x3=rv_d.data_ptr(), p_out=consts.data_ptr(),
                   p_x4=sm.data_ptr(), p_x5=si.data_ptr()))
    assert torch.equal(sm.cpu(), torch.from_numpy(x))
    _within(si, ref["istd"], 1, ref["istd"], "count 1 istd")
    _within(rv_d, ref["running_var"], 5, np.abs(0.75 * rv0) + np.abs(0.25 * ref["var"]), "count 1 running_var")
    _within(rm_d, ref["running_mean"], 5, np.abs(0.75 * rm0) + np.abs(0.25 * x), "count 1 running_mean")


@pytest.mark.parametrize("C", [8, 16, 64, 128])
@pytest.mark.parametrize("n_part", [1, 63, 257, 1000])
def test_bn_backward_vs_float64(C, n_part):
    """The constants of both load kinds (RCV_LOAD_GRAD_ENC reads rows 0..2, RCV_LOAD_GRAD_DEC also the forward's scale / shift in
    rows 3, 4: copied bit for bit), dgamma, dbeta."""
    rng = np.random.default_rng(C * 11 + n_part)
    count = 3 * 13 * 17
    rows = (rng.standard_normal((n_part, 2, C)) * 3).astype(np.float32)
    gamma, mean = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    istd, fc = rng.uniform(0.3, 3.0, C).astype(np.float32), rng.standard_normal((5, C)).astype(np.float32)
    ref = R.bn_backward(rows, count, gamma, mean, istd, fc)
    S = np.abs(rows.astype(np.float64)).sum(0)
    rows_d, g_d, m_d, i_d, fc_d = (_dev(a) for a in (rows, gamma, mean, istd, fc))
    consts, dg, db = _nan(5, C), _nan(C), _nan(C)
    op = L.make_op(L.OP_BN_BWD, 0, n=count, ho=1, wo=1, cout=C, npart=n_part, p_part=rows_d.data_ptr(), p_x0=g_d.data_ptr(),
                   p_x4=m_d.data_ptr(), p_x5=i_d.data_ptr(), p_in_c=fc_d.data_ptr(), p_out=consts.data_ptr(), p_x1=dg.data_ptr(),
                   p_x2=db.data_ptr())
    assert _label(op) == "bn_bwd"
    _run(op)
    A = np.abs(gamma.astype(np.float64) * istd)
    Cabs = A * istd.astype(np.float64) * istd * S[1] / count
    what = "bn_bwd C=%d n_part=%d " % (C, n_part)
    _within(consts[0], ref["consts"][0], 1, A, what + "A")
    _within(consts[1], ref["consts"][1], 1, A * S[0] / count + Cabs * np.abs(mean), what + "B")
    _within(consts[2], ref["consts"][2], 1, Cabs, what + "C")
    assert torch.equal(consts[3:].cpu(), torch.from_numpy(fc[:2]))
    _within(dg, ref["dgamma"], 1, istd.astype(np.float64) * S[1], what + "dgamma")
    _within(db, ref["dbeta"], 1, S[0], what + "dbeta")
    # dgamma / dbeta are optional outputs
    consts2 = _nan(5, C)
    op.p[L.RCV_P_OUT], op.p[L.RCV_P_X1], op.p[L.RCV_P_X2] = consts2.data_ptr(), None, None
    _run(op)
    assert torch.equal(consts, consts2)


@pytest.mark.parametrize("C", [8, 16, 64, 128])
@pytest.mark.parametrize("with_bias", [False, True])
def test_bn_eval_vs_float64(C, with_bias):
    rng = np.random.default_rng(C + with_bias)
    gamma, beta, rm, bias = (rng.standard_normal(C).astype(np.float32) for _ in range(4))
    rv, eps = rng.uniform(0.01, 4.0, C).astype(np.float32), np.float32(1e-5)
    ref = R.bn_eval(gamma, beta, rm, rv, eps, bias if with_bias else None)
    g_d, b_d, rm_d, rv_d, bias_d = (_dev(a) for a in (gamma, beta, rm, rv, bias))
    consts = _nan(5, C)
    op = L.make_op(L.OP_BN_EVAL, 0, cout=C, f1=eps, p_x0=g_d.data_ptr(), p_x1=b_d.data_ptr(), p_x2=rm_d.data_ptr(), p_x3=rv_d.data_ptr(),
                   p_x4=bias_d.data_ptr() if with_bias else 0, p_out=consts.data_ptr())
    assert _label(op) == "bn_eval"
    _run(op)
    sc = np.abs(ref[0])
    tsh = np.abs(beta) + np.abs(rm * sc)
    _within(consts[0], ref[0], 4, sc, "bn_eval scale")
    _within(consts[1], ref[1], 6, tsh, "bn_eval shift")
    _within(consts[3], ref[3], 7, tsh + (np.abs(bias * sc) if with_bias else 0.0), "bn_eval folded bias")
    assert torch.equal(consts[2], torch.zeros(C, device=DEV)) and torch.equal(consts[4], torch.zeros(C, device=DEV))
    if not with_bias:
        assert torch.equal(consts[3], consts[1])


# ------------------------------------------------------------------------------------------ max-pool
def _pool_run(c, stats):
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    mode = L.LOAD_AFFINE if c["affine"] else L.LOAD_PLAIN
    r_d, dp_d, c_d = _dev(c["r"]), _dev(c["dp"]), _dev(np.concatenate([c["c"], np.zeros((5 - len(c["c"]), C), np.float32)]))
    res_d = _dev(c["res"]) if c["resid"] else None
    y = _nan(N, H // 2, W // 2, C)
    fop = L.make_op(L.OP_POOL_FWD, 0, n=N, h=H, w=W, cout=C, inmode=mode, p_in=r_d.data_ptr(), p_in_c=c_d.data_ptr(), p_out=y.data_ptr())
    assert _label(fop) == "pool_fwd"
    dy = _nan(N, H, W, C)
    bop = L.make_op(L.OP_POOL_BWD, L.F_RESID if c["resid"] else 0, n=N, h=H, w=W, cout=C, inmode=mode, stats=stats, p_in=dp_d.data_ptr(),
                    p_epi_aux=r_d.data_ptr(), p_in_c=c_d.data_ptr() if c["affine"] else 0, p_resid=res_d.data_ptr() if c["resid"] else 0,
                    p_out=dy.data_ptr())
    ws = _ws(bop)
    rows_kernel = K.pool_rows_kernel(W, C)
    assert _label(bop) == ("pool_bwd_rows" if rows_kernel else "pool_bwd")
    _run(fop, bop)
    return y, dy, ws, bop.i[L.RCV_I_NPART], rows_kernel


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("resid", [False, True])
def test_pool_forward_backward_statistics_exact(affine, resid):
    """RCV_OP_POOL_FWD and RCV_OP_POOL_BWD with RCV_STATS_BWD_ENC through both backward kernels (asserted by label), LOAD_PLAIN and
    LOAD_AFFINE with scales of both signs, ties in most windows, with and without the skip gradient; the last two planes exceed one
    grid pass (one per kernel)."""
    small, big, _ = K.pool_cases(_cus())
    cap = 256 * 4 * _cus()
    seen = set()
    for k, (N, H, W, C) in enumerate(small + big):
        beyond = k >= len(small)
        if beyond:
            assert N * (H // 2) * (W // 2) * (C // 4) > cap
        c = K.build_pool(N, H, W, C, affine, resid, second_item=cap if beyond else 0)
        K.check_pool(c)
        y, dy, ws, n_part, rows_kernel = _pool_run(c, L.STATS_BWD_ENC)
        seen.add((rows_kernel, beyond))
        what = "pool %s affine=%d resid=%d " % ((N, H, W, C), affine, resid)
        _exact(y, R.pool_forward(c["r"], c["c"], K.pool_mode(c)), what + "forward")
        ref = K.pool_dy(c)
        _exact(dy, ref, what + "dy")
        _exact(torch.from_numpy(_rowsum(ws, n_part, 2 * C).reshape(2, C)), R.stats(R.STATS_BWD_ENC, ref, c["r"], K.pool_ec(c)), what + "rows")
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_pool_backward_statistics_randn():
    rng = np.random.default_rng(4)
    for (N, H, W, C) in [(2, 6, 32, 8), (3, 10, 22, 16)]:
        c = dict(N=N, H=H, W=W, C=C, affine=True, resid=True, r=rng.standard_normal((N, H, W, C)).astype(np.float32),
                 dp=rng.standard_normal((N, H // 2, W // 2, C)).astype(np.float32), res=rng.standard_normal((N, H, W, C)).astype(np.float32))
        c["c"] = rng.standard_normal((5, C)).astype(np.float32)
        y, dy, ws, n_part, _ = _pool_run(c, L.STATS_BWD_ENC)
        ref = K.pool_dy(c)
        _exact(dy, ref.astype(np.float32), "pool randn dy")         # one fp32 addition per element: the rounded float64 sum
        rows = torch.from_numpy(_rowsum(ws, n_part, 2 * C).reshape(2, C))
        close(rows, torch.from_numpy(R.stats(R.STATS_BWD_ENC, ref.astype(np.float32), c["r"], K.pool_ec(c))), "pool randn rows", rtol=1e-4, floor=1.0)


# ------------------------------------------------------------------------------------------ BWD_STATS
def _bwd_stats_run(c, stats):
    N, H, W = c["plane"]
    g_d, e_d, ec_d = _dev(c["g"]), _dev(c["e"]), _dev(c["ec"])
    out = _nan(N, H, W, c["C"])
    op = L.make_op(L.OP_BWD_STATS, 0, n=N, h=H, w=W, cin=c["Csrc"], cout=c["C"], aux0=c["coff"], stats=stats, p_in=g_d.data_ptr(),
                   p_epi_aux=e_d.data_ptr(), p_epi_c=ec_d.data_ptr(), p_out=out.data_ptr())
    ws = _ws(op)
    assert _label(op) == "bwd_stats"
    _run(op)
    return out, ws, op.i[L.RCV_I_NPART]


@pytest.mark.parametrize("Csrc,coff,C", K.BWD_STATS_SLICES)
def test_bwd_stats_exact(Csrc, coff, C):
    cap = 256 * 4 * _cus()
    cases = [(pl, 0) for pl in K.PLANES]
    if (Csrc, coff, C) == (16, 8, 8):
        plane = K.big_planes(_cus())["reducing"][1]
        assert plane[0] * plane[1] * plane[2] * (C // 4) > cap
        cases.append((plane, cap))
    for plane, second in cases:
        c = K.build_bwd_stats(plane, Csrc, coff, C, second_item=second)
        K.check_bwd_stats(c)
        ref = K.bwd_stats_out(c)
        for stats in (L.STATS_NONE, L.STATS_BWD_ENC, L.STATS_BWD_DEC):
            out, ws, n_part = _bwd_stats_run(c, stats)
            what = "bwd_stats %s slice %s stats %d " % (plane, (Csrc, coff, C), stats)
            _exact(out, ref, what + "copy")
            if stats != L.STATS_NONE:
                _exact(torch.from_numpy(_rowsum(ws, n_part, 2 * C).reshape(2, C)), R.stats(stats, ref, c["e"], c["ec"]), what + "rows")
            else:
                assert n_part == 0


def test_bwd_stats_randn():
    rng = np.random.default_rng(8)
    plane, Csrc, coff, C = (3, 13, 17), 32, 16, 16
    c = dict(plane=plane, Csrc=Csrc, coff=coff, C=C, g=rng.standard_normal(plane + (Csrc,)).astype(np.float32),
             e=rng.standard_normal(plane + (C,)).astype(np.float32), ec=rng.standard_normal((3, C)).astype(np.float32))
    for stats in (L.STATS_BWD_ENC, L.STATS_BWD_DEC):
        out, ws, n_part = _bwd_stats_run(c, stats)
        _exact(out, K.bwd_stats_out(c), "bwd_stats randn copy")
        rows = torch.from_numpy(_rowsum(ws, n_part, 2 * C).reshape(2, C))
        ec = c["ec"].astype(np.float64)
        ref = R.stats(stats, K.bwd_stats_out(c), c["e"], c["ec"])
        near = np.abs(c["e"] * ec[0] + ec[1]) < 1e-5                 # a mask decided by an fp32 fma may differ next to zero
        assert stats == L.STATS_BWD_ENC or not near.any()
        close(rows, torch.from_numpy(ref), "bwd_stats randn rows", rtol=1e-4, floor=1.0)


# ------------------------------------------------------------------------------------------ 1x1 classifier
def _cls_ops(c, stats, dev):
    """The CLS_FWD and CLS_BWD records of a case (operands in `dev`)."""
    N, H, W = c["plane"]
    cin, nC, fused = c["cin"], c["nC"], c["form"] != "plain"
    dev.update(logits=_nan(N, nC, H, W), d_up=_nan(N, H, W, cin), dW=_nan(nC, cin), db=_nan(nC))
    kw = dict(n=N, h=H, w=W, cin=cin, cout=nC, p_w=dev["w"].data_ptr())
    if fused:
        kw.update(aux0=c["mode2"], p_x3=dev["r"].data_ptr(), p_x4=dev["rc"].data_ptr())
        fop = L.make_op(L.OP_CLS_FWD, L.F_FUSED_UP, p_in=dev["t"].data_ptr(), p_in_c=dev["tc"].data_ptr(), p_bias=dev["b"].data_ptr(),
                        p_out=dev["logits"].data_ptr(), **kw)
        bop = L.make_op(L.OP_CLS_BWD, L.F_FUSED_UP, stats=L.STATS_BWD_DEC, p_in2=dev["dl"].data_ptr(), p_out=dev["d_up"].data_ptr(),
                        p_epi_aux=dev["t"].data_ptr(), p_epi_c=dev["tc"].data_ptr(), p_x1=dev["dW"].data_ptr(), p_x2=dev["db"].data_ptr(), **kw)
    else:
        fop = L.make_op(L.OP_CLS_FWD, 0, p_in=dev["up"].data_ptr(), p_bias=dev["b"].data_ptr(), p_out=dev["logits"].data_ptr(), **kw)
        bop = L.make_op(L.OP_CLS_BWD, 0, stats=stats, p_in=dev["up"].data_ptr(), p_in2=dev["dl"].data_ptr(), p_out=dev["d_up"].data_ptr(),
                        p_epi_aux=dev["t"].data_ptr(), p_epi_c=dev["tc"].data_ptr(), p_x1=dev["dW"].data_ptr(), p_x2=dev["db"].data_ptr(), **kw)
    dev["ws"] = _ws(bop)
    assert _label(fop) == "cls_fwd" and _label(bop) == "cls_bwd"
    return fop, bop


def _cls_dev(c):
    return {k: _dev(c[k]) for k in ("t", "tc", "w", "b", "dl", "up", "r", "rc") if k in c}


@pytest.mark.parametrize("nC", range(1, 9))
def test_classifier_exact(nC):
    """RCV_OP_CLS_FWD / RCV_OP_CLS_BWD, 8 input channels (and the non-fused 16-channel form for 1, 5, 8 classes): plain, and the fused
    decoder input in each skip load mode; statistics off (plain form) and RCV_STATS_BWD_DEC; logits, d_up, dW, db and the statistics
    rows equal the float64 restatement.  Both store paths of cls_bwd_kernel (pixel count a multiple of 64 or not) and, on the planes
    beyond one grid pass, its prefetch of the next pixel."""
    cus = _cus()
    cap = 256 * 4 * cus
    cases = [k for k in K.cls_case_list(cus) if k[1] == nC]
    assert any(k[2][0] * k[2][1] * k[2][2] > cap for k in cases)
    for case in cases:
        c = K.build_cls(*case)
        K.check_cls(c)
        cin = c["cin"]
        up = K.cls_up(c)
        ref_logits = R.cls_forward(up, c["w"], c["b"])
        ref_dup, ref_dW, ref_db = R.cls_backward(up, c["dl"], c["w"])
        ref_rows = R.stats(R.STATS_BWD_DEC, ref_dup, c["t"], c["tc"])
        for stats in ((L.STATS_NONE, L.STATS_BWD_DEC) if c["form"] == "plain" else (L.STATS_BWD_DEC,)):
            dev = _cls_dev(c)
            fop, bop = _cls_ops(c, stats, dev)
            _run(fop, bop)
            what = "cls %d->%d %s %s stats %d " % (cin, nC, c["plane"], c["form"], stats)
            _exact(dev["logits"], ref_logits, what + "logits")
            _exact(dev["d_up"], ref_dup, what + "d_up")
            _exact(dev["dW"], ref_dW, what + "dW")
            _exact(dev["db"], ref_db, what + "db")
            if stats == L.STATS_BWD_DEC:
                n_part = bop.i[L.RCV_I_NPART]
                _exact(torch.from_numpy(_rowsum(dev["ws"], n_part, 2 * cin).reshape(2, cin)), ref_rows, what + "statistics rows")


def _ce_planes():
    return K.PLANES + K.big_planes(_cus())["reducing"]


@pytest.mark.parametrize("nC", range(1, 9))
def test_classifier_fused_loss_is_bit_identical_and_close(nC):
    """Random operands.  RCV_F_FUSED_UP|RCV_F_FUSED_CE forward = RCV_OP_CLS_FWD then RCV_OP_CE_FWD bit for bit (logits, loss row,
    arg-max); its backward = RCV_OP_CE_BWD then RCV_OP_CLS_BWD bit for bit (d_up, dW, db, statistics rows); all of it against float64
    at the project's bars.  Labels include -100 and values >= C."""
    for pi, (N, H, W) in enumerate(_ce_planes()):
        rng = np.random.default_rng(500 + 10 * nC + pi)
        mode2 = (L.LOAD_PLAIN, L.LOAD_AFFINE, L.LOAD_AFFINE_RELU)[(nC + pi) % 3]
        t, r = (rng.standard_normal((N, H, W, 8)).astype(np.float32) for _ in range(2))
        tc, rc = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
        tc[0], tc[1], tc[2] = rng.uniform(0.5, 1.5, 8) * rng.choice([-1, 1], 8), rng.standard_normal(8) * 0.3, rng.standard_normal(8) * 0.2
        rc[0], rc[1] = rng.uniform(0.5, 1.5, 8), rng.standard_normal(8) * 0.3
        w, b = (rng.standard_normal((nC, 8)) * 0.5).astype(np.float32), (rng.standard_normal(nC) * 0.1).astype(np.float32)
        tgt = rng.integers(0, nC, (N, H, W)).astype(np.int64)
        tgt.reshape(-1)[::37] = -100
        tgt.reshape(-1)[5::41] = nC + (pi % 3)
        cw = rng.uniform(0.5, 6.0, nC).astype(np.float32)
        t_d, r_d, tc_d, rc_d, w_d, b_d, cw_d = (_dev(a) for a in (t, r, tc, rc, w, b, cw))
        tgt_d, one_d = _dev(tgt, torch.int64), torch.ones(1, device=DEV)
        kw = dict(n=N, h=H, w=W, cin=8, cout=nC, aux0=mode2, p_w=w_d.data_ptr(), p_x3=r_d.data_ptr(), p_x4=rc_d.data_ptr())
        fkw = dict(p_in=t_d.data_ptr(), p_in_c=tc_d.data_ptr(), p_bias=b_d.data_ptr(), **kw)
        # forward
        lg1, lg2, loss1, loss2 = _nan(N, nC, H, W), _nan(N, nC, H, W), _nan(4), _nan(4)
        am1, am2 = (torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV) for _ in range(2))
        f1 = L.make_op(L.OP_CLS_FWD, L.F_FUSED_UP | L.F_FUSED_CE, p_out=lg1.data_ptr(), p_in2=tgt_d.data_ptr(), p_x0=cw_d.data_ptr(),
                       p_x1=loss1.data_ptr(), p_x2=am1.data_ptr(), **fkw)
        ws1 = _ws(f1)
        f2 = L.make_op(L.OP_CLS_FWD, L.F_FUSED_UP, p_out=lg2.data_ptr(), **fkw)
        ce = L.make_op(L.OP_CE_FWD, L.F_ARGMAX, n=N, h=H, w=W, cout=nC, p_in=lg2.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(),
                       p_out=loss2.data_ptr(), p_x0=am2.data_ptr())
        ws2 = _ws(ce)
        assert _label(ce) == "ce_fwd"
        _run(f1, f2, ce)
        what = "fused CE %d classes %s: " % (nC, (N, H, W))
        assert torch.equal(lg1, lg2) and torch.equal(loss1, loss2) and torch.equal(am1, am2), what + "forward forms differ"
        assert torch.equal(ws1[:f1.i[L.RCV_I_NPART] * 3], ws2[:ce.i[L.RCV_I_NPART] * 3])
        up = R.fused_up(t, tc, r, rc, mode2)
        logits = R.cls_forward(up, w, b)
        close(lg1, torch.from_numpy(logits), what + "logits", rtol=1e-4)
        ref = R.cross_entropy(logits, tgt, cw)
        got = _np(loss1)
        print(what + "loss %.8f vs %.8f" % (got[0], ref["loss"]))
        assert abs(got[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and abs(got[1] - ref["sum_w"]) <= 1e-5 * ref["sum_w"]
        srt = np.sort(logits, 1)
        clear = torch.from_numpy((srt[:, -1] - srt[:, -2]) > 1e-4) if nC > 1 else torch.ones(N, H, W, dtype=torch.bool)
        assert torch.equal(am1.cpu()[clear].long(), torch.from_numpy(ref["argmax"])[clear])
        assert torch.equal(am1.long(), lg1.argmax(1)) and int(got[2]) == int((lg1.argmax(1).cpu() == torch.from_numpy(tgt)).sum())
        # backward
        dl_d = _nan(N, nC, H, W)
        ceb = L.make_op(L.OP_CE_BWD, 0, n=N, h=H, w=W, cout=nC, p_in=lg1.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(),
                        p_x0=loss1.data_ptr(), p_x1=one_d.data_ptr(), p_out=dl_d.data_ptr())
        assert _label(ceb) == "ce_bwd"
        outs = []
        for with_ce in (False, True):
            d_up, dW, db = _nan(N, H, W, 8), _nan(nC, 8), _nan(nC)
            bop = L.make_op(L.OP_CLS_BWD, L.F_FUSED_UP | (L.F_FUSED_CE if with_ce else 0), stats=L.STATS_BWD_DEC, p_out=d_up.data_ptr(),
                            p_epi_aux=t_d.data_ptr(), p_epi_c=tc_d.data_ptr(), p_x1=dW.data_ptr(), p_x2=db.data_ptr(),
                            p_in2=(tgt_d if with_ce else dl_d).data_ptr(), **kw)
            if with_ce:
                bop.p[L.RCV_P_X0], bop.p[L.RCV_P_BIAS] = cw_d.data_ptr(), b_d.data_ptr()
                bop.p[L.RCV_P_X5], bop.p[L.RCV_P_IN2_AUX] = loss1.data_ptr(), one_d.data_ptr()
            ws = _ws(bop)
            _run(*([bop] if with_ce else [ceb, bop]))
            outs.append((d_up, dW, db, ws[:bop.i[L.RCV_I_NPART] * 16].clone()))
        for a, c_, name in zip(outs[0], outs[1], ("d_up", "dW", "db", "statistics rows")):
            assert torch.equal(a, c_), what + "%s of the fused-loss backward differs from CE_BWD + CLS_BWD" % name
        close(dl_d, torch.from_numpy(ref["dlogits"]), what + "dlogits", rtol=1e-4)
        ref_dup, ref_dW, ref_db = R.cls_backward(up, ref["dlogits"], w)
        close(outs[1][0], torch.from_numpy(ref_dup), what + "d_up", rtol=1e-4)
        close(outs[1][1], torch.from_numpy(ref_dW), what + "dW", rtol=1e-4, floor=1.0)
        close(outs[1][2], torch.from_numpy(ref_db), what + "db", rtol=1e-4, floor=1.0)
        rows = _np(outs[1][3]).reshape(-1, 2, 8).sum(0)
        close(torch.from_numpy(rows), torch.from_numpy(R.stats(R.STATS_BWD_DEC, ref_dup, t, tc)), what + "statistics rows", rtol=1e-4, floor=1.0)


@pytest.mark.parametrize("nC", range(1, 9))
def test_classifier_forward_beyond_a_streaming_pass(nC):
    """cls_fwd_kernel<8, false, false> and <8, true, false> (and cls_fwd16_kernel for 1, 5, 8 classes) are sized by the streaming cap,
    8 workgroups per CU: both planes beyond it, integer grid, logits exact."""
    cap = 256 * 8 * _cus()
    for pi, plane in enumerate(K.big_planes(_cus())["streaming"]):
        assert plane[0] * plane[1] * plane[2] > cap
        for cin, form in [(8, "plain"), (8, K.CLS_FORMS[1 + (nC + pi) % 3])] + ([(16, "plain")] if nC in (1, 5, 8) and pi == 1 else []):
            c = K.build_cls(cin, nC, plane, form, cap)
            up = K.cls_up(c)
            R.assert_exact(np.abs(R._f(c["w"])).sum(1) * np.abs(up).max() + np.abs(R._f(c["b"])), 1.0, "cls logits")
            dev = _cls_dev(c)
            fop, _ = _cls_ops(c, L.STATS_BWD_DEC, dev)
            _run(fop)
            _exact(dev["logits"], R.cls_forward(up, c["w"], c["b"]), "cls forward %d->%d %s %s" % (cin, nC, plane, form))


@pytest.mark.parametrize("nC", [1, 5, 8])
def test_cross_entropy_beyond_a_streaming_pass(nC):
    """ce_bwd_kernel is sized by the streaming cap (ce_fwd_kernel by the reducing one): both planes beyond it against float64."""
    cap = 256 * 8 * _cus()
    for pi, (N, H, W) in enumerate(K.big_planes(_cus())["streaming"]):
        assert N * H * W > cap
        rng = np.random.default_rng(700 + 10 * nC + pi)
        lg = (rng.standard_normal((N, nC, H, W)) * 2).astype(np.float32)
        tgt = rng.integers(0, nC, (N, H, W)).astype(np.int64)
        tgt.reshape(-1)[::37] = -100
        tgt.reshape(-1)[-1] = nC - 1
        tgt.reshape(-1)[cap] = 0
        cw = rng.uniform(0.5, 6.0, nC).astype(np.float32)
        lg_d, tgt_d, cw_d, go_d = _dev(lg), _dev(tgt, torch.int64), _dev(cw), _dev(np.array([0.5], np.float32))
        loss, dl = _nan(4), _nan(N, nC, H, W)
        fop = L.make_op(L.OP_CE_FWD, 0, n=N, h=H, w=W, cout=nC, p_in=lg_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(), p_out=loss.data_ptr())
        ws = _ws(fop)
        bop = L.make_op(L.OP_CE_BWD, 0, n=N, h=H, w=W, cout=nC, p_in=lg_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_w=cw_d.data_ptr(),
                        p_x0=loss.data_ptr(), p_x1=go_d.data_ptr(), p_out=dl.data_ptr())
        _run(fop, bop)
        ref = R.cross_entropy(lg, tgt, cw, grad_out=0.5)
        got = _np(loss)
        assert abs(got[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]) if nC > 1 else abs(got[0]) <= 1e-12
        close(dl, torch.from_numpy(ref["dlogits"]), "ce_bwd %d classes %s" % (nC, (N, H, W)), rtol=1e-4)
        if nC > 1:      # the last pixel and the first one of the second pass were written (a one-class gradient is identically zero)
            flat = dl.permute(0, 2, 3, 1).reshape(-1, nC)
            assert float(flat[-1].abs().max()) > 0 and float(flat[cap].abs().max()) > 0
        del ws


# ------------------------------------------------------------------------------------------ Dice loss
@pytest.mark.parametrize("nC", range(2, 9))
@pytest.mark.parametrize("weighted", [False, True])
def test_dice_vs_float64(nC, weighted):
    # dice_fwd_kernel reduces (4 workgroups per CU), dice_bwd_kernel streams (8): both planes beyond each cap (the streaming ones once
    # per class count: the weights do not reach the backward kernel)
    big = K.big_planes(_cus())
    planes = K.PLANES + big["reducing"] + (big["streaming"] if weighted else [])
    assert all(n * h * w > 256 * 8 * _cus() for n, h, w in big["streaming"]) and all(n * h * w > 256 * 4 * _cus() for n, h, w in big["reducing"])
    for pi, (N, H, W) in enumerate(planes):
        rng = np.random.default_rng(900 + 10 * nC + pi)
        lg = (rng.standard_normal((N, nC, H, W)) * 2).astype(np.float32)
        tgt = rng.integers(0, nC, (N, H, W)).astype(np.int64)
        tgt.reshape(-1)[::29] = -100
        tgt.reshape(-1)[3::31] = nC + 1
        cw = rng.uniform(0.5, 4.0, nC)
        cw = (cw / cw.sum() * nC).astype(np.float32)
        eps, go = np.float32(1e-7), np.float32(0.75)
        lg_d, tgt_d, cw_d, go_d = _dev(lg), _dev(tgt, torch.int64), _dev(cw), _dev(np.array([go]))
        out, am, dl = _nan(20), torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV), _nan(N, nC, H, W)
        fop = L.make_op(L.OP_DICE_FWD, L.F_ARGMAX, n=N, h=H, w=W, cout=nC, f1=eps, p_in=lg_d.data_ptr(), p_in2=tgt_d.data_ptr(),
                        p_w=cw_d.data_ptr() if weighted else 0, p_out=out.data_ptr(), p_x0=am.data_ptr())
        ws = _ws(fop)
        bop = L.make_op(L.OP_DICE_BWD, 0, n=N, h=H, w=W, cout=nC, p_in=lg_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_x0=out.data_ptr(),
                        p_x1=go_d.data_ptr(), p_out=dl.data_ptr())
        assert _label(fop) == "dice_fwd" and _label(bop) == "dice_bwd"
        _run(fop, bop)
        assert not bool(torch.isnan(ws[:fop.i[L.RCV_I_NPART] * 25]).any()), "a partial row was not written"
        ref = R.dice(lg, tgt, cw if weighted else None, eps, grad_out=go)
        got = _np(out)
        what = "dice %d classes %s weighted=%d: " % (nC, (N, H, W), weighted)
        print(what + "loss %.8f vs %.8f" % (got[0], ref["loss"]))
        assert abs(got[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
        close(out[4:4 + nC], torch.from_numpy(ref["A"]), what + "A_c", rtol=1e-4)
        close(out[12:12 + nC], torch.from_numpy(ref["B"]), what + "B_c", rtol=1e-4)
        assert float(out[4 + nC:12].abs().sum()) == 0.0 and float(out[12 + nC:20].abs().sum()) == 0.0
        srt = np.sort(lg.astype(np.float64), 1)
        clear = torch.from_numpy((srt[:, -1] - srt[:, -2]) > 1e-4)
        assert torch.equal(am.cpu()[clear].long(), torch.from_numpy(ref["argmax"])[clear])
        assert torch.equal(am.long(), lg_d.argmax(1)) and int(got[2]) == int((lg_d.argmax(1).cpu() == torch.from_numpy(tgt)).sum())
        close(dl, torch.from_numpy(ref["dlogits"]), what + "dlogits", rtol=1e-4)


# ------------------------------------------------------------------------------------------ optimizers
def _sgd_op(p, g, buf, lre, n, lr, mom, wd, step, gs):
    return L.make_op(L.OP_SGD, 0, count=n, aux0=step, f0=lr, f1=mom, f2=wd, f5=gs, p_in=p.data_ptr(), p_in2=g.data_ptr(), p_x0=buf.data_ptr(),
                     p_x2=lre.data_ptr() if lre is not None else 0)


@pytest.mark.parametrize("n", [1, 255, 100003])
def test_sgd_vs_float64(n):
    """Three steps: each against the restatement applied to the device's own previous state (the derived one-step bound), the
    trajectory against torch.optim.SGD in float64 (one-step bounds added up: a buffer error e moves later parameters by lr e, decaying
    with the momentum, so the factor 1 / (1 - momentum) covers it); lr_elem == 0 leaves the element and its buffer untouched."""
    rng = np.random.default_rng(n)
    lr, mom, wd, gs = np.float32(0.2), np.float32(0.5), np.float32(1e-3), np.float32(0.25)
    p0 = rng.standard_normal(n).astype(np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.SGD([ref], lr=float(lr), momentum=float(mom), weight_decay=float(wd))
    p, buf = _dev(p0), torch.full((n,), 123.0, device=DEV)         # the buffer's content is ignored at step 1
    lre = np.full(n, lr, np.float32)
    lre[::3] = 0.0
    q, qbuf, lre_d = _dev(p0), torch.full((n,), 7.0, device=DEV), _dev(lre)
    assert _label(_sgd_op(p, p, buf, None, n, lr, mom, wd, 1, gs)) == "sgd"
    acc = np.zeros(n)
    for step in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        g_d = _dev(g)
        p_prev, b_prev = _np(p), _np(buf)
        _run(_sgd_op(p, g_d, buf, None, n, lr, mom, wd, step, gs), _sgd_op(q, g_d, qbuf, lre_d, n, lr, mom, wd, step, gs))
        rp, rb = R.sgd_step(p_prev, g, b_prev, step, lr, mom, wd, gs)
        tb = (np.abs(mom * b_prev) if step > 1 else 0.0) + np.abs(np.float64(wd) * p_prev) + np.abs(g.astype(np.float64) * gs)
        _within(buf, rb, 3, tb, "sgd n=%d step %d buffer" % (n, step))
        _within(p, rp, 5, np.abs(p_prev) + lr * tb, "sgd n=%d step %d parameter" % (n, step))
        ref.grad = torch.from_numpy(g).double() * float(gs)
        opt.step()
        acc += 6 * U * (np.abs(p_prev) + lr * tb) / (1.0 - float(mom))
        assert np.all(np.abs(_np(p) - ref.detach().numpy()) <= acc), "sgd trajectory vs torch.optim.SGD"
    live = lre != 0
    assert torch.equal(q.cpu()[~live], torch.from_numpy(p0)[~live]) and bool((qbuf.cpu()[~live] == 7.0).all())
    assert torch.equal(q.cpu()[live], p.cpu()[live])


def test_sgd_integer_grid_exact():
    """Integer parameters and gradients, lr = momentum = 1/2, weight decay 1/4, grad_scale 2: every value of three steps is a short
    dyadic fraction, so torch.optim.SGD in float64 gives the kernel's bits."""
    rng = np.random.default_rng(2)
    n = 100003
    p0 = R.grid(rng, (n,), 2)
    ref = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.SGD([ref], lr=0.5, momentum=0.5, weight_decay=0.25)
    p, buf = _dev(p0), _nan(n)
    for step in (1, 2, 3):
        g = R.grid(rng, (n,), 2)
        ref.grad = torch.from_numpy(g).double() * 2.0
        opt.step()
        assert torch.equal(ref.detach().float().double(), ref.detach()), "not exact in fp32"
        _run(_sgd_op(p, _dev(g), buf, None, n, 0.5, 0.5, 0.25, step, 2.0))
        _exact(p, ref.detach().numpy(), "sgd integer grid step %d" % step)


def test_adam_l1_unaligned_prune_mask_takes_the_scalar_path():
    """A prune mask that is not 4-byte aligned (a view one byte into its allocation) cannot be read as uchar4: the element-by-element
    path must give the same bits as the aligned run."""
    n = 100003
    g = torch.Generator().manual_seed(5)
    p0, gr, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g) * 0.01
    mask = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    outs = []
    for shift in (0, 1, 4):
        p, gd, m, v = (x.clone().to(DEV) for x in (p0, gr, m0, v0))
        mbuf = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        mk = mbuf[shift:shift + n]
        mk.copy_(mask)
        assert (mk.data_ptr() % 4 == 0) == (shift != 1) and p.data_ptr() % 16 == 0
        op = L.make_op(L.OP_ADAM_L1, 0, count=n, aux0=3, f0=2e-3, f1=0.9, f2=0.999, f3=1e-8, f4=1e-3, f5=1.0, p_in=p.data_ptr(),
                       p_in2=gd.data_ptr(), p_x0=m.data_ptr(), p_x1=v.data_ptr(), p_x5=mk.data_ptr())
        assert _label(op) == "adam_l1"
        _run(op)
        outs.append((p, m, v))
    for k in (1, 2):
        for a, b in zip(outs[0], outs[k]):
            assert torch.equal(a, b)
    # a pruned element has a zero gradient this step: its moments only decay
    pruned = mask.bool()
    assert torch.equal(outs[0][1].cpu()[pruned], (torch.tensor(0.9, dtype=torch.float32) * m0)[pruned])
    assert not torch.equal(outs[0][0].cpu()[~pruned], p0[~pruned])


def _adam_op(c, t, p, g, m, v, lre=None, prune=None, decay=None, step_dev=None, metrics=None, loss_stats=None):
    """One RCV_OP_ADAM_L1 record on device tensors; step_dev: an int32 tensor holding t (the record's own step is then 0)."""
    ptr = lambda x: x.data_ptr() if x is not None else 0
    return L.make_op(L.OP_ADAM_L1, 0, count=c["n"], aux0=0 if step_dev is not None else t, f0=c["lr"], f1=c["b1"], f2=c["b2"], f3=c["eps"],
                     f4=c["decay"] if decay is None else decay, f5=c["gs"], p_in=ptr(p), p_in2=ptr(g), p_x0=ptr(m), p_x1=ptr(v), p_x2=ptr(lre),
                     p_x5=ptr(prune), p_in_aux=ptr(step_dev), p_x3=ptr(metrics), p_x4=ptr(loss_stats))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inside(got, ref, bound, where, what):
    g = _np(got)
    err = np.abs(g - ref)[where]
    b = bound[where]
    ratio = float(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0).max()) if err.size else 0.0
    print("%s: max error / bound %.3f" % (what, ratio))
    assert np.all(err <= b), "%s: %d of %d elements over the bound, largest error / bound %.3f" % (what, int((~(err <= b)).sum()), err.size, ratio)
    return ratio


@pytest.mark.parametrize("k", range(len(K.adam_cases(256))))
def test_adam_l1_vs_float64(k):
    """One step from the uploaded state, plain / with lr_elem / with lr_elem and the prune mask, against R.adam_l1_step inside its
    running bound (p, m, v each); lr_elem == 0: p keeps its bits, the moments their sentinels; a pruned element's moments are exactly
    fl(b1 m), fl(b2 v); with decay = 0 an element with g = m = v = 0 keeps its bits (-0 stays -0)."""
    n, t, gs = K.adam_cases(_cus())[k]
    c = K.build_adam(n, t, gs)
    g_d, lre_d, pr_d = _dev(c["g"]), _dev(c["lr_elem"]), _dev(c["prune"], torch.uint8)
    p0_bits = _bits(torch.from_numpy(c["p"]))
    for form in K.ADAM_FORMS:
        lre, pr = K.adam_form(c, form)
        dead = (lre == 0) if lre is not None else np.zeros(n, bool)
        live = ~dead
        p = _dev(c["p"])
        m, v = _dev(np.where(dead, np.float32(123.0), c["m"])), _dev(np.where(dead, np.float32(7.0), c["v"]))
        op = _adam_op(c, t, p, g_d, m, v, lre_d if lre is not None else None, pr_d if pr is not None else None)
        assert _label(op) == "adam_l1"
        _run(op)
        (rp, rm, rv), (ep, em, ev) = K.adam_reference(c, form)
        what = "adam n=%d t=%d gs=%.3f %s " % (n, t, gs, form)
        _inside(p, rp, ep, live, what + "p")
        _inside(m, rm, em, live, what + "m")
        _inside(v, rv, ev, live, what + "v")
        if dead.any():
            d = torch.from_numpy(dead)
            assert torch.equal(_bits(p)[d], p0_bits[d]), what + "lr_elem == 0 must leave p's bits"
            assert bool((m.cpu()[d] == 123.0).all()) and bool((v.cpu()[d] == 7.0).all()), what + "lr_elem == 0 must leave the moments"
        if pr is not None:
            pl = torch.from_numpy((pr != 0) & live)
            assert torch.equal(_bits(m)[pl], _bits(torch.from_numpy(c["b1"] * c["m"]))[pl]), what + "pruned: m' = fl(b1 m)"
            assert torch.equal(_bits(v)[pl], _bits(torch.from_numpy(c["b2"] * c["v"]))[pl]), what + "pruned: v' = fl(b2 v)"
    # no decay: nothing moves an element whose gradient and moments are zero
    p, m, v = _dev(c["p"]), _dev(c["m"]), _dev(c["v"])
    _run(_adam_op(c, t, p, g_d, m, v, decay=0.0))
    (rp, rm, rv), (ep, em, ev) = K.adam_reference(c, "plain", decay=0.0)
    every = np.ones(n, bool)
    _inside(p, rp, ep, every, "adam n=%d t=%d decay 0 p" % (n, t))
    _inside(m, rm, em, every, "adam n=%d t=%d decay 0 m" % (n, t))
    _inside(v, rv, ev, every, "adam n=%d t=%d decay 0 v" % (n, t))
    z = torch.from_numpy((c["g"] == 0) & (c["m"] == 0) & (c["v"] == 0))
    assert torch.equal(_bits(p)[z], p0_bits[z]) and not bool(_bits(m)[z].any()) and not bool(_bits(v)[z].any())
    if n >= 1027:
        assert bool((p0_bits[z] == -2 ** 31).any()) and bool(z.any()), "the case must hold a -0 with zero gradient and moments"


@pytest.mark.parametrize("t", [1, 1000])
def test_adam_l1_device_step_counter(t):
    """The step of a replayed graph comes from an int32 on the device (p[RCV_P_IN_AUX]): the same bits as the record that carries t;
    two such records of one op list with the counter advanced on the device between them = the records of t and t + 1."""
    c = K.build_adam(100003, t, 0.125)
    g_d, lre_d, pr_d = _dev(c["g"]), _dev(c["lr_elem"]), _dev(c["prune"], torch.uint8)
    host = [_dev(c[k]) for k in "pmv"]
    devc = [_dev(c[k]) for k in "pmv"]
    counter = torch.tensor([t], dtype=torch.int32, device=DEV)
    _run(_adam_op(c, t, *host[:1], g_d, *host[1:], lre_d, pr_d), _adam_op(c, t, *devc[:1], g_d, *devc[1:], lre_d, pr_d, step_dev=counter))
    for a, b, name in zip(host, devc, "pmv"):
        assert torch.equal(_bits(a), _bits(b)), "step %d from the device counter: %s differs" % (t, name)
    assert not torch.equal(_bits(host[0]), _bits(torch.from_numpy(c["p"])))
    # second step
    _run(_adam_op(c, t + 1, *host[:1], g_d, *host[1:], lre_d, pr_d))
    two = [_dev(c[k]) for k in "pmv"]
    ops = L.OpList([_adam_op(c, t, *two[:1], g_d, *two[1:], lre_d, pr_d, step_dev=counter)] * 2)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ops.run_slice(_h(), stream, 0, 1)
    counter.add_(1)
    ops.run_slice(_h(), stream, 1, 2)
    torch.cuda.synchronize()
    assert int(counter.item()) == t + 1
    for a, b, name in zip(host, two, "pmv"):
        assert torch.equal(_bits(a), _bits(b)), "steps %d, %d from the device counter: %s differs" % (t, t + 1, name)
    if t == 1:      # the two steps do differ in their bias corrections: a counter read as t twice is seen
        stale = [_dev(c[k]) for k in "pmv"]
        _run(_adam_op(c, t, *stale[:1], g_d, *stale[1:], lre_d, pr_d), _adam_op(c, t, *stale[:1], g_d, *stale[1:], lre_d, pr_d))
        assert not torch.equal(_bits(stale[0]), _bits(host[0]))


@pytest.mark.parametrize("size", ["5", "100003", "beyond a grid pass"])
def test_adam_l1_metrics_exact(size):
    """The metrics launch: p on the grid k / 8 (sum|p| exact in any order), a third of the elements unstepped, a quarter pruned;
    metrics == [0.5 + decay sum|p|, decay sum|p|, 7, 1] over ALL n elements before the update, the ticket is left 0, p / m / v have
    the bits of the launch without metrics; a second launch adds its row (p is off the grid by then: 1e-12 relative)."""
    n = K.adam_big_n(_cus()) if size == "beyond a grid pass" else int(size)
    c = K.adam_metrics_inputs(n)
    c.update({k: np.float32(x) for k, x in K.ADAM_HYPER.items()})
    c["gs"], c["decay"] = np.float32(1.0), np.float32(2.0 ** -10)
    g_d, lre_d, pr_d = _dev(c["g"]), _dev(c["lr_elem"]), _dev(c["prune"], torch.uint8)
    loss = _dev(np.array([0.5, np.nan, 7.0, np.nan], np.float32))
    plain, met = [_dev(c[k]) for k in "pmv"], [_dev(c[k]) for k in "pmv"]
    metrics = torch.zeros(4, dtype=torch.float64, device=DEV)
    op = _adam_op(c, 3, *met[:1], g_d, *met[1:], lre_d, pr_d, metrics=metrics, loss_stats=loss)
    nbytes = L.op_workspace(_h(), op)
    rows = op.i[L.RCV_I_NPART]
    assert nbytes == (rows + 1) * 8 and rows == min((n // 4 + 255) // 256 or 1, 2 * _cus())
    ws = torch.full((rows + 1,), float("nan"), dtype=torch.float64, device=DEV)
    ws[rows] = 0.0                                               # the ticket word (and its padding)
    op.p[L.RCV_P_PART] = ws.data_ptr()
    _run(_adam_op(c, 3, *plain[:1], g_d, *plain[1:], lre_d, pr_d), op)
    reg = np.float64(c["decay"]) * np.abs(c["p"].astype(np.float64)).sum()
    want = np.array([0.5 + reg, reg, 7.0, 1.0])
    got = metrics.cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert not bool(torch.isnan(ws[:rows]).any()) and float(ws[:rows].sum()) * float(c["decay"]) == reg
    assert int(ws[rows:].view(torch.int32)[0].item()) == 0, "the ticket must read 0 after the launch"
    for a, b, name in zip(plain, met, "pmv"):
        assert torch.equal(_bits(a), _bits(b)), "metrics launch: %s differs from the plain launch" % name
    p1 = _np(met[0])
    assert (np.abs(p1[c["lr_elem"] == 0]) == np.abs(c["p"][c["lr_elem"] == 0])).all() and (p1 != c["p"]).any()
    _run(op)
    reg2 = np.float64(c["decay"]) * np.abs(p1).sum()
    want2 = want + np.array([0.5 + reg2, reg2, 7.0, 1.0])
    got2 = metrics.cpu().numpy()
    print("adam metrics n=%d second launch: relative difference %.2e" % (n, float(np.abs(got2 - want2).max() / np.abs(want2).max())))
    assert np.all(np.abs(got2 - want2) <= 1e-12 * np.abs(want2)), (got2.tolist(), want2.tolist())
    assert int(ws[rows:].view(torch.int32)[0].item()) == 0


# ------------------------------------------------------------------------------------------ filter-gradient reductions
GUARD = 777.0


class _ReduceOut:
    """NaN-prefilled dW [CB][CA][3][3] and db [n_db] with 16 guard floats before, between and after them."""

    def __init__(self, CB, CA, n_db=None):
        self.nw, self.nb = CB * CA * 9, CB if n_db is None else n_db
        self.buf = torch.full((48 + self.nw + self.nb,), GUARD, device=DEV)
        self.dw = self.buf[16:16 + self.nw]
        self.db = self.buf[32 + self.nw:32 + self.nw + self.nb]
        self.dw.fill_(float("nan"))
        self.db.fill_(float("nan"))
        self.shape = (CB, CA, 3, 3)

    def guards_intact(self, db_written=True):
        b = self.buf.cpu()
        ok = bool((b[:16] == GUARD).all()) and bool((b[16 + self.nw:32 + self.nw] == GUARD).all()) and bool((b[-16:] == GUARD).all())
        return ok and (db_written or bool(torch.isnan(b[32 + self.nw:32 + self.nw + self.nb]).all()))


def _reduce_single(c, part_d, with_bias):
    out = _ReduceOut(c["CB"], c["CA"])
    op = L.make_op(L.OP_WGRAD_REDUCE, 0, cin=c["CA"], cout=c["CB"], nsplit=c["nsplit"], p_part=part_d.data_ptr(), p_out=out.dw.data_ptr(),
                   p_bias=out.db.data_ptr() if with_bias else 0)
    assert _label(op) == "wgrad_reduce"
    _run(op)
    return out


@pytest.mark.parametrize("CB,CA", K.REDUCE_SHAPES + (K.REDUCE_WIDE[0],))
def test_wgrad_reduce_every_split_regime(CB, CA):
    """RCV_OP_WGRAD_REDUCE alone on hand-made partials [nsplit][9][CBP][CAP] (+ [nsplit][CBP]) with NaN in the pad rows / columns and
    in a whole extra split behind the last: nsplit across every edge of the loop structure (<= 16, the 16-stride tail, the
    four-loads-in-flight main loop from 49, its second round from 65 ... 113), with and without the bias row.  Exact on distinct
    integer weights per split and on the cancelling integers only a double accumulation gets right; randn within one fp32 rounding
    of the double sum."""
    wide = (CB, CA) == K.REDUCE_WIDE[0]
    worst = 0.0
    for ns in (K.REDUCE_WIDE[1] if wide else K.REDUCE_NSPLIT):
        for kind in ("weights", "cancel") + (("randn",) if ns in (49, 200) else ()):
            c = K.build_reduce(ns, CB, CA, kind)
            ref_dw, ref_db = K.reduce_reference(c)
            for with_bias in ((True,) if wide else (True, False)):
                part_d = _dev(K.reduce_buffer(c, with_bias))
                out = _reduce_single(c, part_d, with_bias)
                what = "wgrad_reduce (%d, %d) nsplit %d %s bias=%d " % (CB, CA, ns, kind, with_bias)
                assert out.guards_intact(db_written=with_bias), what + "wrote outside its outputs"
                got = [(out.dw.reshape(out.shape), ref_dw, c["part"][:, :, :CB, :CA].transpose(0, 2, 3, 1).reshape((ns,) + out.shape), "dW")]
                if with_bias:
                    got.append((out.db, ref_db, c["bias"][:, :CB], "db"))
                for g, r, terms, name in got:
                    if kind != "randn":
                        _exact(g, r, what + name)
                        continue
                    assert not bool(torch.isnan(g).any()), what + name + ": an entry was not written (or took in a pad)"
                    bound = U * np.abs(r) + ns * 2.0 ** -53 * np.abs(terms.astype(np.float64)).sum(0)
                    err = np.abs(_np(g) - r)
                    worst = max(worst, float((err / bound).max()))
                    assert np.all(err <= bound), what + name + ": error / bound %.3f" % float((err / bound).max())
    print("wgrad_reduce (%d, %d) randn: max error / bound %.3f" % (CB, CA, worst))


def test_wgrad_reduce_batch_equals_the_single_records():
    """One RCV_OP_WGRAD_REDUCE_BATCH whose job table is built here from the header's formula (rcv_reduce_job): reductions with and
    without a bias row and two zero-fill jobs (one of two blocks); every output is bit for bit the single record's and equals the
    float64 sums; a zero-filled vector is 0 over [0, CB) and nothing beyond; every guard is intact."""
    import ctypes as C
    specs = [("red", 16, 8, 49, True, "cancel"), ("zero", 300, 0, 0, True, None), ("red", 8, 3, 1, False, "weights"), ("red", 64, 32, 65, True, "cancel"),
             ("zero", 1, 0, 0, True, None), ("red", 5, 16, 17, True, "weights")]
    table = (L.RcvReduceJob * len(specs))()
    keep, first = [], 0
    for j, (what, CB, CA, ns, with_bias, kind) in enumerate(specs):
        table[j].nsplit, table[j].CB, table[j].CA, table[j].first_block = ns, CB, CA, first
        if what == "zero":
            out = _ReduceOut(1, 1, n_db=CB)
            table[j].db = out.db.data_ptr()
            first += (CB + 255) // 256
            keep.append((None, None, out))
            continue
        c = K.build_reduce(ns, CB, CA, kind, seed=j)
        part_d = _dev(K.reduce_buffer(c, with_bias))
        out = _ReduceOut(CB, CA)
        table[j].part, table[j].dw, table[j].db = part_d.data_ptr(), out.dw.data_ptr(), out.db.data_ptr() if with_bias else None
        CBP, CAP = (CB + 15) // 16 * 16, 4 if CA <= 4 else (CA + 15) // 16 * 16
        first += (9 * CBP * CAP + (CBP if with_bias else 0) + 63) // 64
        keep.append((c, part_d, out))
    assert first == 37 + 2 + 9 + 289 + 1 + 37
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    op = L.make_op(L.OP_WGRAD_REDUCE_BATCH, 0, count=len(specs), npart=first, p_in=table_d.data_ptr())
    assert _label(op) == "wgrad_reduce_batch"
    _run(op)
    for (what, CB, CA, ns, with_bias, kind), (c, part_d, out) in zip(specs, keep):
        name = "batch job %s (%d, %d) nsplit %d: " % (what, CB, CA, ns)
        if what == "zero":
            assert out.guards_intact() and bool(torch.isnan(out.dw).all()), name + "wrote outside [0, CB)"
            assert torch.equal(out.db, torch.zeros(CB, device=DEV)), name + "not zero-filled"
            continue
        assert out.guards_intact(db_written=with_bias), name + "wrote outside its outputs"
        single = _reduce_single(c, part_d, with_bias)
        assert torch.equal(_bits(out.dw), _bits(single.dw)), name + "dW differs from the single record"
        ref_dw, ref_db = K.reduce_reference(c)
        _exact(out.dw.reshape(out.shape), ref_dw, name + "dW")
        if with_bias:
            assert torch.equal(_bits(out.db), _bits(single.db)), name + "db differs from the single record"
            _exact(out.db, ref_db, name + "db")


# ------------------------------------------------------------------------------------------ confusion counts
def _confusion_op(pred_d, tgt_d, counts, C):
    N, H, W = pred_d.shape
    return L.make_op(L.OP_CONFUSION, 0, n=N, h=H, w=W, cout=C, p_in=pred_d.data_ptr(), p_in2=tgt_d.data_ptr(), p_out=counts.data_ptr())


@pytest.mark.parametrize("C", K.CONF_CLASSES)
def test_confusion_exact(C):
    """RCV_OP_CONFUSION against numpy's bincount: uint8 predictions (some >= C), int64 labels with -100, -1, C, 255, 2^32 + 1 and
    -2^32 + 2 among them (no class: the range test is made on the int64), one workgroup per image, odd planes, one pixel, and a plane
    past the workgroup cap whose last pixel carries a pair of its own; the op accumulates."""
    for N, H, W in K.confusion_planes():
        pred, tgt = K.build_confusion(N, H, W, C)
        ref = R.confusion(pred, tgt, C)
        pred_d, tgt_d = _dev(pred, torch.uint8), _dev(tgt, torch.int64)
        counts = torch.zeros(N, C, C, dtype=torch.int32, device=DEV)
        op = _confusion_op(pred_d, tgt_d, counts, C)
        _run(op)
        what = "confusion %d classes %s: " % (C, (N, H, W))
        got = counts.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref), what + "counts differ at %s: got %s, expected %s" % (
            np.argwhere(got != ref)[:4].tolist(), got[got != ref][:4].tolist(), ref[got != ref][:4].tolist())
        ok = (pred < C) & (tgt >= 0) & (tgt < C)
        assert np.array_equal(got.sum((1, 2)), ok.reshape(N, -1).sum(1)), what + "the counts of an image must add up to its pixels in range"
        _run(op)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), 2 * ref), what + "a second run must add to the first"


def test_confusion_more_images_than_a_grid_dimension():
    """The image index is a grid dimension (at most 65535): more images fold onto it -- PatchMetrics counts one 1x1 image per patch."""
    N, C = 65536 + 3, 4
    pred, tgt = K.build_confusion(N, 1, 1, C)
    ref = R.confusion(pred, tgt, C)
    assert ref[65535:].sum() > 0 and ref.sum() < N
    pred_d, tgt_d = _dev(pred, torch.uint8), _dev(tgt, torch.int64)
    counts = torch.zeros(N, C, C, dtype=torch.int32, device=DEV)
    _run(_confusion_op(pred_d, tgt_d, counts, C))
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref)
    from robocupvision_amd.metrics import PatchMetrics
    pm = PatchMetrics(C, DEV)
    pm.update(pred_d.reshape(N), tgt_d.reshape(N))
    assert np.array_equal(pm.conf.cpu().numpy(), ref.sum(0))


# ------------------------------------------------------------------------------------------ pointwise ops
def _stream_planes():
    return [K.PLANES[3], K.big_planes(_cus())["streaming"][1]]


@pytest.mark.parametrize("big", [False, True])
def test_combine_concat_materialize_add_slice_exact(big):
    """RCV_OP_COMBINE (three skip modes), RCV_F_CONCAT, RCV_OP_MATERIALIZE (three modes) and RCV_OP_ADD_SLICE (Ca < C) on the integer
    grid, on an odd plane and on one beyond a streaming grid pass."""
    N, H, W = _stream_planes()[int(big)]
    C, Ca = 8, 4
    if big:
        assert N * H * W * (Ca // 4) > 256 * 8 * _cus()
    rng = np.random.default_rng(40 + big)
    t, r, a = (R.grid(rng, (N, H, W, ch), 2) for ch in (C, C, Ca))
    tc, rc, ac = (R.grid_consts(rng, ch, scales=(0.5, -0.5, 1.0, -1.0, 2.0, -2.0)) for ch in (C, C, Ca))
    t_d, r_d, a_d, tc_d, rc_d, ac_d = (_dev(x) for x in (t, r, a, tc, rc, ac))
    relu_t = np.maximum(R.load(t, tc, R.LOAD_AFFINE), 0.0)
    for mode in (L.LOAD_PLAIN, L.LOAD_AFFINE, L.LOAD_AFFINE_RELU):
        out, cat, mat = _nan(N, H, W, C), _nan(N, H, W, 2 * C), _nan(N, H, W, C)
        x_d = _dev(t)
        kw = dict(n=N, h=H, w=W, cout=C, inmode2=mode, p_in=t_d.data_ptr(), p_in_c=tc_d.data_ptr(), p_in2=r_d.data_ptr(), p_in2_c=rc_d.data_ptr())
        ops = [L.make_op(L.OP_COMBINE, 0, p_out=out.data_ptr(), **kw), L.make_op(L.OP_COMBINE, L.F_CONCAT, p_out=cat.data_ptr(), **kw),
               L.make_op(L.OP_MATERIALIZE, 0, n=N, h=H, w=W, cout=C, inmode=mode, p_in=r_d.data_ptr(), p_in_c=rc_d.data_ptr(), p_out=mat.data_ptr()),
               L.make_op(L.OP_ADD_SLICE, 0, n=N, h=H, w=W, cin=Ca, cout=C, inmode=mode, p_in=a_d.data_ptr(), p_in_c=ac_d.data_ptr(), p_out=x_d.data_ptr())]
        assert [_label(o) for o in ops] == ["combine", "combine", "materialize", "add_slice"]
        _run(*ops)
        fr = R.load(r, rc, mode)
        _exact(out, relu_t + fr, "combine mode %d" % mode)
        _exact(cat, np.concatenate([relu_t, fr], -1), "concat mode %d" % mode)
        _exact(mat, fr, "materialize mode %d" % mode)
        ref = t.astype(np.float64)
        ref[..., :Ca] += R.load(a, ac, mode)
        _exact(x_d, ref, "add_slice mode %d" % mode)


@pytest.mark.parametrize("big", [False, True])
def test_layout_changes_exact(big):
    """RCV_OP_NHWC_TO_NCHW (+ bias) and RCV_OP_NCHW_TO_NHWC for 1..8 channels of the 8 padded ones."""
    N, H, W = _stream_planes()[int(big)]
    if big:
        assert N * H * W > 256 * 8 * _cus()
    rng = np.random.default_rng(60 + big)
    x = R.grid(rng, (N, H, W, 8), 2)
    x_d = _dev(x)
    for C in ((1, 5, 8) if big else range(1, 9)):
        bias = R.grid(rng, (C,), 2)
        nchw, back, b_d = _nan(N, C, H, W), _nan(N, H, W, 8), _dev(bias)
        a = L.make_op(L.OP_NHWC_TO_NCHW, 0, n=N, h=H, w=W, cin=8, cout=C, p_in=x_d.data_ptr(), p_bias=b_d.data_ptr(), p_out=nchw.data_ptr())
        b = L.make_op(L.OP_NCHW_TO_NHWC, 0, n=N, h=H, w=W, cin=C, cout=8, p_in=nchw.data_ptr(), p_out=back.data_ptr())
        assert _label(a) == "nhwc_to_nchw" and _label(b) == "nchw_to_nhwc"
        _run(a, b)
        ref = x[..., :C].astype(np.float64).transpose(0, 3, 1, 2) + bias[None, :, None, None]
        _exact(nchw, ref, "nhwc_to_nchw %d channels" % C)
        pad = np.zeros((N, H, W, 8))
        pad[..., :C] = ref.transpose(0, 2, 3, 1)
        _exact(back, pad, "nchw_to_nhwc %d channels" % C)
        nobias = _nan(N, C, H, W)
        a.p[L.RCV_P_BIAS], a.p[L.RCV_P_OUT] = None, nobias.data_ptr()
        _run(a)
        _exact(nobias, x[..., :C].astype(np.float64).transpose(0, 3, 1, 2), "nhwc_to_nchw without bias")
