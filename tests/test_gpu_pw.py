"""GPU: the pointwise (1x1) convolution family and the cross filters (csrc/conv_pw.hip) through the C ABI, one record per case, against
the float64 restatement tests/pw_restatement.py (itself pinned to torch's float64 conv2d by tests/test_rest.py).

Pixels (N, H, W): (1, 1, 1) one pixel, (2, 9, 13) = 234 pixels, a multiple of no tile (64-pixel chunks, 128- and 256-pixel tiles) inside
one tile, (3, 16, 20) = 960 pixels: several tiles and a ragged last one.  Channels: the reference's plans from trConvSep(16, 8) to
128 -> 128, every accumulator shape of the kernels (1, 2, 4, 8 blocks of 16 output channels; 1, 2, 4 filter blocks per wave).
Bars, those of tests/test_gpu_kernels.py (K <= 128 products per output is below the 1 152 they already cover), relative to the largest
float64 entry: convolutions 3e-6, filter gradients 5e-7; the float64 sum of the statistics rows within close(rtol=1e-4, floor=1.0).

At those pixel counts every workgroup of pw_kernel and pw_wgrad_kernel takes its tile / chunk loop once.  The second half of the file
runs the shapes of tests/persistent_cases.py, 263 700 and 131 850 pixels -- 1031 tiles over 512 workgroups, 4121 / 2061 chunks over
1024 / 512 / 256 rows: three rounds or more with a ragged last one -- on small-integer operands, where the result must equal the
float64 restatement bit for bit, and on randn operands under the load transforms at the bars above; then RCV_OP_PW_WGRAD_REDUCE alone
around every edge of its loops against its documented order, and the forms the engine never emits: i[AUX0] = 8 (pw_wgrad_kernel<8>),
RCV_LOAD_AFFINE, RCV_LOAD_GRAD_ENC and RCV_STATS_BWD_ENC."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pw_restatement as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PIXELS = [(1, 1, 1), (2, 9, 13), (3, 16, 20)]
PAIRS = [(8, 8), (16, 8), (16, 16), (32, 16), (128, 64), (128, 128)]
# the kernel forms those pairs leave out: two 16-channel output blocks per wave (32 outputs), 2 and 4 filter blocks per wave of the
# filter gradient (64 x 32, 64 x 64), and channel counts that are no multiple of 16 on either side (a half-filled last block)
PAIRS += [(32, 32), (64, 32), (64, 64), (24, 40)]
NAN = float("nan")


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


GUARD = 1024      # floats behind every output: a store past the tensor lands here and is seen


def _guarded(*shape):
    """A NaN-filled tensor of ``shape`` followed, in the same allocation, by GUARD floats of a sentinel: (view, whole buffer)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + GUARD,), NAN, device=DEV)
    buf[n:] = -12345.0
    return buf[:n].view(*shape), buf


def _guard_intact(buf):
    return bool((buf[-GUARD:] == -12345.0).all())


def _run_twice(L, h, op, out_shape, stats_cols):
    """Runs the record twice into NaN-filled outputs and NaN-filled partial rows, each with a guard band behind it; returns (out, rows)
    of the first run after checking that the second is bitwise equal, that no element kept a NaN and that nothing was stored past
    either tensor."""
    got = []
    for _ in range(2):
        out, out_buf = _guarded(*out_shape)
        op.p[L.RCV_P_OUT] = out.data_ptr()
        part = part_buf = None
        if stats_cols:
            nbytes = L.op_workspace(h, op)
            n_part = op.i[L.RCV_I_NPART]
            assert n_part > 0 and nbytes == n_part * 2 * stats_cols * 4
            part, part_buf = _guarded(n_part, 2, stats_cols)
            op.p[L.RCV_P_PART] = part.data_ptr()
        L.OpList([op]).run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _guard_intact(out_buf) and (part_buf is None or _guard_intact(part_buf)), "a store past the tensor"
        got.append((out.cpu(), None if part is None else part.cpu()))
    assert torch.equal(got[0][0], got[1][0]), "two runs differ"
    assert not bool(torch.isnan(got[0][0]).any()), "an output element was not written"
    if stats_cols:
        assert torch.equal(got[0][1], got[1][1]) and not bool(torch.isnan(got[0][1]).any()), "a partial row was not written (or differs)"
    return got[0]


@pytest.mark.parametrize("cin,cout", PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("N,H,W", PIXELS, ids=lambda v: str(v))
def test_pointwise_conv_records_vs_fp64(N, H, W, cin, cout):
    """RCV_OP_PW in the four forms the engine emits: the training forward (RCV_LOAD_PLAIN and RCV_LOAD_AFFINE_RELU, RCV_STATS_FWD), the
    folded inference forward (per-channel filter factor, bias, ReLU) and the data gradient (RCV_F_TRANSPOSED_SRC, RCV_LOAD_GRAD_DEC on
    dy with its aux tensor, a residual, RCV_STATS_BWD_DEC).  NaN-filled outputs and partial rows; two runs bitwise equal.
    Measured (MI355X), largest over the pixel counts and channel pairs: plain 4.7e-07, affine_relu 3.8e-07, folded 4.9e-07, data gradient 3.4e-07
    (all at 128 input channels; <= 2.7e-07 at 32 and fewer)."""
    from robocupvision_amd import _lib as L
    from test_gpu_blocks import close
    h = L.handle(0)
    gen = torch.Generator().manual_seed(9000 + 17 * N * H * W + 3 * cin + cout)
    x, xa, c = _rand(gen, N, H, W, cin), _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    w, wt = _rand(gen, cout, cin, 1, 1, scale=0.1), _rand(gen, cin, cout, 1, 1, scale=0.1)
    bias, scale = _rand(gen, cout), torch.rand(cout, generator=gen) + 0.5
    resid, e, ec = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 3, cout, scale=0.5)
    dev = {k: v.to(DEV) for k, v in dict(x=x, xa=xa, c=c, w=w, wt=wt, bias=bias, scale=scale, resid=resid, e=e, ec=ec).items()}
    base = dict(n=N, h=H, w=W, cin=cin, cout=cout, p_in=dev["x"].data_ptr(), p_in_c=dev["c"].data_ptr())
    cases = {
        "plain": (L.make_op(L.OP_PW, 0, inmode=L.LOAD_PLAIN, stats=L.STATS_FWD, p_w=dev["w"].data_ptr(), **base),
                  lambda: R.pw_conv(R.load(R.LOAD_PLAIN, x), w), 1),
        "affine_relu": (L.make_op(L.OP_PW, 0, inmode=L.LOAD_AFFINE_RELU, stats=L.STATS_FWD, p_w=dev["w"].data_ptr(), **base),
                        lambda: R.pw_conv(R.load(R.LOAD_AFFINE_RELU, x, c), w), 1),
        "folded": (L.make_op(L.OP_PW, L.F_BIAS | L.F_RELU, inmode=L.LOAD_PLAIN, p_w=dev["w"].data_ptr(), p_x0=dev["scale"].data_ptr(),
                             p_bias=dev["bias"].data_ptr(), **base),
                   lambda: R.pw_conv(R.load(R.LOAD_PLAIN, x), w, scale=scale, bias=bias, relu=True), 0),
        "dgrad": (L.make_op(L.OP_PW, L.F_TRANSPOSED_SRC | L.F_RESID, inmode=L.LOAD_GRAD_DEC, stats=L.STATS_BWD_DEC, p_w=dev["wt"].data_ptr(),
                            p_in_aux=dev["xa"].data_ptr(), p_resid=dev["resid"].data_ptr(), p_epi_aux=dev["e"].data_ptr(),
                            p_epi_c=dev["ec"].data_ptr(), **base),
                  lambda: R.pw_conv(R.load(R.LOAD_GRAD_DEC, x, c, xa), wt, transposed=True, resid=resid), 3),
    }
    for name, (op, ref_fn, stats) in cases.items():
        ref = ref_fn()
        label = L.OpList([op]).labels(h)[0]
        assert label.startswith("pw_mfma<") and label.endswith(",t>") == (name == "dgrad"), label
        out, rows = _run_twice(L, h, op, (N, H, W, cout), cout if stats else 0)
        err = float((out.double() - ref).abs().max() / ref.abs().max())
        print(".%s %s %s: max error %.3e" % (label, (N, H, W, cin, cout), name, err))
        assert err <= 3e-6, (label, name, err)
        if stats:
            close(rows.double().sum(0), R.stats_rows(stats, ref, e, ec), "%s %s statistics rows" % (label, name), rtol=1e-4, floor=1.0)


@pytest.mark.parametrize("cin,cout", PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("N,H,W", PIXELS, ids=lambda v: str(v))
def test_pointwise_filter_gradient_vs_fp64(N, H, W, cin, cout):
    """RCV_OP_PW_WGRAD + RCV_OP_PW_WGRAD_REDUCE as bwd_pw emits them: the layer input through RCV_LOAD_PLAIN / RCV_LOAD_AFFINE_RELU, the
    output gradient through RCV_LOAD_GRAD_DEC (and plain).  NaN-filled partial rows and gradient; two runs bitwise equal (no atomics).
    Measured (MI355X): <= 2.1e-07 over all cases."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(9500 + 17 * N * H * W + 3 * cin + cout)
    x, xc = _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    dy, dya, dyc = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 5, cout, scale=0.5)
    xd, xcd, dyd, dyad, dycd = (v.to(DEV) for v in (x, xc, dy, dya, dyc))
    for xm, gm in ((L.LOAD_PLAIN, L.LOAD_GRAD_DEC), (L.LOAD_AFFINE_RELU, L.LOAD_GRAD_DEC), (L.LOAD_AFFINE_RELU, L.LOAD_PLAIN)):
        ref = R.pw_wgrad(R.load(xm, x, xc), R.load(gm, dy, dyc, dya))
        got = []
        for _ in range(2):
            wop = L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, cin=cin, cout=cout, inmode=xm, inmode2=gm, p_in=xd.data_ptr(), p_in_c=xcd.data_ptr(),
                            p_in2=dyd.data_ptr(), p_in2_aux=dyad.data_ptr(), p_in2_c=dycd.data_ptr())
            nbytes = L.op_workspace(h, wop)
            ns = wop.i[L.RCV_I_NSPLIT]
            assert ns == R.wgrad_rows(N * H * W, cin, cout, L.load().rcv_num_cus(h)) and nbytes == ns * cin * cout * 4
            (part, part_buf), (dw, dw_buf) = _guarded(ns, cout, cin), _guarded(cout, cin)
            wop.p[L.RCV_P_PART] = part.data_ptr()
            red = L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=ns, p_part=part.data_ptr(), p_out=dw.data_ptr())
            lst = L.OpList([wop, red])
            labels = lst.labels(h)
            lst.run(h, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert _guard_intact(part_buf) and _guard_intact(dw_buf), "a store past the tensor"
            got.append((dw.cpu(), part.cpu()))
        assert not bool(torch.isnan(got[0][1]).any()), "a partial row was not written"
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "two runs differ"
        err = float((got[0][0].double() - ref).abs().max() / ref.abs().max())
        print(".%s %s modes %d/%d: max error %.3e" % (labels[0], (N, H, W, cin, cout), xm, gm, err))
        assert err <= 5e-7, (labels[0], xm, gm, err)


@pytest.mark.parametrize("form,a_shape,b_shape", [(0, (16, 16, 3, 1), (16, 16, 1, 3)), (0, (64, 64, 3, 1), (64, 64, 1, 3)),
                                                  (1, (16, 16, 1, 3), (16, 16, 3, 1)), (1, (64, 64, 1, 3), (64, 64, 3, 1)),
                                                  (0, (3, 5, 3, 1), (3, 5, 1, 3)), (1, (5, 3, 1, 3), (5, 3, 3, 1))])
def test_cross_pack_and_gather_are_exact(form, a_shape, b_shape):
    """RCV_OP_CROSS_PACK writes every element of the dense filter (NaN-filled before), bit for bit the restatement; RCV_OP_CROSS_GRAD
    gathers a gradient back, the centre tap of the summed form to both filters."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(31 + form)
    a, b = _rand(gen, *a_shape), _rand(gen, *b_shape)
    D0, D1 = (2 * a_shape[0] if form == 0 else a_shape[0]), a_shape[1]
    ad, bd = a.to(DEV), b.to(DEV)
    dense = torch.full((D0, D1, 3, 3), NAN, device=DEV)
    L.OpList([L.make_op(L.OP_CROSS_PACK, 0, cout=D0, cin=D1, aux0=form, p_in=ad.data_ptr(), p_in2=bd.data_ptr(), p_out=dense.data_ptr())]).run(
        h, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(dense.cpu(), R.cross_pack(a, b, form))
    g = _rand(gen, D0, D1, 3, 3)
    gd = g.to(DEV)
    ga, gb = torch.full(a_shape, NAN, device=DEV), torch.full(b_shape, NAN, device=DEV)
    L.OpList([L.make_op(L.OP_CROSS_GRAD, 0, cout=D0, cin=D1, aux0=form, p_in=gd.data_ptr(), p_out=ga.data_ptr(), p_x0=gb.data_ptr())]).run(
        h, torch.cuda.current_stream().cuda_stream)
    ra, rb = R.cross_grad(g, form)
    assert torch.equal(ga.cpu(), ra) and torch.equal(gb.cpu(), rb)


# ------------------------------------------------------------------------------------------ beyond the first tile round
# tests/persistent_cases.py: the shapes at which a workgroup of pw_kernel / pw_wgrad_kernel walks three rounds or more of its loop
# `for (t = blockIdx.x; t < n; t += gridDim.x)` with a ragged last one; every case guards that on the real handle.
import persistent_cases as PCS      # noqa: E402

EXACT = float(1 << 24)      # every integer of magnitude below 2^24 is an fp32 number: sums that stay below it are exact in any order


def _ints(gen, *shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _case_id(case):
    return "%dx%d-%s" % (case[0], case[1], "x".join(map(str, case[2])))


def _wgrad_twice(L, h, make_wop, cin, cout):
    """RCV_OP_PW_WGRAD (built by make_wop(), its workspace attached here) + RCV_OP_PW_WGRAD_REDUCE twice into NaN-filled partial rows
    and a NaN-filled gradient, each with a guard band; -> (dW, rows, label, row count) of the first run after checking that the
    second is bitwise equal, that no element kept a NaN and that nothing was stored past either tensor."""
    got = []
    for _ in range(2):
        wop = make_wop()
        nbytes = L.op_workspace(h, wop)
        ns = wop.i[L.RCV_I_NSPLIT]
        assert ns > 0 and nbytes == ns * cin * cout * 4
        (part, part_buf), (dw, dw_buf) = _guarded(ns, cout, cin), _guarded(cout, cin)
        wop.p[L.RCV_P_PART] = part.data_ptr()
        red = L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=ns, p_part=part.data_ptr(), p_out=dw.data_ptr())
        lst = L.OpList([wop, red])
        labels = lst.labels(h)
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _guard_intact(part_buf) and _guard_intact(dw_buf), "a store past the tensor"
        got.append((dw.cpu(), part.cpu()))
    assert not bool(torch.isnan(got[0][1]).any()), "a partial row was not written"
    assert not bool(torch.isnan(got[0][0]).any()), "a gradient element was not written"
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "two runs differ"
    return got[0][0], got[0][1], labels[0], ns


@pytest.mark.parametrize("case", PCS.PW_CASES, ids=_case_id)
def test_multi_round_pointwise_integers_are_exact(case):
    """RCV_OP_PW plain, folded (integer filter factor 1..3, bias, ReLU) and as the data gradient (RCV_F_TRANSPOSED_SRC, RCV_F_RESID), all
    under RCV_LOAD_PLAIN, at 1031 tiles over 512 workgroups: integer operands |x|, |w|, |bias|, |resid| <= 4, so that every fp32 sum
    is an integer of magnitude at most Cin * 4 * (4 * 3) + 4 + 4 <= 6152 < 2^24 (asserted from the operands) and the result equals the
    float64 restatement bit for bit: a skipped, doubled or misplaced tile or pixel shows at any tolerance."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    cin, cout, (N, H, W), _ = case
    gen = torch.Generator().manual_seed(9900 + 3 * cin + cout)
    x, w, wt = _ints(gen, N, H, W, cin), _ints(gen, cout, cin, 1, 1), _ints(gen, cin, cout, 1, 1)
    bias, scale, resid = _ints(gen, cout), _ints(gen, cout, lo=1, hi=3), _ints(gen, N, H, W, cout)
    bound = cin * float(x.abs().max()) * float(max(w.abs().max(), wt.abs().max())) * float(scale.abs().max()) \
        + float(bias.abs().max()) + float(resid.abs().max())
    assert bound < EXACT, bound
    dev = {k: v.to(DEV) for k, v in dict(x=x, w=w, wt=wt, bias=bias, scale=scale, resid=resid).items()}
    forms = {
        "plain": (dict(p_w=dev["w"].data_ptr()), lambda: R.pw_conv(x, w, matmul=True)),
        "folded": (dict(p_w=dev["w"].data_ptr(), p_x0=dev["scale"].data_ptr(), p_bias=dev["bias"].data_ptr()),
                   lambda: R.pw_conv(x, w, scale=scale, bias=bias, relu=True, matmul=True)),
        "dgrad": (dict(p_w=dev["wt"].data_ptr(), p_resid=dev["resid"].data_ptr()),
                  lambda: R.pw_conv(x, wt, transposed=True, resid=resid, matmul=True)),
    }
    assert tuple(forms) == PCS.PW_EXACT_FORMS
    for form, (ptrs, ref_fn) in forms.items():
        op = PCS.pw_record(case, form, p_in=dev["x"].data_ptr(), **ptrs)
        grid, tiles = PCS.assert_multi_round(op, h, PCS.pw_pin(case, form))
        out, _ = _run_twice(L, h, op, (N, H, W, cout), 0)
        ref = ref_fn()
        assert float(ref.abs().max()) <= bound
        wrong = int((out.double() != ref).sum())
        assert wrong == 0, "%s %s: %d of %d elements differ (%d tiles over %d workgroups)" % (PCS.pw_pin(case, form)[0], form, wrong, ref.numel(), tiles, grid)


@pytest.mark.parametrize("case", PCS.PW_WGRAD_CASES, ids=_case_id)
def test_multi_round_pointwise_filter_gradient_integers_are_exact(case):
    """RCV_OP_PW_WGRAD + RCV_OP_PW_WGRAD_REDUCE, plain / plain, at 4121 chunks over 1024 or 512 rows and 2061 over 256: integer operands
    |x|, |g| <= 4.  Every partial sum of an accumulator, of a row and of the reduction is an integer of magnitude at most
    max over (co, ci) of sum_p |g[p][co]| |x[p][ci]| (<= 16 * 263 700 = 4 219 200), asserted below 2^24 from the operands: the gradient
    equals the float64 restatement bit for bit, and so does the float64 sum of the partial rows."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    cin, cout, (N, H, W), pin = case
    gen = torch.Generator().manual_seed(9950 + 3 * cin + cout)
    x, g = _ints(gen, N, H, W, cin), _ints(gen, N, H, W, cout)
    bound = float(R.pw_wgrad(x.abs(), g.abs(), matmul=True).max())
    assert bound < EXACT, bound
    xd, gd = x.to(DEV), g.to(DEV)
    make = lambda: PCS.pw_wgrad_record(case, p_in=xd.data_ptr(), p_in2=gd.data_ptr())
    rows, chunks = PCS.assert_multi_round(make(), h, pin)
    dw, part, label, ns = _wgrad_twice(L, h, make, cin, cout)
    assert (label, ns) == (pin[0], rows)
    ref = R.pw_wgrad(x, g, matmul=True)
    wrong = int((dw.double() != ref).sum())
    assert wrong == 0, "%s: %d of %d elements differ (%d chunks over %d rows)" % (label, wrong, ref.numel(), chunks, rows)
    assert torch.equal(part.double().sum(0), ref), "the partial rows do not add up to the gradient"


def test_multi_round_pointwise_random_operands_vs_fp64():
    """randn operands at 1031 tiles over 512 workgroups, 24 -> 40 channels (pw_mfma<4,4>): RCV_LOAD_AFFINE_RELU + RCV_STATS_FWD, and the
    data gradient under RCV_LOAD_GRAD_DEC with a residual and RCV_STATS_BWD_DEC.  The products per output do not grow with the rounds:
    the bar of test_pointwise_conv_records_vs_fp64 stands, 3e-6 of the largest float64 entry; the float64 sum of the 1031 statistics
    rows within close(rtol=1e-4, floor=1.0).
    Measured (MI355X): affine_relu 2.4e-07, data gradient 1.6e-07."""
    from robocupvision_amd import _lib as L
    from test_gpu_blocks import close
    h = L.handle(0)
    case = PCS.PW_RANDOM_CASE
    cin, cout, (N, H, W), _ = case
    gen = torch.Generator().manual_seed(9970)
    x, xa, c = _rand(gen, N, H, W, cin), _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    w, wt = _rand(gen, cout, cin, 1, 1, scale=0.1), _rand(gen, cin, cout, 1, 1, scale=0.1)
    resid, e, ec = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 3, cout, scale=0.5)
    dev = {k: v.to(DEV) for k, v in dict(x=x, xa=xa, c=c, w=w, wt=wt, resid=resid, e=e, ec=ec).items()}
    forms = {
        "affine_relu": (dict(p_w=dev["w"].data_ptr()), lambda: R.pw_conv(R.load(R.LOAD_AFFINE_RELU, x, c), w, matmul=True), 1),
        "grad_dec": (dict(p_w=dev["wt"].data_ptr(), p_in_aux=dev["xa"].data_ptr(), p_resid=dev["resid"].data_ptr(),
                          p_epi_aux=dev["e"].data_ptr(), p_epi_c=dev["ec"].data_ptr()),
                     lambda: R.pw_conv(R.load(R.LOAD_GRAD_DEC, x, c, xa), wt, transposed=True, resid=resid, matmul=True), 3),
    }
    assert tuple(forms) == PCS.PW_RANDOM_FORMS
    for form, (ptrs, ref_fn, stats) in forms.items():
        op = PCS.pw_record(case, form, p_in=dev["x"].data_ptr(), p_in_c=dev["c"].data_ptr(), **ptrs)
        PCS.assert_multi_round(op, h, PCS.pw_pin(case, form))
        out, rows = _run_twice(L, h, op, (N, H, W, cout), cout)
        ref = ref_fn()
        err = float((out.double() - ref).abs().max() / ref.abs().max())
        print(".%s multi-round %s: max error %.3e" % (PCS.pw_pin(case, form)[0], form, err))
        assert err <= 3e-6, (form, err)
        close(rows.double().sum(0), R.stats_rows(stats, ref, e, ec), "multi-round %s statistics rows" % form, rtol=1e-4, floor=1.0)


def test_multi_round_pointwise_filter_gradient_random_operands_vs_fp64():
    """randn operands, x under RCV_LOAD_AFFINE_RELU and g under RCV_LOAD_GRAD_DEC, 64 x 64 channels at 4121 chunks over 512 rows
    (pw_wgrad_mfma<4,64,1>): an accumulator's fp32 chain is ceil(4121 / 512) * 64 = 576 products, against at most 64 * 15 at the shapes
    of test_pointwise_filter_gradient_vs_fp64; the rows are added in float64.  The bar of that test, 5e-7 of the largest float64 entry,
    is kept: the measured error leaves a factor 10 to spare (1.5 was asked for).
    Measured (MI355X): 4.7e-08."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    case = PCS.PW_WGRAD_RANDOM_CASE
    cin, cout, (N, H, W), pin = case
    gen = torch.Generator().manual_seed(9980)
    x, xc = _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    dy, dya, dyc = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 5, cout, scale=0.5)
    xd, xcd, dyd, dyad, dycd = (v.to(DEV) for v in (x, xc, dy, dya, dyc))
    make = lambda: PCS.pw_wgrad_record(case, L.LOAD_AFFINE_RELU, L.LOAD_GRAD_DEC, p_in=xd.data_ptr(), p_in_c=xcd.data_ptr(),
                                       p_in2=dyd.data_ptr(), p_in2_aux=dyad.data_ptr(), p_in2_c=dycd.data_ptr())
    PCS.assert_multi_round(make(), h, pin)
    dw, part, label, ns = _wgrad_twice(L, h, make, cin, cout)
    ref = R.pw_wgrad(R.load(R.LOAD_AFFINE_RELU, x, xc), R.load(R.LOAD_GRAD_DEC, dy, dyc, dya), matmul=True)
    err = float((dw.double() - ref).abs().max() / ref.abs().max())
    print(".%s multi-round affine_relu / grad_dec, %d rows: max error %.3e" % (label, ns, err))
    assert err <= 5e-7, (label, err)


# ------------------------------------------------------------------------------------------ the reduction's loop edges
@pytest.mark.parametrize("cin,cout", PCS.PW_REDUCE_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("nsplit", PCS.PW_REDUCE_NSPLIT)
def test_pointwise_reduction_order_is_the_documented_one(nsplit, cin, cout):
    """RCV_OP_PW_WGRAD_REDUCE alone on partial rows the test writes, around every edge of its loops (16 row lanes; four loads in
    flight while s + 48 < nsplit, then one at a time): bit for bit pw_restatement.pw_reduce -- lane l adds the rows l, l + 16, ... in
    float64, the 16 lane sums are added in lane order, the total is rounded once.  Twice: on randn rows, and on
    pw_restatement.order_sensitive_rows, where cancelling terms of 2^40 make the float64 additions round at 2^-12, so that another
    order gives another fp32 result (on randn rows the final rounding hides the order): asserted for the order with the rows l and
    l + 16 of every group of four exchanged."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(700 + 5 * nsplit + cin)
    for name, part in (("randn", _rand(gen, nsplit, cout, cin)), ("order-sensitive", R.order_sensitive_rows(gen, nsplit, cout, cin))):
        pd = part.to(DEV)
        dw, dw_buf = _guarded(cout, cin)
        L.OpList([L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=nsplit, p_part=pd.data_ptr(), p_out=dw.data_ptr())]).run(
            h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _guard_intact(dw_buf), "a store past the tensor"
        ref = R.pw_reduce(part)
        assert torch.equal(dw.cpu(), ref), "%s rows: %d of %d elements differ" % (name, int((dw.cpu() != ref).sum()), ref.numel())
        if nsplit >= 113 and name != "randn":      # (the first group of four starts from zero: its order cannot show)
            assert not torch.equal(R.pw_reduce(part, swap=True), ref), "these rows would not show a changed order"


# ------------------------------------------------------------------------------------------ the forms never launched before
@pytest.mark.parametrize("cin,cout", PCS.PW_CAP8_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("N,H,W", PIXELS, ids=lambda v: str(v))
def test_pointwise_filter_gradient_eight_blocks_per_wave(N, H, W, cin, cout):
    """RCV_OP_PW_WGRAD with i[AUX0] = 8 (up to eight 16 x 16 filter blocks per wave; pw_wgrad_kernel<8> at 128 input channels): the label
    from the launcher's rule, the modes and the bar of test_pointwise_filter_gradient_vs_fp64 (5e-7), and on integer operands
    (|x|, |g| <= 4, at most 960 pixels: sums below 15 360) bit for bit the float64 restatement AND the default cap's gradient and
    partial rows -- the chain of every element is the same whichever wave holds it.
    Measured (MI355X): <= 2.6e-07 over all cases (128 x 128 at 234 pixels, plain / grad_dec)."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    want = PCS.pw_cap_label(cin, cout, 8)
    assert want.startswith("pw_wgrad_mfma<8,") == (cin == 128) and ((cin, cout) != (128, 128) or want == "pw_wgrad_mfma<8,64,2>")
    gen = torch.Generator().manual_seed(9600 + 17 * N * H * W + 3 * cin + cout)
    x, xc = _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    dy, dya, dyc = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 5, cout, scale=0.5)
    xd, xcd, dyd, dyad, dycd = (v.to(DEV) for v in (x, xc, dy, dya, dyc))
    for xm, gm in ((L.LOAD_PLAIN, L.LOAD_GRAD_DEC), (L.LOAD_AFFINE_RELU, L.LOAD_GRAD_DEC), (L.LOAD_AFFINE_RELU, L.LOAD_PLAIN)):
        make = lambda: L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, cin=cin, cout=cout, inmode=xm, inmode2=gm, aux0=8, p_in=xd.data_ptr(),
                                 p_in_c=xcd.data_ptr(), p_in2=dyd.data_ptr(), p_in2_aux=dyad.data_ptr(), p_in2_c=dycd.data_ptr())
        dw, part, label, ns = _wgrad_twice(L, h, make, cin, cout)
        assert label == want and ns == R.wgrad_rows(N * H * W, cin, cout, L.load().rcv_num_cus(h)), (label, want, ns)
        ref = R.pw_wgrad(R.load(xm, x, xc), R.load(gm, dy, dyc, dya))
        err = float((dw.double() - ref).abs().max() / ref.abs().max())
        print(".%s %s modes %d/%d: max error %.3e" % (label, (N, H, W, cin, cout), xm, gm, err))
        assert err <= 5e-7, (label, xm, gm, err)
    xi, gi = _ints(gen, N, H, W, cin), _ints(gen, N, H, W, cout)
    assert 16 * N * H * W < EXACT
    xid, gid = xi.to(DEV), gi.to(DEV)
    got = {}
    for cap in (0, 8):
        make = lambda: L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, cin=cin, cout=cout, aux0=cap, p_in=xid.data_ptr(), p_in2=gid.data_ptr())
        got[cap] = _wgrad_twice(L, h, make, cin, cout)
    assert got[0][2] == PCS.pw_cap_label(cin, cout, 4) and got[8][2] == want, (got[0][2], got[8][2])
    assert torch.equal(got[8][0].double(), R.pw_wgrad(xi, gi)), "i[AUX0] = 8 on integers"
    assert torch.equal(got[8][0], got[0][0]) and torch.equal(got[8][1], got[0][1]), "i[AUX0] = 8 and the default cap differ"


@pytest.mark.parametrize("cin,cout", [(16, 8), (24, 40), (128, 128)], ids=lambda v: str(v))
@pytest.mark.parametrize("N,H,W", PIXELS, ids=lambda v: str(v))
def test_pointwise_records_under_affine_and_grad_enc_vs_fp64(N, H, W, cin, cout):
    """The load and statistics modes the ABI takes and the engine does not emit: RCV_OP_PW under RCV_LOAD_AFFINE (RCV_STATS_FWD) and,
    as the data gradient, under RCV_LOAD_GRAD_ENC with a residual and RCV_STATS_BWD_ENC; RCV_OP_PW_WGRAD with x under RCV_LOAD_AFFINE
    and g under RCV_LOAD_GRAD_ENC.  The bars of the tests above: 3e-6, 5e-7, close(rtol=1e-4, floor=1.0).
    Measured (MI355X), largest over the cases: affine 4.6e-07 (128 input channels; <= 2.1e-07 at 24 and fewer), grad_enc 2.1e-07, filter
    gradient 1.1e-07."""
    from robocupvision_amd import _lib as L
    from test_gpu_blocks import close
    h = L.handle(0)
    gen = torch.Generator().manual_seed(9700 + 17 * N * H * W + 3 * cin + cout)
    x, xa, c = _rand(gen, N, H, W, cin), _rand(gen, N, H, W, cin), _rand(gen, 5, cin, scale=0.5)
    w, wt = _rand(gen, cout, cin, 1, 1, scale=0.1), _rand(gen, cin, cout, 1, 1, scale=0.1)
    resid, e, ec = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 3, cout, scale=0.5)
    dev = {k: v.to(DEV) for k, v in dict(x=x, xa=xa, c=c, w=w, wt=wt, resid=resid, e=e, ec=ec).items()}
    base = dict(n=N, h=H, w=W, cin=cin, cout=cout, p_in=dev["x"].data_ptr(), p_in_c=dev["c"].data_ptr())
    cases = {
        "affine": (L.make_op(L.OP_PW, 0, inmode=L.LOAD_AFFINE, stats=L.STATS_FWD, p_w=dev["w"].data_ptr(), **base),
                   lambda: R.pw_conv(R.load(R.LOAD_AFFINE, x, c), w), 1),
        "grad_enc": (L.make_op(L.OP_PW, L.F_TRANSPOSED_SRC | L.F_RESID, inmode=L.LOAD_GRAD_ENC, stats=L.STATS_BWD_ENC, p_w=dev["wt"].data_ptr(),
                               p_in_aux=dev["xa"].data_ptr(), p_resid=dev["resid"].data_ptr(), p_epi_aux=dev["e"].data_ptr(),
                               p_epi_c=dev["ec"].data_ptr(), **base),
                     lambda: R.pw_conv(R.load(R.LOAD_GRAD_ENC, x, c, xa), wt, transposed=True, resid=resid), 2),
    }
    for name, (op, ref_fn, stats) in cases.items():
        ref = ref_fn()
        label = L.OpList([op]).labels(h)[0]
        assert label.startswith("pw_mfma<") and label.endswith(",t>") == (name == "grad_enc"), label
        out, rows = _run_twice(L, h, op, (N, H, W, cout), cout)
        err = float((out.double() - ref).abs().max() / ref.abs().max())
        print(".%s %s %s: max error %.3e" % (label, (N, H, W, cin, cout), name, err))
        assert err <= 3e-6, (label, name, err)
        close(rows.double().sum(0), R.stats_rows(stats, ref, e, ec), "%s %s statistics rows" % (label, name), rtol=1e-4, floor=1.0)
    # the filter gradient: x (cin channels) under AFFINE, the output gradient (cout channels) under GRAD_ENC
    dy, dya, dyc = _rand(gen, N, H, W, cout), _rand(gen, N, H, W, cout), _rand(gen, 5, cout, scale=0.5)
    dyd, dyad, dycd = dy.to(DEV), dya.to(DEV), dyc.to(DEV)
    make = lambda: L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, cin=cin, cout=cout, inmode=L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_ENC,
                             p_in=dev["x"].data_ptr(), p_in_c=dev["c"].data_ptr(), p_in2=dyd.data_ptr(), p_in2_aux=dyad.data_ptr(),
                             p_in2_c=dycd.data_ptr())
    dw, part, label, ns = _wgrad_twice(L, h, make, cin, cout)
    ref = R.pw_wgrad(R.load(R.LOAD_AFFINE, x, c), R.load(R.LOAD_GRAD_ENC, dy, dyc, dya))
    err = float((dw.double() - ref).abs().max() / ref.abs().max())
    print(".%s %s affine / grad_enc: max error %.3e" % (label, (N, H, W, cin, cout), err))
    assert err <= 5e-7, (label, err)
