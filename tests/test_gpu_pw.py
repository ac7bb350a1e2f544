"""GPU: the pointwise (1x1) convolution family and the cross filters (csrc/conv_pw.hip) through the C ABI, one record per case, against
the float64 restatement tests/pw_restatement.py (itself pinned to torch's float64 conv2d by tests/test_rest.py).

Pixels (N, H, W): (1, 1, 1) one pixel, (2, 9, 13) = 234 pixels, a multiple of no tile (64-pixel chunks, 128- and 256-pixel tiles) inside
one tile, (3, 16, 20) = 960 pixels: several tiles and a ragged last one.  Channels: the reference's plans from trConvSep(16, 8) to
128 -> 128, every accumulator shape of the kernels (1, 2, 4, 8 blocks of 16 output channels; 1, 2, 4 filter blocks per wave).
Bars, those of tests/test_gpu_kernels.py (K <= 128 products per output is below the 1 152 they already cover), relative to the largest
float64 entry: convolutions 3e-6, filter gradients 5e-7; the float64 sum of the statistics rows within close(rtol=1e-4, floor=1.0)."""
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
