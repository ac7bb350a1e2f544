"""The 5x5 classifier convolution family (csrc/conv5.hip) on the device.

Exact cases: small-integer operands (|x|, |w| <= 4), so every fp32 sum is exact (25 * 16 products of at most 16, and at most
3 * 17 * 33 pixels in a filter gradient, stay far below 2^24): forward, data gradient with and without RCV_F_RESID, filter and bias
gradient equal the float64 restatement (tests/cls5_restatement.py) bit for bit -- a wrong tap, halo or pad index shows at any tolerance.
Planes: 3x4 (every window leaves the plane), 5x7, one tile of the kernel (8x32; 16x16 for planes at most 16 wide) and one tile +- 1 in
each dimension, 17x33.

Random cases on the same planes under every load mode the kernels take (PLAIN, AFFINE, AFFINE_RELU; the lowering hands the classifier
PLAIN), at the bars of tests/test_gpu_kernels.py relative to the largest entry of the float64 result: convolutions 3e-6, filter
gradients 5e-7, bias gradients 5e-7 (K <= 400 products per output, below the 1 152 those bars already cover); statistics rows within
close(rtol=1e-4, floor=1.0).
Measured maxima (MI355X): convolutions <= 7.9e-7, filter gradients <= 2.8e-7, bias gradients <= 2.4e-7; per kernel label in the docstring
of test_random_operands_vs_fp64.

Multi-round cases (tests/persistent_cases.py): on the planes above a workgroup of conv5_kernel / wgrad5_kernel takes its tile loop
once (at most 9 tiles).  11 x 121 x 161 (1056 tiles of 8x32) and 345 x 33 x 16 (1035 tiles of 16x16) give every workgroup three
rounds or more with a ragged last one: exact on small integers, statistics rows included, and randn at the bars above; then
RCV_OP_WGRAD5_REDUCE alone against its documented order.
Measured (MI355X) at 1056 tiles: forward 6.2e-7, data gradient 4.4e-7, filter gradient 2.2e-7, bias gradient 1.4e-7.

Whole steps against tests/golden/cls5.npz and `predict` follow further down."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cls5_restatement as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# 8x32 is the kernel's tile for planes wider than 16, 16x16 the one for the others (label "...<CIN,RxWt>")
PLANES = [(3, 4), (5, 7), (8, 32), (7, 31), (9, 33), (17, 33), (16, 16), (15, 15), (17, 16)]
BATCHES = (1, 3)
CLASSES = (1, 5, 8)
MODES = {"plain": R.LOAD_PLAIN, "affine": R.LOAD_AFFINE, "affine_relu": R.LOAD_AFFINE_RELU}
_MAXIMA = {}


def _note(label, err):
    _MAXIMA[label] = max(_MAXIMA.get(label, 0.0), err)


def _L():
    from robocupvision_amd import _lib as L
    return L, L.handle(0)


def _run(L, h, ops):
    lst = L.OpList(ops)
    labels = lst.labels(h)
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return labels


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).float()


def _packed(L, h, w, flip):
    """The filter through RCV_OP_PACK5, compared with the restatement's layout on the way."""
    Cout, Cin = w.shape[0], w.shape[1]
    wd = w.to(DEV)
    dst = torch.full((25, 8 if flip else Cin, 16), float("nan"), device=DEV)
    _run(L, h, [L.make_op(L.OP_PACK5, L.F_FLIP if flip else 0, cin=Cin, cout=Cout, p_in=wd.data_ptr(), p_out=dst.data_ptr())])
    assert torch.equal(dst.cpu().double(), R.pack5(w, flip)), "pack5 layout (flip=%d)" % flip
    return dst


def _conv5(L, h, x, c, mode, wp, cin, cout, flags=0, bias=None, resid=None, stats=0, e=None, epi_c=None):
    N, H, W, _ = x.shape
    keep = [v.to(DEV) if v is not None else None for v in (x, c, bias, resid, e, epi_c)]
    xd, cd, bd, rd, ed, ecd = keep
    out = torch.full((N, H, W, cout), float("nan"), device=DEV)
    op = L.make_op(L.OP_CONV5, flags, n=N, h=H, w=W, cin=cin, cout=cout, ho=H, wo=W, stride=1, dil=1, inmode=mode, stats=stats,
                   p_in=xd.data_ptr(), p_in_c=cd.data_ptr() if cd is not None else 0, p_w=wp.data_ptr(), p_out=out.data_ptr(),
                   p_bias=bd.data_ptr() if bd is not None else 0, p_resid=rd.data_ptr() if rd is not None else 0,
                   p_epi_aux=ed.data_ptr() if ed is not None else 0, p_epi_c=ecd.data_ptr() if ecd is not None else 0)
    part = None
    nbytes = L.op_workspace(h, op)
    if stats:
        assert nbytes == op.i[L.RCV_I_NPART] * 2 * cout * 4 and nbytes > 0
        part = torch.full((op.i[L.RCV_I_NPART], 2, cout), float("nan"), device=DEV)
        op.p[L.RCV_P_PART] = part.data_ptr()
    label = _run(L, h, [op])[0]
    return out.cpu(), (part.cpu() if part is not None else None), label


def _wgrad5(L, h, x, c, mode, g, cin, classes, with_bias=True):
    N, H, W, _ = x.shape
    xd, gd = x.to(DEV), g.to(DEV)
    cd = c.to(DEV) if c is not None else None
    wop = L.make_op(L.OP_WGRAD5, L.F_BIAS if with_bias else 0, n=N, h=H, w=W, cin=cin, cout=8, ho=H, wo=W, stride=1, dil=1, inmode=mode,
                    inmode2=L.LOAD_PLAIN, p_in=xd.data_ptr(), p_in_c=cd.data_ptr() if cd is not None else 0, p_in2=gd.data_ptr())
    nbytes = L.op_workspace(h, wop)
    assert nbytes == wop.i[L.RCV_I_NSPLIT] * (25 * 8 * 16 + 8) * 4
    part = torch.full((nbytes // 4,), float("nan"), device=DEV)
    wop.p[L.RCV_P_PART] = part.data_ptr()
    dw = torch.full((classes, cin, 5, 5), float("nan"), device=DEV)
    db = torch.full((classes,), float("nan"), device=DEV)
    rop = L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=cin, cout=classes, nsplit=wop.i[L.RCV_I_NSPLIT], p_part=part.data_ptr(),
                    p_out=dw.data_ptr(), p_bias=db.data_ptr() if with_bias else 0)
    labels = _run(L, h, [wop, rop])
    return dw.cpu(), db.cpu(), labels[0]


@pytest.mark.parametrize("cin", [8, 16])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_integer_operands_are_exact(plane, cin):
    """Forward (with and without RCV_F_BIAS), data gradient (with and without RCV_F_RESID), filter and bias gradient, N in {1, 3},
    classes in {1, 5, 8}: bitwise the float64 restatement."""
    L, h = _L()
    H, W = plane
    gen = torch.Generator().manual_seed(50 + 97 * H + W + cin)
    tile = "8x32" if W > 16 else "16x16"
    for N in BATCHES:
        for classes in CLASSES:
            x, w = _ints(gen, N, H, W, cin), _ints(gen, classes, cin, 5, 5)
            g, resid, bias = _ints(gen, N, H, W, 8), _ints(gen, N, H, W, cin), _ints(gen, 8)
            wp, wd = _packed(L, h, w, False), _packed(L, h, w, True)
            what = "%dx%dx%d, %d -> %d classes" % (N, H, W, cin, classes)
            z, _, label = _conv5(L, h, x, None, L.LOAD_PLAIN, wp, cin, 8)
            assert label == "conv5_mfma<%d,%s>" % (cin, tile), label
            assert torch.equal(z.double(), R.conv5(x.double(), R.pack5(w, False), 8)), "forward " + what
            assert not z[..., classes:].any(), "padded class channels " + what
            z, _, _ = _conv5(L, h, x, None, L.LOAD_PLAIN, wp, cin, 8, flags=L.F_BIAS, bias=bias)
            assert torch.equal(z.double(), R.conv5(x.double(), R.pack5(w, False), 8, bias=bias)), "forward + bias " + what
            dx, _, label = _conv5(L, h, g, None, L.LOAD_PLAIN, wd, 8, cin)
            assert label == "conv5_mfma<8,%s>" % tile, label
            assert torch.equal(dx.double(), R.conv5(g.double(), R.pack5(w, True), cin)), "data gradient " + what
            dx, _, _ = _conv5(L, h, g, None, L.LOAD_PLAIN, wd, 8, cin, flags=L.F_RESID, resid=resid)
            assert torch.equal(dx.double(), R.conv5(g.double(), R.pack5(w, True), cin, resid=resid)), "data gradient + resid " + what
            dw, db, label = _wgrad5(L, h, x, None, L.LOAD_PLAIN, g, cin, classes)
            assert label == "wgrad5_mfma<%d,%s>" % (cin, tile), label
            rw, rb = R.wgrad5(x.double(), g)
            assert torch.equal(dw.double(), rw[:classes]), "filter gradient " + what
            assert torch.equal(db.double(), rb[:classes]), "bias gradient " + what


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("cin", [8, 16])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_random_operands_vs_fp64(plane, cin, mode_name):
    """randn operands, N = 3, 5 classes: the forward and the filter / bias gradient under the load mode, the data gradient (its operand is
    RCV_LOAD_PLAIN, as the lowering emits it) with RCV_F_RESID and the statistics rows of RCV_STATS_BWD_ENC / _DEC.
    Measured maxima over all cases (MI355X): conv5_mfma<8,8x32> 5.9e-7, <8,16x16> 6.7e-7, <16,8x32> 7.9e-7, <16,16x16> 7.2e-7;
    wgrad5_mfma filter / bias <8,8x32> 2.8e-7 / 1.2e-7, <8,16x16> 2.3e-7 / 9.5e-8, <16,8x32> 2.2e-7 / 1.9e-7, <16,16x16> 2.1e-7 / 2.4e-7.
    (With the bias gradient summed as a chain of single adds through all pixels of a workgroup, 17x33 / 8 channels / plain gave 6.2e-7,
    over its bar, and as a chain through a tile's 16 values 16x16 / 16 channels / affine_relu gave 5.4e-7: the kernel sums it pairwise
    per tile and the reduction accumulates in float64.)"""
    L, h = _L()
    from test_gpu_blocks import close
    H, W = plane
    N, classes = 3, 5
    mode = MODES[mode_name]
    gen = torch.Generator().manual_seed(900 + 31 * H + W + cin + mode)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=gen) * scale
    x, c, w = rnd(N, H, W, cin), rnd(5, cin, scale=0.5), rnd(classes, cin, 5, 5, scale=0.1)
    g, resid, e, epi_c = rnd(N, H, W, 8), rnd(N, H, W, cin), rnd(N, H, W, cin), rnd(3, cin, scale=0.5)
    g[..., classes:] = 0
    wp, wd = _packed(L, h, w, False), _packed(L, h, w, True)
    v = R.load(mode, x, c)
    cc = None if mode == R.LOAD_PLAIN else c
    z, _, label = _conv5(L, h, x, cc, mode, wp, cin, 8)
    ref = R.conv5(v, R.pack5(w, False), 8)
    err = float((z.double() - ref).abs().max() / ref.abs().max())
    print(".%s %s forward %s: %.3e" % (label, (N, H, W), mode_name, err))
    _note(label, err)
    assert err <= 3e-6, (label, err)
    for kind in (R.STATS_BWD_ENC, R.STATS_BWD_DEC):
        dx, part, label = _conv5(L, h, g, None, L.LOAD_PLAIN, wd, 8, cin, flags=L.F_RESID, resid=resid, stats=kind, e=e, epi_c=epi_c)
        ref = R.conv5(g.double(), R.pack5(w, True), cin, resid=resid)
        err = float((dx.double() - ref).abs().max() / ref.abs().max())
        print(".%s %s data gradient stats %d: %.3e" % (label, (N, H, W), kind, err))
        _note(label, err)
        assert err <= 3e-6, (label, err)
        assert not torch.isnan(part).any(), "every partial row is written"
        close(part.double().sum(0), R.stats_rows(kind, ref, e, epi_c), "statistics rows (%d)" % kind, rtol=1e-4, floor=1.0)
    dw, db, label = _wgrad5(L, h, x, cc, mode, g, cin, classes)
    rw, rb = R.wgrad5(v, g)
    ew = float((dw.double() - rw[:classes]).abs().max() / rw[:classes].abs().max())
    eb = float((db.double() - rb[:classes]).abs().max() / rb[:classes].abs().max())
    print(".%s %s %s: filter %.3e bias %.3e" % (label, (N, H, W), mode_name, ew, eb))
    _note(label + " filter", ew)
    _note(label + " bias", eb)
    assert ew <= 5e-7 and eb <= 5e-7, (label, ew, eb)


# ------------------------------------------------------------------------------------------ beyond the first tile round
# tests/persistent_cases.py: 11 x 121 x 161 is 1056 tiles of 8x32 and 345 x 33 x 16 is 1035 tiles of 16x16, over 512 workgroups of
# conv5_kernel and 256 of wgrad5_kernel on 256 CUs: three rounds or more of `for (t = blockIdx.x; t < n; t += gridDim.x)` with a ragged
# last one -- the loop-top barrier, the reuse of xl / red, the accumulators and bsum carried across tiles.  Every case guards that on
# the real handle.
import persistent_cases as PCS      # noqa: E402
import pw_restatement as PR         # noqa: E402

EXACT = float(1 << 24)      # every integer of magnitude below 2^24 is an fp32 number: sums that stay below it are exact in any order


def _c5_case(table, what, shape, cin):
    hit = [c for c in table if (c[0], c[1]) == (what, shape) and (c[2] if what == "forward" else c[3]) == cin]
    assert len(hit) == 1, (what, shape, cin)
    return hit[0]


@pytest.mark.parametrize("cin", PCS.C5_CIN)
@pytest.mark.parametrize("plane", PCS.C5_PLANES, ids=lambda p: "x".join(map(str, p[0])))
def test_multi_round_integer_operands_are_exact(plane, cin):
    """Forward with RCV_F_BIAS, data gradient with RCV_F_RESID, filter and bias gradient, 5 classes, NaN-filled outputs and partial
    rows: bitwise the float64 restatement.  Bounds, asserted from the operands (|x|, |w|, |g|, |bias|, |resid| <= 4): an output is a
    sum of at most 25 * 16 products of at most 16 plus 4: 6404; a filter-gradient element is a sum over at most N H W = 214 291 pixels of
    products of at most 16: 3 428 656; a bias-gradient element at most 4 N H W = 857 164: all below 2^24, so every fp32 partial sum, in
    any order, is exact.
    The statistics of RCV_STATS_FWD: with |x| <= 2 and w in {-1, 0, 1} an output v is an integer with 256 v^2 < 2^24 (asserted from the
    float64 result: |v| <= 255), so a tile's fp32 sums of v and of v^2 over its 256 pixels are exact in any order; every row is
    written, and the float64 sum of the rows equals the restatement's (sum v, sum v^2) exactly."""
    L, h = _L()
    shape, tile, tiles = plane
    N, H, W = shape
    classes = 5
    gen = torch.Generator().manual_seed(70 + 97 * H + W + cin)
    x, w = _ints(gen, N, H, W, cin), _ints(gen, classes, cin, 5, 5)
    g, resid, bias = _ints(gen, N, H, W, 8), _ints(gen, N, H, W, cin), _ints(gen, 8)
    g[..., classes:] = 0
    xm, wm, gm = float(x.abs().max()), float(w.abs().max()), float(g.abs().max())
    assert 25 * cin * xm * wm + float(bias.abs().max()) < EXACT and 25 * 8 * gm * wm + float(resid.abs().max()) < EXACT
    assert N * H * W * xm * gm < EXACT and N * H * W * gm < EXACT
    fwd, dgr = _c5_case(PCS.CONV5_CASES, "forward", shape, cin), _c5_case(PCS.CONV5_CASES, "dgrad", shape, cin)
    wg = [c for c in PCS.WGRAD5_CASES if (c[0], c[1]) == (shape, cin)][0]
    PCS.assert_multi_round(PCS.conv5_record(fwd, flags=L.F_BIAS), h, fwd[4])
    PCS.assert_multi_round(PCS.conv5_record(dgr, flags=L.F_RESID), h, dgr[4])
    rows, _ = PCS.assert_multi_round(PCS.wgrad5_record(wg), h, wg[2])
    wp, wd = _packed(L, h, w, False), _packed(L, h, w, True)
    what = "%dx%dx%d, %d channels, %d tiles" % (N, H, W, cin, tiles)

    def differ(got, ref):
        return int((got.double() != ref).sum())

    z, _, label = _conv5(L, h, x, None, L.LOAD_PLAIN, wp, cin, 8, flags=L.F_BIAS, bias=bias)
    assert label == fwd[4][0], label
    ref = R.conv5(x.double(), R.pack5(w, False), 8, bias=bias)
    assert differ(z, ref) == 0, "forward + bias %s: %d elements differ" % (what, differ(z, ref))
    dx, _, label = _conv5(L, h, g, None, L.LOAD_PLAIN, wd, 8, cin, flags=L.F_RESID, resid=resid)
    assert label == dgr[4][0], label
    ref = R.conv5(g.double(), R.pack5(w, True), cin, resid=resid)
    assert differ(dx, ref) == 0, "data gradient + resid %s: %d elements differ" % (what, differ(dx, ref))
    dw, db, label = _wgrad5(L, h, x, None, L.LOAD_PLAIN, g, cin, classes)
    assert label == wg[2][0], label
    rw, rb = R.wgrad5(x.double(), g)
    assert float(rw.abs().max()) < EXACT and float(rb.abs().max()) < EXACT
    assert differ(dw, rw[:classes]) == 0, "filter gradient %s over %d rows: %d elements differ" % (what, rows, differ(dw, rw[:classes]))
    assert differ(db, rb[:classes]) == 0, "bias gradient %s over %d rows" % (what, rows)
    # the statistics rows
    xs, ws = torch.randint(-2, 3, (N, H, W, cin), generator=gen).float(), torch.randint(-1, 2, (classes, cin, 5, 5), generator=gen).float()
    ws_p = _packed(L, h, ws, False)
    ref = R.conv5(xs.double(), R.pack5(ws, False), 8)
    assert 256 * float(ref.abs().max()) ** 2 < EXACT, float(ref.abs().max())
    PCS.assert_multi_round(PCS.conv5_record(fwd, stats=L.STATS_FWD), h, fwd[4])
    z, part, _ = _conv5(L, h, xs, None, L.LOAD_PLAIN, ws_p, cin, 8, stats=L.STATS_FWD)
    assert differ(z, ref) == 0, "forward with statistics " + what
    assert tuple(part.shape) == (tiles, 2, 8) and not torch.isnan(part).any(), "every partial row is written"
    assert torch.equal(part.double().sum(0), torch.stack([ref.sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))])), "statistics rows " + what


def test_multi_round_random_operands_vs_fp64():
    """randn operands at 11 x 121 x 161, 16 channels, 5 classes (1056 tiles): the forward under RCV_LOAD_AFFINE_RELU, the data gradient
    with RCV_F_RESID and RCV_STATS_BWD_DEC, the filter and bias gradient with x under RCV_LOAD_AFFINE_RELU (the kernel reads g as it
    is).  The products per output of the convolutions do not grow with the rounds: 3e-6 of the largest float64 entry stands.  An
    accumulator of the filter gradient runs a chain of ceil(1056 / 256) * 64 = 320 products (64 pixels per wave and tile), four waves
    and 256 rows are added after it; the bar of test_random_operands_vs_fp64, 5e-7 of the largest entry, is kept: the measured errors
    leave a factor 2.2 to spare (1.5 was asked for).
    Measured (MI355X): forward 6.2e-07, data gradient 4.4e-07, filter gradient 2.2e-07, bias gradient 1.4e-07."""
    L, h = _L()
    from test_gpu_blocks import close
    fwd, dgr = PCS.CONV5_RANDOM_CASES
    wg = PCS.WGRAD5_RANDOM_CASE
    (N, H, W), cin, classes = fwd[1], fwd[2], 5
    assert dgr[1] == wg[0] == (N, H, W) and dgr[3] == wg[1] == cin
    gen = torch.Generator().manual_seed(977)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=gen) * scale
    x, c, w = rnd(N, H, W, cin), rnd(5, cin, scale=0.5), rnd(classes, cin, 5, 5, scale=0.1)
    g, resid, e, epi_c = rnd(N, H, W, 8), rnd(N, H, W, cin), rnd(N, H, W, cin), rnd(3, cin, scale=0.5)
    g[..., classes:] = 0
    wp, wd = _packed(L, h, w, False), _packed(L, h, w, True)
    v = R.load(R.LOAD_AFFINE_RELU, x, c)
    PCS.assert_multi_round(PCS.conv5_record(fwd, inmode=L.LOAD_AFFINE_RELU), h, fwd[4])
    z, _, label = _conv5(L, h, x, c, L.LOAD_AFFINE_RELU, wp, cin, 8)
    ref = R.conv5(v, R.pack5(w, False), 8)
    err = float((z.double() - ref).abs().max() / ref.abs().max())
    print(".%s multi-round forward affine_relu: %.3e" % (label, err))
    assert label == fwd[4][0] and err <= 3e-6, (label, err)
    PCS.assert_multi_round(PCS.conv5_record(dgr, flags=L.F_RESID, stats=L.STATS_BWD_DEC), h, dgr[4])
    dx, part, label = _conv5(L, h, g, None, L.LOAD_PLAIN, wd, 8, cin, flags=L.F_RESID, resid=resid, stats=R.STATS_BWD_DEC, e=e, epi_c=epi_c)
    ref = R.conv5(g.double(), R.pack5(w, True), cin, resid=resid)
    err = float((dx.double() - ref).abs().max() / ref.abs().max())
    print(".%s multi-round data gradient: %.3e" % (label, err))
    assert label == dgr[4][0] and err <= 3e-6, (label, err)
    assert part.shape[0] == dgr[4][2] and not torch.isnan(part).any(), "every partial row is written"
    close(part.double().sum(0), R.stats_rows(R.STATS_BWD_DEC, ref, e, epi_c), "multi-round statistics rows", rtol=1e-4, floor=1.0)
    rows, tiles = PCS.assert_multi_round(PCS.wgrad5_record(wg, inmode=L.LOAD_AFFINE_RELU), h, wg[2])
    dw, db, label = _wgrad5(L, h, x, c, L.LOAD_AFFINE_RELU, g, cin, classes)
    rw, rb = R.wgrad5(v, g)
    ew = float((dw.double() - rw[:classes]).abs().max() / rw[:classes].abs().max())
    eb = float((db.double() - rb[:classes]).abs().max() / rb[:classes].abs().max())
    print(".%s multi-round affine_relu, %d tiles over %d rows: filter %.3e bias %.3e" % (label, tiles, rows, ew, eb))
    assert label == wg[2][0] and ew <= 5e-7 and eb <= 5e-7, (label, ew, eb)


@pytest.mark.parametrize("classes", PCS.WGRAD5_REDUCE_CLASSES)
@pytest.mark.parametrize("nsplit", PCS.WGRAD5_REDUCE_NSPLIT)
def test_reduction_order_is_the_documented_one(nsplit, classes):
    """RCV_OP_WGRAD5_REDUCE alone on partial rows the test writes (randn, and pw_restatement.order_sensitive_rows, on which another
    order of the float64 additions gives another fp32 result), 8 and 16 input channels: bit for bit cls5_restatement.wgrad5_reduce --
    rows 0, 1, ... added in float64 in that order, rounded once; the filter part and the bias part.  NaN-filled outputs, each with a
    guard band behind it."""
    L, h = _L()
    guard = 256
    row = 25 * 8 * 16 + 8
    gen = torch.Generator().manual_seed(800 + 7 * nsplit + classes)
    for cin in (8, 16):
        for name, part in (("randn", torch.randn(nsplit, row, generator=gen)), ("order-sensitive", PR.order_sensitive_rows(gen, nsplit, row))):
            pd = part.to(DEV)
            nw = classes * cin * 25
            bufs = []
            for n in (nw, classes):
                buf = torch.full((n + guard,), float("nan"), device=DEV)
                buf[n:] = -12345.0
                bufs.append(buf)
            _run(L, h, [L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=cin, cout=classes, nsplit=nsplit, p_part=pd.data_ptr(),
                                  p_out=bufs[0].data_ptr(), p_bias=bufs[1].data_ptr())])
            assert all(bool((b[-guard:] == -12345.0).all()) for b in bufs), "a store past the tensor"
            rw, rb = R.wgrad5_reduce(part, cin, classes)
            assert torch.equal(bufs[0][:nw].cpu().view(classes, cin, 5, 5), rw), "%s rows, %d channels: filter part" % (name, cin)
            assert torch.equal(bufs[1][:classes].cpu(), rb), "%s rows, %d channels: bias part" % (name, cin)


def test_measured_maxima_are_reported():
    """Prints the largest error per kernel label over the random cases above (run after them, in file order)."""
    for label in sorted(_MAXIMA):
        print(".maximum %s: %.3e" % (label, _MAXIMA[label]))


# ------------------------------------------------------------------------------------------ whole steps against tests/golden/cls5.npz
GOLDEN = os.path.join(ROOT, "tests", "golden")
PB_W = [1, 6, 1.5, 3, 3]
CE_W = [1, 10, 30, 10, 2]
CASES = {
    "pbfcn5_s_2x48x64": lambda M: M.PB_FCN(32, 5, 5, False, 0),
    "pbfcn5_l_1x64x96": lambda M: M.PB_FCN(32, 5, 5, True, 0),
    "robo5_s_2x48x64": lambda M: M.ROBO_UNet(classSize=5),
    "v25_s_2x48x64": lambda M: M.ROBO_UNet(v2=True, classSize=5, levels=1, bellySize=2),
}


@pytest.fixture(scope="module")
def c5():
    import json
    import numpy as np
    with open(os.path.join(GOLDEN, "cls5.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "cls5.npz")), meta


def _model(tag, meta):
    import robocupvision_amd.model as M
    from conftest import sd_hash
    torch.manual_seed(12345678)
    model = CASES[tag](M)
    assert sd_hash(model.state_dict()) == meta[tag]["sd_hash_init"]
    return model.to(DEV)


def _inputs(m):
    from oracle import cpu_reference as O
    x, t = O.synthetic_batch(m["B"], m["H"], m["W"])
    return x.to(DEV), t.to(DEV)


def _check_step(tag, kats, m, pred, loss, grads):
    """The bars of tests/test_gpu_pbfcn.py / tests/test_gpu_net.py: loss 1e-3, logits close(), gradients close(rtol=1e-3, floor=1.0)
    against the reference's fp32 step or its float64 evaluation, the arg-max mask equal outside the stored near-tie pixels."""
    from test_gpu_blocks import close, _t
    from test_gpu_net import check_mask
    assert kats[tag + "/near_tie_idx"].size <= 0.01 * kats[tag + "/argmax"].size
    close(pred, _t(kats[tag + "/logits"]), tag + " logits")
    print("%s: loss %.8f vs %.8f (fp64 %.8f)" % (tag, loss, m["ce"], m["ce64"]))
    assert abs(loss - m["ce"]) <= 1e-3 * abs(m["ce"]), (loss, m["ce"])
    check_mask(torch.max(pred, 1)[1], kats[tag + "/argmax"], kats[tag + "/near_tie_idx"], tag)
    assert sorted(k for k, g in grads.items() if g is None) == sorted(m["none_grads"])
    for k, g in grads.items():
        if g is None or (k.startswith("up") and k.endswith("conv.bias")):      # zero by construction (bias ahead of BatchNorm)
            continue
        full = "%s/grad/%s" % (tag, k) in kats.files
        got = g if full else g.reshape(-1)[:64]
        refs = [_t(kats["%s/%s%s/%s" % (tag, kind, "" if full else "_head", k)]).reshape(got.shape) for kind in ("grad", "grad64")]
        try:
            close(got, refs[0], "%s grad %s" % (tag, k), rtol=1e-3, floor=1.0)
        except AssertionError:
            close(got, refs[1], "%s grad %s (float64 evaluation)" % (tag, k), rtol=1e-3, floor=1.0)
        if not full:
            gn, n32, n64 = float(g.double().norm()), m["grad_norm"][k], m["grad_norm64"][k]
            assert abs(gn - n32) <= 1e-3 * n32 + 1e-7 or abs(gn - n64) <= 1e-3 * n64 + 1e-7, (k, gn, n32, n64)


def _check_eval(tag, kats, model, x):
    from test_gpu_blocks import close, _t
    model.eval()
    with torch.no_grad():
        pe = model(x[:1])
    close(pe, _t(kats[tag + "/eval_logits0"]), tag + " eval logits", rtol=5e-3)


@pytest.mark.parametrize("tag", list(CASES))
def test_trainer_step_vs_golden(c5, tag):
    """Trainer.step with the fused optimizers -- optim.SGD for PB_FCN (trainer.py), AdamL1 for ROBO_UNet (train.py) -- then the
    eval-mode forward with the updated running statistics."""
    from robocupvision_amd.optim import SGD
    from robocupvision_amd.train import Trainer
    kats, meta = c5
    m = meta[tag]
    model = _model(tag, meta)
    x, t = _inputs(m)
    if m["adam"]:
        tr = Trainer(model, class_weights=CE_W, lr=1e-3, decay=1e-6)
    else:
        tr = Trainer(model, class_weights=PB_W, optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    pred = tr.step(x, t).detach().clone()
    plan = model._get_engine()._last[0]
    labels = plan.fwd.labels(model._get_engine().handle) + plan.bwd.labels(model._get_engine().handle)
    assert any(s.startswith("conv5_mfma") for s in labels) and any(s.startswith("wgrad5_mfma") for s in labels)
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    if m["adam"]:      # AdamL1 adds the L1 term's gradient inside its own launch; the reference's gradients carry it (train.py:52-57)
        grads = {k: g + 1e-6 * torch.sign(before[k]) for k, g in grads.items()}
    met = tr.pop_metrics()
    _check_step(tag, kats, m, pred, met["loss"] - met["reg"], grads)
    _check_eval(tag, kats, model, x)
    tr.step(x, t)           # plan reuse, optimizer state, updated statistics: the second iteration's cross entropy (bar of test_gpu_pbfcn.py)
    met = tr.pop_metrics()
    ce2 = met["loss"] - met["reg"]
    print("%s: second step %.8f vs %.8f" % (tag, ce2, m["ce_step2"]))
    assert abs(ce2 - m["ce_step2"]) <= 2e-3 * abs(m["ce_step2"]), (ce2, m["ce_step2"])


@pytest.mark.parametrize("tag", ["pbfcn5_s_2x48x64", "v25_s_2x48x64"])
def test_autograd_step_vs_golden(c5, tag):
    """The plain autograd path: model(x), the package's loss module, loss.backward()."""
    import robocupvision_amd.model as M
    kats, meta = c5
    m = meta[tag]
    model = _model(tag, meta).train()
    x, t = _inputs(m)
    crit = M.CrossEntropyLoss2d(torch.tensor(m["weights"], dtype=torch.float32)).to(DEV)
    pred = model(x)
    ce = crit(pred, t)
    loss = ce
    if m["adam"]:
        reg = 0
        for p in model.parameters():
            reg = reg + torch.sum(torch.abs(p))
        loss = ce + 1e-6 * reg
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    _check_step(tag, kats, m, pred.detach(), float(ce), grads)


@pytest.mark.parametrize("tag", ["pbfcn5_s_2x48x64", "robo5_s_2x48x64", "v25_s_2x48x64"])
def test_predict_is_the_argmax_of_the_same_build(c5, tag):
    """`predict` (RCV_OP_CLS_LABEL behind the 5x5 conv) and `Segmenter`: bit for bit torch.max(model(x), 1)[1]."""
    from robocupvision_amd.infer import Segmenter
    kats, meta = c5
    model = _model(tag, meta).eval()
    x, _ = _inputs(meta[tag])
    with torch.no_grad():
        want = torch.max(model(x), 1)[1]
    got = model.predict(x)
    assert got.dtype == torch.uint8 and torch.equal(got.long(), want)
    labels, colour = model.predict(x, colour=True)
    assert torch.equal(labels, got) and tuple(colour.shape) == tuple(got.shape) + (3,)
    assert len(torch.unique(got)) > 1, "a constant map would prove nothing"
    # Segmenter: decoded frames -> prepare_frames -> predict
    from robocupvision_amd.data import prepare_frames
    m = meta[tag]
    frames = torch.randint(0, 256, (m["B"], 2 * m["H"], 2 * m["W"], 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    labels, colour = Segmenter(model, img_size=(m["H"], m["W"]))(frames)
    with torch.no_grad():
        want = torch.max(model(prepare_frames(frames, (m["H"], m["W"]))), 1)[1]
    assert torch.equal(labels.long(), want) and tuple(colour.shape) == tuple(labels.shape) + (3,)


@pytest.mark.parametrize("cin", [8, 16])
@pytest.mark.parametrize("classes", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_class_count_through_the_engine(classes, cin):
    """A one-node graph (a 5x5 classifier on an NHWC input) in eval mode: pack, conv, bias + NCHW tail as the lowering emits them, and
    the eval-labels plan, for every class count -- against conv2d in float64 (3e-6 of the largest logit)."""
    import torch.nn.functional as F
    from robocupvision_amd.engine import Engine
    gen = torch.Generator().manual_seed(77 + classes + cin)
    conv = torch.nn.Conv2d(cin, classes, 5, padding=2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(classes, cin, 5, 5, generator=gen) * 0.1)
        conv.bias.copy_(torch.randn(classes, generator=gen))
    conv = conv.to(DEV)
    graph = {"inputs": [{"layout": "nhwc"}], "nodes": [{"op": "cls", "src": ("in", 0), "weight": conv.weight, "bias": conv.bias}]}
    eng = Engine(graph, list(conv.parameters()), [])
    x = torch.randn(2, 24, 40, cin, generator=gen)
    out = eng.forward([x.to(DEV)], False)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=2)
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 3e-6, err
    labels = eng.predict([x.to(DEV)])
    assert torch.equal(labels.long(), torch.max(out, 1)[1])
