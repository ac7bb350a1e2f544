"""Seeded operands of the exact (integer-grid) cases of tests/test_gpu_small_ops.py and of the epilogue-statistics cases of
tests/test_gpu_kernels.py, with their float64 answers (small_ops_restatement) -- numpy, and torch's float64 convolution for the
conv cases; nothing from the library, so that tests/test_small_ops.py can assert every case's preconditions without a GPU:

  * every reduction's sum of |terms| is an integer multiple of its quantum q below 2^24 q (exact in fp32 in any order);
  * removing the last pixel, or the first pixel of the second grid pass, changes EVERY entry of every reduced result (the inputs
    are forced so that those pixels carry non-zero terms in every channel)."""
import numpy as np

import small_ops_restatement as R

# pixel counts shared by the cases: under one wave, multiples of 64 under / over one workgroup (not of 256), odd
PLANES = [(1, 7, 5), (2, 8, 12), (3, 8, 24), (3, 13, 17)]
WG = 256


def big_planes(num_cus):
    """Two planes per grid cap whose pixel count exceeds one grid pass of 256-thread workgroups: a multiple of 64 and an odd one.
    reducing kernels: 4 workgroups per CU, streaming kernels: 8 (256 CUs: 2x360x368, 3x297x295 / 2x520x512, 3x417x421)."""
    out = {}
    for name, per_cu, w64, wodd in (("reducing", 4, 368, 295), ("streaming", 8, 512, 421)):
        lim = WG * per_cu * num_cus
        h64 = (lim // (2 * w64) + 1 + 7) // 8 * 8
        hodd = lim // (3 * wodd) + 1
        hodd += 1 - hodd % 2
        assert 2 * h64 * w64 > lim and (2 * h64 * w64) % 64 == 0 and 3 * hodd * wodd > lim and (3 * hodd * wodd) % 2 == 1
        out[name] = [(2, h64, w64), (3, hodd, wodd)]
    return out


def _amp(npix):
    return 1 if npix > 50000 else 2


def _forced(npix, second):
    return R.drop_masks(npix, second)


def assert_sensitive(reduce_fn, npix, second, what):
    """reduce_fn(keep) -> tuple of arrays; each removal must move every entry of every array."""
    full = reduce_fn(None)
    idx, masks = R.drop_masks(npix, second)
    for i, k in zip(idx, masks):
        for a, b in zip(full, reduce_fn(k)):
            assert np.all(np.asarray(a) != np.asarray(b)), "%s: removing pixel %d leaves %d entries unchanged" % (
                what, i, int((np.asarray(a) == np.asarray(b)).sum()))


# ------------------------------------------------------------------------------------------ classifier
CLS_FORMS = ("plain", "fused_plain", "fused_affine", "fused_affine_relu")
MODE2 = {"fused_plain": R.LOAD_PLAIN, "fused_affine": R.LOAD_AFFINE, "fused_affine_relu": R.LOAD_AFFINE_RELU}


def cls_case_list(num_cus):
    """(cin, classes, plane, form, first pixel of the second grid pass) of every exact classifier case: every form and class count
    on the four small planes; beyond one grid pass of the reducing kernels BOTH planes (the multiple of 64: the wave-shuffle store
    path of cls_bwd_kernel; the odd one: its plain path) for every class count in the plain and in a fused form (the skip load mode,
    a run-time argument, rotates with the class count); the 16-channel backward for 1, 5, 8 classes."""
    cap = WG * 4 * num_cus
    big = big_planes(num_cus)["reducing"]
    out = [(8, nC, pl, form, cap) for nC in range(1, 9) for pl in PLANES for form in CLS_FORMS]
    out += [(8, nC, pl, form, cap) for nC in range(1, 9) for pl in big for form in ("plain", CLS_FORMS[1 + nC % 3])]
    out += [(16, nC, pl, "plain", cap) for nC in (1, 5, 8) for pl in PLANES + [big[nC % 2]]]
    return out


def pool_cases(cus):
    """(N, H, W, C): W*C/4 a multiple of 64 (rows kernel where C/4 is a power of two) and not; one plane per backward kernel just
    beyond one grid pass (N = 2, C = 8: 2 * (H / 2) * (W / 2) * 2 work items); the cap in work items."""
    small = [(2, 8, 32, 8), (2, 6, 16, 16), (1, 4, 8, 64), (3, 10, 64, 8), (2, 6, 24, 8), (2, 4, 6, 16), (1, 6, 10, 64), (3, 4, 2, 8)]
    cap = WG * 4 * cus
    return small, [(2, 2 * (cap // 512 + 1), 256, 8), (2, 2 * (cap // 500 + 1), 250, 8)], cap


BWD_STATS_SLICES = [(8, 0, 8), (16, 8, 8), (32, 16, 16)]        # (Csrc, coff, C)


def build_cls(cin, nC, plane, form, second, seed=0):
    """Operands of RCV_OP_CLS_FWD / _BWD on the integer grid.  `second`: index of the first pixel of the second grid pass."""
    N, H, W = plane
    npix = N * H * W
    rng = np.random.default_rng(7000 + 97 * seed + 13 * nC + npix + cin)
    a = _amp(npix)
    c = dict(cin=cin, nC=nC, plane=plane, form=form, npix=npix, second=second)
    c["t"] = R.grid(rng, (N, H, W, cin), a)
    c["tc"] = R.grid_consts(rng, cin)
    c["w"] = R.grid(rng, (nC, cin), 2)
    c["b"] = R.grid(rng, (nC,), 2)
    c["dl"] = R.grid(rng, (N, nC, H, W), a)
    col = c["w"].sum(0)
    c["w"][0, col == 0] += np.where(c["w"][0, col == 0] < 2, 1, -1)          # d_up of an all-ones gradient: non-zero in every channel
    idx, _ = _forced(npix, second)
    tf, dlf = c["t"].reshape(npix, cin), c["dl"].transpose(0, 2, 3, 1).reshape(npix, nC).copy()
    tf[idx] = 2 * np.sign(c["tc"][0])                                         # mask on, t - mean != 0
    dlf[idx] = 1.0
    c["dl"] = np.ascontiguousarray(dlf.reshape(N, H, W, nC).transpose(0, 3, 1, 2))
    if form == "plain":
        c["up"] = R.grid(rng, (N, H, W, cin), a)
        c["up"].reshape(npix, cin)[idx] = 1.0
    else:
        c["mode2"] = MODE2[form]
        c["r"] = R.grid(rng, (N, H, W, cin), a)
        c["rc"] = R.grid_consts(rng, cin)
        c["r"].reshape(npix, cin)[idx] = 1.0 if form == "fused_plain" else 2 * np.sign(c["rc"][0])
    return c


def cls_up(c):
    return R._f(c["up"]) if c["form"] == "plain" else R.fused_up(c["t"], c["tc"], c["r"], c["rc"], c["mode2"])


def cls_reduced(c, keep=None):
    """dW, db and the BWD_DEC statistics of d_up against t."""
    up = cls_up(c)
    d_up, dW, db = R.cls_backward(up, c["dl"], c["w"], keep)
    return dW, db, R.stats(R.STATS_BWD_DEC, d_up, c["t"], c["tc"], keep)


def check_cls(c):
    up = cls_up(c)
    d_up = R.cls_backward(up, c["dl"], c["w"])[0]
    dWa, dba = R.cls_backward_abs(up, c["dl"])
    R.assert_exact(dWa, 1.0, "cls dW")
    R.assert_exact(dba, 1.0, "cls db")
    R.assert_exact(R.stats_abs(R.STATS_BWD_DEC, d_up, c["t"], c["tc"]), 1.0, "cls statistics")
    R.assert_exact(np.abs(R._f(c["w"])).sum(1) * np.abs(up).max() + np.abs(R._f(c["b"])), 1.0, "cls logits")
    z = R._f(c["t"]) * R._f(c["tc"])[0] + R._f(c["tc"])[1]
    assert (z == 0).any() and (z < 0).any(), "the mask must meet pixels at and below zero"
    assert_sensitive(lambda k: cls_reduced(c, k), c["npix"], c["second"], "cls %s" % c["form"])


# ------------------------------------------------------------------------------------------ max-pool
def pool_rows_kernel(W, C):
    """The launcher's choice of pool_bwd_rows_kernel: C/4 a power of two below 64 and W * C/4 a multiple of 64."""
    C4 = C // 4
    return (C4 & (C4 - 1)) == 0 and C4 < 64 and (W * C4) % 64 == 0


def build_pool(N, H, W, C, affine, resid, second_item=0, seed=0):
    """RCV_OP_POOL_FWD / _BWD: r with few distinct values (most windows hold ties), scales of both signs.  second_item: the first
    work item (output pixel x channel quad) of the second grid pass."""
    rng = np.random.default_rng(8000 + seed + H * W + C + 2 * affine + resid)
    npix = N * H * W
    a = _amp(npix)
    c = dict(N=N, H=H, W=W, C=C, affine=affine, resid=resid, npix=npix)
    c["r"] = R.grid(rng, (N, H, W, C), 2)
    c["dp"] = R.grid(rng, (N, H // 2, W // 2, C), a)
    c["c"] = R.grid_consts(rng, C, scales=(0.5, -0.5, 2.0, -2.0))
    if not affine:
        c["c"][:] = 0
        c["c"][0] = 1
    c["res"] = R.grid(rng, (N, H, W, C), a) if resid else None
    # the two pixels of the sensitivity check: strict maxima of their windows in every channel, with a non-zero gradient
    C4, Ho, Wo = C // 4, H // 2, W // 2
    if pool_rows_kernel(W, C):      # pool_bwd_rows_kernel: item = (output row, 16-byte piece of the input row): column piece / C4 of input row 2 oy
        orow, col = second_item // (W * C4), (second_item % (W * C4)) // C4
        second = (orow * 2) * W + col if 0 < second_item < N * Ho * W * C4 else 0
    else:                           # pool_bwd_kernel: item = (output pixel, channel quad): the window's first pixel
        opix = second_item // C4
        n2, oy2, ox2 = opix // (Ho * Wo), (opix // Wo) % Ho, opix % Wo
        second = (n2 * H + 2 * oy2) * W + 2 * ox2 if 0 < opix < N * Ho * Wo else 0
    c["second"] = second
    idx, _ = _forced(npix, second)
    for i in idx:
        n, y, x = i // (H * W), (i // W) % H, i % W
        c["r"][n, y, x] = 5 * np.sign(c["c"][0])
        c["dp"][n, y // 2, x // 2] = 1.0
        if resid:
            c["res"][n, y, x] = 1.0
    return c


def pool_mode(c):
    return R.LOAD_AFFINE if c["affine"] else R.LOAD_PLAIN


def pool_dy(c):
    return R.pool_backward(c["dp"], c["r"], c["c"], pool_mode(c), c["res"])


def pool_ec(c):
    """(unused, unused, centre) of the statistics: the batch mean (row 2) under LOAD_AFFINE, 0 under LOAD_PLAIN."""
    ec = np.zeros((3, c["C"]))
    ec[2] = c["c"][2] if c["affine"] else 0.0
    return ec


def check_pool(c):
    dy = pool_dy(c)
    R.assert_exact(R.stats_abs(R.STATS_BWD_ENC, dy, c["r"], pool_ec(c)), 1.0, "pool statistics")
    v = R._windows(R.load(c["r"], c["c"], pool_mode(c)))
    ties = (np.sort(v, 3)[:, :, :, -1] == np.sort(v, 3)[:, :, :, -2]).mean()
    assert ties > 0.1, "too few tied windows (%.2f)" % ties
    assert_sensitive(lambda k: (R.stats(R.STATS_BWD_ENC, dy, c["r"], pool_ec(c), k),), c["npix"], c["second"], "pool")


# ------------------------------------------------------------------------------------------ BWD_STATS
def build_bwd_stats(plane, Csrc, coff, C, second_item=0, seed=0):
    N, H, W = plane
    npix = N * H * W
    rng = np.random.default_rng(9000 + seed + npix + Csrc + coff)
    a = _amp(npix)
    c = dict(plane=plane, Csrc=Csrc, coff=coff, C=C, npix=npix, second=second_item // (C // 4))
    c["g"] = R.grid(rng, (N, H, W, Csrc), a)
    c["e"] = R.grid(rng, (N, H, W, C), a)
    c["ec"] = R.grid_consts(rng, C, rows=3)
    idx, _ = _forced(npix, c["second"])
    c["g"].reshape(npix, Csrc)[idx] = 1.0
    c["e"].reshape(npix, C)[idx] = 2 * np.sign(c["ec"][0])
    return c


def bwd_stats_out(c):
    return R._f(c["g"])[..., c["coff"]:c["coff"] + c["C"]]


def check_bwd_stats(c):
    out = bwd_stats_out(c)
    for kind in (R.STATS_BWD_ENC, R.STATS_BWD_DEC):
        R.assert_exact(R.stats_abs(kind, out, c["e"], c["ec"]), 1.0, "bwd_stats")
        assert_sensitive(lambda k: (R.stats(kind, out, c["e"], c["ec"], k),), c["npix"], c["second"], "bwd_stats")
    z = R._f(c["e"]) * R._f(c["ec"])[0] + R._f(c["ec"])[1]
    assert (z == 0).any() and (z < 0).any()


# ------------------------------------------------------------------------------------------ conv / transposed-conv epilogue statistics
# the ragged and tiny members of CONV_SHAPES / TCONV_SHAPES of tests/test_gpu_kernels.py, plus one per family with more than one tile
# row per workgroup; (N, H, W, Cin, Cout, stride)
CONV_STATS_SHAPES = [(3, 5, 7, 64, 64, 1), (2, 37, 53, 32, 64, 1), (5, 9, 11, 128, 128, 1), (4, 15, 20, 64, 128, 1), (4, 15, 20, 128, 64, 1),
                     (2, 30, 40, 128, 128, 1), (4, 30, 40, 64, 32, 1), (4, 30, 40, 32, 64, 2), (4, 30, 40, 32, 32, 1), (1, 33, 47, 16, 16, 1),
                     (2, 47, 33, 8, 16, 2), (2, 48, 64, 16, 32, 2), (1, 29, 41, 64, 128, 2), (4, 60, 80, 16, 16, 1), (2, 120, 160, 8, 16, 2)]
TCONV_STATS_SHAPES = [(3, 7, 9, 128, 64), (1, 33, 21, 64, 32), (2, 24, 32, 32, 16), (4, 8, 10, 64, 64), (2, 20, 28, 16, 16), (1, 5, 6, 128, 128),
                      (2, 15, 20, 128, 64), (1, 27, 35, 16, 8)]
# NCHW-image first layers and the tiny dilated planes (the latter leave conv_small when statistics are requested)
IMAGE_STATS_SHAPES = [(3, 37, 53, 4, 16, 1, 1), (1, 33, 47, 3, 16, 2, 1), (2, 40, 56, 3, 8, 1, 2), (2, 24, 40, 2, 32, 1, 2), (2, 48, 64, 3, 8, 1, 1)]
TINY_STATS_SHAPES = [(2, 15, 20, 32, 64, 1, 2), (1, 7, 9, 128, 64, 1, 1), (3, 9, 11, 16, 48, 2, 1), (2, 5, 3, 20, 36, 1, 2)]
# dilation 2 on NHWC operands (LabelProp conv1..3, PB_FCN conv4..8, ConvPool.conv1): conv_dma, conv_mfma and the run-time-pitch branch
# of convs_mfma, ragged planes, several tiles per workgroup, stride 2, and a plane whose off-centre taps all lie in the padding
DILATED_STATS_SHAPES = [(2, 37, 53, 64, 64, 1, 2), (2, 30, 40, 64, 32, 1, 2), (2, 33, 47, 16, 16, 1, 2), (2, 33, 47, 32, 16, 1, 2),
                        (3, 5, 7, 128, 64, 1, 2), (2, 33, 47, 16, 32, 2, 2), (1, 2, 2, 32, 32, 1, 2)]
# (statistics kind, flags): F_BIAS = 1, F_RELU = 2, F_RESID = 4.  Sensitivity: every variant of the convs (the input under the centre
# tap makes the two removed pixels non-zero in every channel); of the transposed convs, whose odd output pixels no centre tap reaches,
# the variants with a residual (which does the same there).
STATS_VARIANTS = [(R.STATS_FWD, 3), (R.STATS_FWD, 0), (R.STATS_FWD, 5), (R.STATS_BWD_ENC, 4), (R.STATS_BWD_DEC, 4)]


# one randn case per kernel family (label prefix the case must reach): (family, shape, filter layout, label prefix)
CONV_RANDN_CASES = [("conv", (4, 15, 20, 64, 64, 1), 0, "conv_dma"), ("conv", (4, 30, 40, 64, 32, 1), 0, "conv_mfma"),
                    ("conv", (2, 37, 53, 32, 64, 1), 2, "conv_wino"), ("conv", (4, 15, 20, 64, 64, 1), 3, "conv_bf3"),
                    ("conv", (4, 30, 40, 32, 64, 2), 5, "conv2_bf3"), ("conv", (4, 30, 40, 32, 32, 1), 3, "convn_bf3"),
                    ("conv", (4, 30, 40, 32, 32, 1), 0, "convs_mfma"), ("image", (2, 48, 64, 3, 8, 1, 1), 0, "conv_first"),
                    ("tconv", (2, 15, 20, 128, 64), 0, "tconva_dma"), ("tconv", (2, 24, 32, 32, 16), 1, "tconvms_mfma"),
                    ("tconv", (2, 24, 32, 32, 16), 4, "tconvn_bf3")]


def build_conv_stats(shape, transposed=False, nchw=False, seed=0, randn=False):
    """Operands shared by the four statistics variants of one shape: x (LOAD_AFFINE constants c, or the NCHW image), sparse filter,
    bias, residual, e and its (c0, c1, mean)."""
    if transposed:
        N, H, W, Cin, Cout = shape
        s, d, Ho, Wo = 2, 1, 2 * H, 2 * W
    else:
        N, H, W, Cin, Cout, s = shape[:6]
        d = shape[6] if len(shape) > 6 else 1
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    rng = np.random.default_rng(11000 + seed + H * W + Cin + 3 * Cout)
    c = dict(shape=shape, transposed=transposed, nchw=nchw, N=N, H=H, W=W, Cin=Cin, Cout=Cout, s=s, d=d, Ho=Ho, Wo=Wo)
    c["x"] = R.grid(rng, (N, Cin, H, W) if nchw else (N, H, W, Cin), 2)
    c["c"] = R.grid_consts(rng, Cin)
    c["w"] = R.sparse_filter(rng, Cout, Cin, transposed=transposed)
    c["bias"] = R.grid(rng, (Cout,), 2)
    c["res"] = R.grid(rng, (N, Ho, Wo, Cout), 2)
    c["e"] = R.grid(rng, (N, Ho, Wo, Cout), 2)
    c["ec"] = R.grid_consts(rng, Cout, rows=3)
    if randn:       # random values: the rounding-order case of every statistics kind
        f = np.float32
        c["x"], c["c"] = rng.standard_normal(c["x"].shape).astype(f), (rng.standard_normal((5, Cin)) * 0.5).astype(f)
        c["w"] = (rng.standard_normal(c["w"].shape) * 0.1).astype(f)
        c["bias"], c["res"], c["e"] = (rng.standard_normal(c[k].shape).astype(f) for k in ("bias", "res", "e"))
        c["ec"] = (rng.standard_normal((3, Cout)) * 0.5).astype(f)
        for _ in range(3):      # keep the BWD_DEC mask away from zero, where an fp32 fma and float64 may decide differently
            near = np.abs(R._f(c["e"]) * R._f(c["ec"])[0] + R._f(c["ec"])[1]) < 1e-3
            c["e"][near] += f(0.0625)
        assert not (np.abs(R._f(c["e"]) * R._f(c["ec"])[0] + R._f(c["ec"])[1]) < 1e-4).any()
    c["npix"] = N * Ho * Wo
    if not randn and not transposed:
        # the two pixels of the sensitivity check reach every output channel without a residual: the input pixel under the centre tap
        # reads 3 after the load transform in every channel, the eight other tapped pixels read 0 (every output channel has one centre
        # tap with a positive weight w: the convolution gives 3 w there, 3 w + bias >= 1 with the bias)
        for i in R.drop_masks(c["npix"], 0)[0]:
            n, oy, ox = i // (Ho * Wo), (i // Wo) % Ho, i % Wo
            for ky in (-1, 0, 1):
                for kx in (-1, 0, 1):
                    iy, ix = oy * s + ky * d, ox * s + kx * d
                    if 0 <= iy < H and 0 <= ix < W:
                        X = 3.0 if ky == 0 and kx == 0 else 0.0
                        if nchw:
                            c["x"][n, :, iy, ix] = X
                        else:
                            c["x"][n, iy, ix] = (X - c["c"][1]) / c["c"][0]
    import torch
    import torch.nn.functional as F
    x = R._f(c["x"]) if nchw else R.load(c["x"], c["c"], R.LOAD_AFFINE).transpose(0, 3, 1, 2)
    xt, wt = torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(R._f(c["w"]))
    if transposed:
        y = F.conv_transpose2d(xt, wt, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(xt, wt, stride=s, padding=d, dilation=d)
    c["y"] = y.permute(0, 2, 3, 1).numpy()                 # the float64 convolution, ahead of bias / ReLU / residual
    # the two pixels of the sensitivity check: residual such that conv + residual = 3, mask on, e - mean != 0
    if randn:
        return c
    idx, _ = R.drop_masks(c["npix"], 0)
    c["res"].reshape(c["npix"], Cout)[idx] = (3.0 - c["y"].reshape(c["npix"], Cout)[idx]).astype(np.float32)
    c["e"].reshape(c["npix"], Cout)[idx] = 2 * np.sign(c["ec"][0])
    return c


def conv_stats_reference(c, kind, flags):
    """-> (stored output [N,Ho,Wo,Cout], statistics [2][Cout], sum of |terms| [2][Cout]) in float64 (torch's float64 convolution)."""
    v = c["y"]
    if flags & 1:
        v = v + R._f(c["bias"])
    if flags & 2:
        v = np.maximum(v, 0.0)
    if flags & 4:
        v = v + R._f(c["res"])
    return v, R.stats(kind, v, c["e"], c["ec"]), R.stats_abs(kind, v, c["e"], c["ec"])


def check_conv_stats(c):
    q4 = R.winograd_filter(c["w"].transpose(1, 0, 2, 3) if c["transposed"] else c["w"]) * 4
    assert np.all(q4 == np.round(q4)), "Winograd-transformed filter x 4 must be integral"
    w = c["w"].transpose(1, 0, 2, 3) if c["transposed"] else c["w"]
    assert int((w.reshape(w.shape[0], -1) != 0).sum(1).max()) <= 4
    for kind, flags in STATS_VARIANTS:
        v, _, sabs = conv_stats_reference(c, kind, flags)
        R.assert_exact(sabs, 1.0, "conv statistics kind %d" % kind)
        assert float(np.abs(v).max()) < 2.0 ** 20
        if flags & 4 or not c["transposed"]:
            assert_sensitive(lambda k: (R.stats(kind, v, c["e"], c["ec"], k),), c["npix"], 0, "conv statistics kind %d" % kind)
    z = R._f(c["e"]) * R._f(c["ec"])[0] + R._f(c["ec"])[1]
    assert (z == 0).any() and (z < 0).any()
