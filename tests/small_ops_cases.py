"""Seeded operands of the exact (integer-grid) cases of tests/test_gpu_small_ops.py and of the epilogue-statistics cases of
tests/test_gpu_kernels.py, with their float64 answers (small_ops_restatement) -- numpy, and torch's float64 convolution for the
conv cases; nothing from the library, so that tests/test_small_ops.py can assert every case's preconditions without a GPU:

  * every reduction's sum of |terms| is an integer multiple of its quantum q below 2^24 q (exact in fp32 in any order);
  * removing the last pixel, or the first pixel of the second grid pass, changes EVERY entry of every reduced result (the inputs
    are forced so that those pixels carry non-zero terms in every channel).

Further down: the seeded Adam + L1 cases with an fp32 emulation of the kernel's expression order and its wrong variants, the
hand-made partial filters of the reduction tests (layout of include/rcv.h, rcv_reduce_job) with the kernel's order of additions
restated in fp32, and the planes and labels of the confusion tests."""
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


STATS_FAMILIES = dict(conv=CONV_STATS_SHAPES, tconv=TCONV_STATS_SHAPES, image=IMAGE_STATS_SHAPES, tiny=TINY_STATS_SHAPES,
                      dilated=DILATED_STATS_SHAPES)

# One shape per persistent kernel family on which a workgroup loops over three tiles or more, the last round ragged (conv_first: two
# rounds): the sums carried in registers across the tiles of a workgroup.  (family of build_conv_stats, shape, filter layout,
# (label, workgroups, tiles) as the planner answers for 256 CUs -- pinned by tests/test_plan_census.py)
MULTI_ROUND_STATS_CASES = [
    ("conv", (65, 64, 80, 8, 8, 1), 0, ("convs_mfma<1,5,8>", 347, 1040)),
    ("conv", (13, 96, 128, 8, 8, 1), 3, ("convn_bf3<8,1,5>", 256, 520)),
    ("tconv", (65, 64, 80, 16, 8), 1, ("tconvms_mfma<2,5,16>", 347, 1040)),
    ("tconv", (9, 96, 128, 32, 16), 4, ("tconvn_bf3<32,4,3>", 256, 576)),
    ("image", (73, 100, 140, 3, 8, 1, 1), 0, ("conv_first<1>", 1024, 1533)),
]
# the randn case beside them (532 tiles over 256 workgroups): appended to CONV_RANDN_CASES
MULTI_ROUND_RANDN_CASE = ("conv", (19, 64, 80, 32, 32, 1), 3, "convn_bf3")
MULTI_ROUND_RANDN_PIN = ("convn_bf3<32,2,3>", 256, 532)
CONV_RANDN_CASES = CONV_RANDN_CASES + [MULTI_ROUND_RANDN_CASE]


def multi_round_stats_variants(case):
    """conv_first takes no residual and no backward statistics (the other variants of an image shape run on convs_mfma)."""
    if case[3][0].startswith("conv_first"):
        return [(R.STATS_FWD, 3), (R.STATS_FWD, 0)]
    return STATS_VARIANTS


def randn_variants(prefix):
    """(statistics kind, flags) of a randn case on the kernel family `prefix`."""
    if prefix == "conv_first":          # the first-layer kernel takes no residual and no backward statistics
        return [(R.STATS_FWD, 3), (R.STATS_FWD, 0)]
    return [(R.STATS_FWD, 3), (R.STATS_BWD_ENC, 4), (R.STATS_BWD_DEC, 4)]


def conv_stats_dims(shape, transposed=False, nchw=False):
    """The dimensions of a statistics case, without its operands."""
    if transposed:
        N, H, W, Cin, Cout = shape
        s, d, Ho, Wo = 2, 1, 2 * H, 2 * W
    else:
        N, H, W, Cin, Cout, s = shape[:6]
        d = shape[6] if len(shape) > 6 else 1
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    return dict(shape=shape, transposed=transposed, nchw=nchw, N=N, H=H, W=W, Cin=Cin, Cout=Cout, s=s, d=d, Ho=Ho, Wo=Wo)


def build_conv_stats(shape, transposed=False, nchw=False, seed=0, randn=False):
    """Operands shared by the four statistics variants of one shape: x (LOAD_AFFINE constants c, or the NCHW image), sparse filter,
    bias, residual, e and its (c0, c1, mean)."""
    c = conv_stats_dims(shape, transposed, nchw)
    N, H, W, Cin, Cout, s, d, Ho, Wo = (c[k] for k in ("N", "H", "W", "Cin", "Cout", "s", "d", "Ho", "Wo"))
    rng = np.random.default_rng(11000 + seed + H * W + Cin + 3 * Cout)
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


def multi_round_row_pixels(case):
    """Upper bound of the output pixels behind ONE partial row of a multi-round case: the tile rounds of a workgroup x the pixel slots
    of its tile (convs_mfma<WM,WN,CK> / convn_bf3<CK,WM,WN>: 64 WN, four output pixels per slot in the merged transposed forms;
    conv_first: 16 x 64).  From the case's pin, i.e. for 256 CUs: on fewer CUs a workgroup runs more rounds and the bound of
    check_multi_round_stats would have to be taken again (on more CUs it only gets easier)."""
    label, grid, tiles = case[3]
    name, args = label.rstrip(">").split("<")
    args = [int(a) for a in args.split(",")]
    slots = 16 * 64 if name == "conv_first" else 64 * (args[2] if name.endswith("n_bf3") else args[1]) * (4 if name.startswith("tconv") else 1)
    return -(-tiles // grid) * slots


def check_multi_round_stats(c, case):
    """The preconditions of an exact case whose plane is too large for one fp32 sum: every PARTIAL ROW is exact -- every term an
    integer, the largest |term| x the pixels behind a row below 2^24 -- and the rows are added in float64; every variant stays
    sensitive to the last and to the middle pixel; the RCV_STATS_BWD_DEC mask meets pixels at and below zero (check_conv_stats)."""
    npx = multi_round_row_pixels(case)
    z = R._f(c["e"]) * R._f(c["ec"])[0] + R._f(c["ec"])[1]
    assert (z == 0).any() and (z < 0).any() and (z > 0).any()
    for kind, flags in multi_round_stats_variants(case):
        v, ref, sabs = conv_stats_reference(c, kind, flags)
        assert np.all(v == np.round(v)) and np.all(sabs == np.round(sabs)) and float(sabs.max()) < 2.0 ** 53
        dev = np.abs(R._f(c["e"]) - R._f(c["ec"])[2])
        assert np.all(dev == np.round(dev))
        worst = max(float((v * v).max()), float((np.abs(v) * dev).max()), float(np.abs(v).max()))
        assert worst * npx < 2.0 ** 24, "largest term %.0f x %d pixels per partial row reaches 2^24" % (worst, npx)
        if flags & 4 or not c["transposed"]:
            assert_sensitive(lambda k: (R.stats(kind, v, c["e"], c["ec"], k),), c["npix"], 0, "conv statistics kind %d" % kind)


# ------------------------------------------------------------------------------------------ Adam + L1
ADAM_HYPER = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-8, decay=1e-3)
ADAM_T = (1, 2, 10, 1000, 100000)
ADAM_GS = (1.0, 1.0 / 8, 1.0 / 3)
f32 = np.float32


def adam_big_n(num_cus):
    """An element count beyond one grid pass of adam_l1_kernel (2 workgroups per CU x 256 threads x 4 elements), with a scalar tail:
    the vector loop makes a second pass in several workgroups and n % 4 == 3."""
    return 2 * num_cus * WG * 4 + 5003


def adam_cases(num_cus):
    """(n, t, grad_scale): every n, every t, every grad_scale with the large n; not the full product."""
    big = adam_big_n(num_cus)
    assert big % 4 == 3 and big // 4 > 2 * num_cus * WG
    g1, g8, g3 = ADAM_GS
    return [(1, 1, g1), (3, 2, g8), (4, 10, g3), (5, 1000, g1), (255, 100000, g8), (1027, 1, g3), (1027, 1000, g1), (100003, 2, g1),
            (100003, 10, g8), (100003, 100000, g3), (big, 1, g1), (big, 1000, g8), (big, 100000, g3)]


def _logu(rng, n, lo, hi):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def build_adam(n, t, gs):
    """fp32 operands spanning what training produces: |g| log-uniform in 1e-10..1 with random sign and exact zeros (i % 11 == 3),
    p over 1e-6..1 with exact +0 (i % 13 == 5) and -0 (i % 13 == 6), m and v of the spread of g and g^2 (zero at t = 1, and where
    i % 22 == 3: there g = m = v = 0), lr_elem in stretches of 7 (one stretch in five 0, two lr, two 10 lr), a prune mask over a
    quarter of the elements."""
    rng = np.random.default_rng(31000 + n % 9973 + 17 * t + int(1000 * gs))
    i = np.arange(n)
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    g = _logu(rng, n, 1e-10, 1.0) * sgn()
    p = _logu(rng, n, 1e-6, 1.0) * sgn()
    mag = _logu(rng, n, 1e-10, 1.0)
    m = mag * rng.uniform(0.1, 1.0, n) * sgn()
    v = mag * mag * rng.uniform(0.5, 2.0, n)
    g[i % 11 == 3] = 0.0
    p[i % 13 == 5] = 0.0
    p[i % 13 == 6] = -0.0
    if t == 1:
        m[:], v[:] = 0.0, 0.0
    m[i % 22 == 3], v[i % 22 == 3] = 0.0, 0.0
    lr = f32(ADAM_HYPER["lr"])
    lre = np.array([0.0, lr, lr, 10 * lr, 10 * lr], f32)[((i // 7) + 1) % 5]
    prune = (rng.random(n) < 0.25).astype(np.uint8)
    c = dict(n=n, t=t, gs=f32(gs), p=p.astype(f32), g=g.astype(f32), m=m.astype(f32), v=v.astype(f32), lr_elem=lre, prune=prune)
    c.update({k: f32(x) for k, x in ADAM_HYPER.items()})
    return c


ADAM_FORMS = ("plain", "lr_elem", "lr_elem+prune")


def adam_form(c, form):
    """(lr_elem, prune) of the three record forms."""
    return (None if form == "plain" else c["lr_elem"]), (c["prune"] if form.endswith("prune") else None)


def adam_reference(c, form, decay=None):
    lre, pr = adam_form(c, form)
    return R.adam_l1_step(c["p"], c["g"], c["m"], c["v"], c["t"], c["lr"], c["b1"], c["b2"], c["eps"], c["decay"] if decay is None else decay,
                          c["gs"], lre, pr)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64 (the sum is rounded twice: at 53 bits, then at 24)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


# the wrong kernels tests/test_small_ops.py shows to leave the bound: name -> the share of the live elements (lr_elem != 0, form "lr_elem+prune") that it must put outside TWICE the bound in at least one
# case of n >= 1027: half of the largest share test_small_ops.py prints
ADAM_MUTANTS = {"eps_before_bc2": 0.36,       # eps added before the division by bc2_sqrt
                "eps_inside_sqrt": 0.44,      # sqrt(v' + eps)
                "bc_t_minus_1": 0.49,         # bias corrections of step t - 1
                "gs_on_decay": 0.31,          # (g + decay sign(p)) * grad_scale
                "l1_on_pruned": 0.11,         # a pruned element keeps gr = decay sign(p)
                "sign0_is_1": 0.06,           # sign(+-0) = 1
                "v_with_gr": 0.36}            # v' = b2 v + (1 - b2) gr


def adam_emulate(c, form, contract=0, variant=None):
    """adam_l1_kernel's expression order in fp32 numpy -> (p', m', v').  contract: 0 = every product rounded (but the kernel's own
    fmaf), 1 / 2 = the two ways a compiler contracts a b + c d into an fma, and p - step r.  variant: one of ADAM_MUTANTS."""
    p, g, m, v = c["p"], c["g"], c["m"], c["v"]
    lr, b1, b2, eps, decay, gs = (c[k] for k in ("lr", "b1", "b2", "eps", "decay", "gs"))
    lre, pr = adam_form(c, form)
    lre = np.full(c["n"], lr, f32) if lre is None else lre
    t = c["t"] - 1 if variant == "bc_t_minus_1" else c["t"]
    with np.errstate(all="ignore"):
        bc1, bc2s = f32(1.0 - np.float64(b1) ** t), f32(np.sqrt(1.0 - np.float64(b2) ** t))
        sg = np.sign(p).astype(f32)
        if variant == "sign0_is_1":
            sg = np.where(p == 0, f32(1), sg)
        gr = _fma(decay, sg, g) * gs if variant == "gs_on_decay" else _fma(decay, sg, g * gs)
        if pr is not None:
            gr = np.where(pr != 0, decay * sg if variant == "l1_on_pruned" else f32(0), gr)
        o1, o2 = f32(1) - b1, f32(1) - b2
        s1 = o2 * gr
        s2 = s1 if variant == "v_with_gr" else s1 * gr
        if contract == 0:
            m1, v1 = b1 * m + o1 * gr, b2 * v + s2
        elif contract == 1:
            m1, v1 = _fma(b1, m, o1 * gr), _fma(b2, v, s2)
        else:
            m1, v1 = _fma(o1, gr, b1 * m), (b2 * v + s2 if variant == "v_with_gr" else _fma(s1, gr, b2 * v))
        if variant == "eps_before_bc2":
            den = (np.sqrt(v1) + eps) / bc2s
        elif variant == "eps_inside_sqrt":
            den = np.sqrt(v1 + eps) / bc2s
        else:
            den = np.sqrt(v1) / bc2s + eps
        step, r = lre / bc1, m1 / den
        p1 = p - step * r if contract == 0 else _fma(-step, r, p)
    live = lre != 0
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    return np.where(live, p1, p), np.where(live, m1, m), np.where(live, v1, v)


def adam_ratios(got, ref, bound):
    """Largest error / bound of each of (p, m, v), and the elements outside `factor` x the bound."""
    out = []
    for a, r, b in zip(got, ref, bound):
        err = np.abs(np.asarray(a, np.float64) - r)
        out.append(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0))
    return out


def adam_metrics_inputs(n, seed=0):
    """p on the grid k / 8, |k| <= 16 (sum|p| exact in double and in fp32 partial sums in any order), a third of the elements with
    lr_elem == 0, a quarter pruned."""
    rng = np.random.default_rng(32000 + seed + n % 9973)
    p = (rng.integers(-16, 17, n) / 8.0).astype(f32)
    lre = np.where(np.arange(n) % 3 == 1, f32(0), f32(ADAM_HYPER["lr"])).astype(f32)
    return dict(n=n, p=p, g=rng.standard_normal(n).astype(f32), m=(rng.standard_normal(n) * 0.1).astype(f32),
                v=(rng.random(n) * 0.01).astype(f32), lr_elem=lre, prune=(np.arange(n) % 4 == 2).astype(np.uint8))


# ------------------------------------------------------------------------------------------ filter-gradient reductions
REDUCE_NSPLIT = (1, 2, 15, 16, 17, 32, 48, 49, 63, 64, 65, 112, 113, 129, 200)
REDUCE_SHAPES = ((8, 3), (8, 4), (16, 8), (5, 16))         # (CB, CA): every nsplit, with and without the bias row
REDUCE_WIDE = ((64, 32), (1, 49, 65, 200))                  # with the bias row


def reduce_pads(CB, CA):
    """include/rcv.h (rcv_reduce_job): CAP = CA <= 4 ? 4 : round16(CA), CBP = round16(CB)."""
    return (CB + 15) // 16 * 16, (4 if CA <= 4 else (CA + 15) // 16 * 16)


def reduce_blocks(CB, CA, with_bias):
    CBP, CAP = reduce_pads(CB, CA)
    return (9 * CBP * CAP + (CBP if with_bias else 0) + 63) // 64


def build_reduce(nsplit, CB, CA, kind, seed=0):
    """Partial filters [nsplit][9][CBP][CAP] and bias rows [nsplit][CBP] with NaN in the pad rows / columns.
    kind "weights": split s = w_s x one pattern with entries in {-2, -1, 1, 2}, the w_s distinct integers 1..nsplit in a seeded order
      (a dropped, doubled or swapped split changes EVERY entry; the sums stay below 2^24: exact);
    kind "cancel": the first nsplit // 2 splits are integers of magnitude up to 2^23, the next nsplit // 2 their negatives (in a
      seeded order of their own, so that a value and its negative seldom meet in one addition) plus grid values in -2..2, an odd
      last split is a plain grid split: the sum is a small integer, exact in double in any order, and out of reach of an fp32
      accumulation;
    kind "randn"."""
    CBP, CAP = reduce_pads(CB, CA)
    rng = np.random.default_rng(33000 + seed + 7 * nsplit + 131 * CB + CA + len(kind))
    shape = (nsplit, 9 * CBP * CAP + CBP)                 # filter part and bias row of a split side by side
    if kind == "weights":
        pat = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), shape[1])
        w = rng.permutation(nsplit) + 1.0
        a = w[:, None] * pat[None]
    elif kind == "cancel":
        h = nsplit // 2
        big = rng.integers(-2 ** 23, 2 ** 23 + 1, (h, shape[1])).astype(np.float64)
        small = rng.integers(-2, 3, (nsplit - h, shape[1])).astype(np.float64)
        a = np.concatenate([big, small])
        a[h:2 * h] -= big[rng.permutation(h)]
    else:
        a = rng.standard_normal(shape)
    a = a.astype(f32)
    part, bias = a[:, :9 * CBP * CAP].reshape(nsplit, 9, CBP, CAP).copy(), a[:, 9 * CBP * CAP:].copy()
    part[:, :, CB:, :], part[:, :, :, CA:], bias[:, CB:] = np.nan, np.nan, np.nan
    return dict(nsplit=nsplit, CB=CB, CA=CA, CBP=CBP, CAP=CAP, kind=kind, part=part, bias=bias)


def reduce_buffer(c, with_bias):
    """The workspace as the reduction reads it: [nsplit][9][CBP][CAP], then (with the bias) [nsplit][CBP], then one more split of NaN."""
    tail = np.full(9 * c["CBP"] * c["CAP"] + c["CBP"], np.nan, f32)
    return np.concatenate([c["part"].reshape(-1)] + ([c["bias"].reshape(-1)] if with_bias else []) + [tail])


def reduce_reference(c, keep=None):
    """(dW, db) in float64; keep: boolean over the splits."""
    k = slice(None) if keep is None else np.asarray(keep, bool)
    return R.wgrad_reduce(c["part"][k], c["bias"][k], c["CB"], c["CA"])


def reduce_fixed_order_fp32(x):
    """x [nsplit][...] fp32 -> the sum in wgrad_reduce_block's order of additions, every addition rounded to fp32: group grp adds
    the splits grp, grp + 16, ..., four at a time ((s, s + 32) and (s + 16, s + 48) on two accumulators) while s + 48 < nsplit, then
    singly; the 16 group sums are added as ((0 + 1) + (2 + 3)) + ... in steps of four."""
    ns = x.shape[0]
    z = np.zeros(x.shape[1:], f32)
    sh = []
    for grp in range(16):
        a0, a1, s = z.copy(), z.copy(), grp
        while s + 48 < ns:
            a0 = a0 + (x[s] + x[s + 32])
            a1 = a1 + (x[s + 16] + x[s + 48])
            s += 64
        while s < ns:
            a0 = a0 + x[s]
            s += 16
        sh.append(a0 + a1)
    u = z.copy()
    for g in range(0, 16, 4):
        u = u + ((sh[g] + sh[g + 1]) + (sh[g + 2] + sh[g + 3]))
    assert u.dtype == f32
    return u


# smallest share of the real entries (filter and bias together) that an fp32 accumulation in the kernel's order gets wrong on the
# "cancel" case, per nsplit: half of what tests/test_small_ops.py measures (0 where two splits cancel inside one addition)
REDUCE_FP32_MISS = {1: 0.0, 2: 0.0, 15: 0.04, 16: 0.08, 17: 0.09, 32: 0.16, 48: 0.27, 49: 0.24, 63: 0.32, 64: 0.32, 65: 0.31, 112: 0.41,
                    113: 0.40, 129: 0.40, 200: 0.43}


def check_reduce(c):
    """The preconditions of the two exact kinds."""
    CB, CA = c["CB"], c["CA"]
    real, realb = c["part"][:, :, :CB, :CA].astype(np.float64), c["bias"][:, :CB].astype(np.float64)
    assert not np.isnan(real).any() and not np.isnan(realb).any()
    assert np.isnan(c["part"][:, :, CB:]).all() and np.isnan(c["part"][:, :, :, CA:]).all() and np.isnan(c["bias"][:, CB:]).all()
    dw, db = reduce_reference(c)
    assert np.all(dw == np.round(dw)) and np.all(db == np.round(db)) and max(np.abs(dw).max(), np.abs(db).max()) < 2.0 ** 24
    if c["kind"] == "weights":
        R.assert_exact(np.abs(real).sum(0), 1.0, "reduce weights")
        assert_sensitive(lambda k: reduce_reference(c, k), c["nsplit"], 16, "wgrad_reduce %d splits" % c["nsplit"])
        w = np.abs(real[:, 0, 0, 0]) / np.abs(real[:, 0, 0, 0]).min()
        assert len(set(w.tolist())) == c["nsplit"], "the splits' weights must be distinct"
        assert np.all(real != 0) and np.all(realb != 0)                 # so any split counted twice moves every entry as well
    else:
        assert max(np.abs(dw).max(), np.abs(db).max()) <= 2 * (c["nsplit"] - c["nsplit"] // 2)


def reduce_fp32_miss(c):
    """Share of the real entries on which the fixed-order fp32 sum differs from the float64 one."""
    CB, CA = c["CB"], c["CA"]
    dw, db = reduce_reference(c)
    gw = reduce_fixed_order_fp32(c["part"][:, :, :CB, :CA])
    gb = reduce_fixed_order_fp32(c["bias"][:, :CB])
    wrong = int((gw.transpose(1, 2, 0).reshape(dw.shape) != dw).sum()) + int((gb != db).sum())
    return wrong / float(dw.size + db.size)


# ------------------------------------------------------------------------------------------ confusion counts
CONF_CLASSES = (1, 2, 5, 8)
CONF_ODD_LABELS = (-100, -1, None, 255, 2 ** 32 + 1, -2 ** 32 + 2)      # None = C


def confusion_planes():
    """(N, H, W): one workgroup per image; an odd plane; one pixel; a plane just past the kernel's workgroup cap (64 workgroups x
    256 threads x 8 pixels = 131072 per image), where its grid-stride loop goes round once more than the launcher sized it for."""
    big = (2, 257, 513)
    assert big[1] * big[2] > 64 * 256 * 8
    return [(3, 24, 40), (2, 37, 53), (2, 1, 1), big]


def build_confusion(N, H, W, C, seed=0):
    """uint8 predictions (some >= C) and int64 labels with about 5 % outside [0, C) -- 2^32 + 1 and -2^32 + 2 among them, which a
    32-bit truncation would take for classes 1 and 2; the last pixel of the last image carries a (pred, label) pair found nowhere
    else where C > 1."""
    rng = np.random.default_rng(34000 + seed + N * H * W + C)
    pred = rng.integers(0, C + 2, (N, H, W)).astype(np.uint8)
    tgt = rng.integers(0, C, (N, H, W)).astype(np.int64)
    odd = rng.random((N, H, W)) < 0.05
    vals = np.array([C if x is None else x for x in CONF_ODD_LABELS], np.int64)
    tgt[odd] = vals[rng.integers(0, len(vals), int(odd.sum()))]
    if N * H * W >= len(vals):
        tgt.reshape(-1)[:len(vals)] = vals                   # every odd label at least once
    if C > 1 and H * W > 1:
        tgt[-1][(pred[-1] == C - 1) & (tgt[-1] == 0)] = -1
        pred[-1, -1, -1], tgt[-1, -1, -1] = C - 1, 0
    return pred, tgt
