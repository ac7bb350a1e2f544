"""Shapes, load modes and record builders of the dilated and decoder-order cases of tests/test_gpu_kernels.py: the conv / transposed-conv
/ filter-gradient records that PB_FCN, PB_FCN_2 and LabelProp emit in training (engine.py bwd_conv / bwd_up; model.py ConvPoolSimple /
ConvPool) and the ROBO-UNet / U-Net step does not -- dilation 2 on NHWC operands, the `bn_relu` order (gathered operand
RCV_LOAD_AFFINE_RELU, gradient RCV_LOAD_GRAD_DEC) and the `relu` order (RCV_LOAD_PLAIN, RCV_LOAD_GRAD_ENC with the rows (1, 0, 0)) --
and of the records behind the packer's flip and scale branches: stride-1 data gradients, the 3x3 classifier's data gradient, folded
inference records.

Records only, no tensors and no device: tests/test_lib_abi.py plans every one of them on the planning handle and pins the kernel
labels they reach, so that a planner change which moves them onto another kernel shows there and not as a silent loss of coverage."""
from robocupvision_amd import _lib as L

# (N, H, W, Cin, Cout, stride, dilation): the smallest planes that still reach each kernel, its ragged edges and its
# several-tiles-per-workgroup path; label -> shapes as the planner answers for 256 CUs (layout 0)
DILATED_CONV_LABELS = {
    (2, 37, 53, 64, 128, 1, 2): "conv_dma<1,5,4,1,4>", (2, 37, 53, 128, 64, 1, 2): "conv_dma<1,5,4,1,4>",
    (3, 5, 7, 128, 64, 1, 2): "conv_dma<1,5,4,1,4>", (2, 3, 4, 64, 64, 1, 2): "conv_dma<1,5,4,1,4>",
    (2, 30, 40, 64, 32, 1, 2): "conv_mfma<1,5,2,2,8>",
    (2, 33, 47, 16, 16, 1, 2): "convs_mfma<1,5,16>", (2, 33, 47, 8, 16, 1, 2): "convs_mfma<1,5,8>",
    (2, 33, 47, 32, 16, 1, 2): "convs_mfma<1,3,32>",
    (1, 2, 2, 32, 32, 1, 2): "convs_mfma<2,3,32>",          # every off-centre tap lies in the padding
}
DILATED_CONV_SHAPES = list(DILATED_CONV_LABELS)
STRIDE2_DILATED_CONV_SHAPES = [(2, 24, 40, 64, 64, 2, 2), (2, 33, 47, 16, 32, 2, 2)]
STRIDE2_CONV_SHAPES = [(2, 48, 64, 16, 32, 2, 1), (2, 30, 40, 32, 64, 2, 1), (2, 14, 18, 64, 128, 2, 1), (2, 48, 64, 8, 16, 2, 1)]
STRIDE1_CONV_SHAPES = [(4, 30, 40, 64, 64, 1, 1), (4, 30, 40, 32, 32, 1, 1), (2, 37, 53, 16, 16, 1, 1)]
# Tilings that only whole networks reached (tests/test_plan_census.py: the records of the bench.py workloads, LabelProp and PB_FCN
# against the records of the kernel-level tests): the smallest plane (N x H x W, found by sweeping the planner) that selects each,
# (shape, filter layout) -> label for 256 CUs.  The two conv_mfma tilings are chosen by tile count against the CU count: nothing
# smaller than 2 x 128 x 171 resp. 52 x 44 x 59 selects them.
CENSUS_CONV_LABELS = {
    ((2, 128, 171, 64, 32, 1, 1), 0): "conv_mfma<2,5,1,4,8>", ((52, 44, 59, 16, 64, 2, 1), 0): "conv_mfma<2,5,2,2,8>",
    ((2, 15, 20, 16, 32, 1, 1), 3): "convn_bf3<16,2,5>", ((2, 30, 40, 32, 16, 1, 1), 3): "convn_bf3<32,1,5>",
    ((2, 8, 10, 16, 16, 2, 1), 0): "convs_mfma<1,2,16>", ((2, 16, 24, 16, 16, 1, 1), 0): "convs_mfma<1,3,16>",
    ((2, 16, 24, 16, 32, 1, 2), 0): "convs_mfma<2,3,16>", ((2, 8, 10, 8, 32, 2, 1), 0): "convs_mfma<2,3,8>",
    ((2, 15, 20, 16, 32, 1, 2), 0): "convs_mfma<2,5,16>",
}
CENSUS_CONV_SHAPES = list(dict.fromkeys(sh for sh, _ in CENSUS_CONV_LABELS))
CONV_RECORD_SHAPES = DILATED_CONV_SHAPES + STRIDE2_DILATED_CONV_SHAPES + STRIDE2_CONV_SHAPES + STRIDE1_CONV_SHAPES + CENSUS_CONV_SHAPES

# load mode of the gathered operand -> (RCV_LOAD_*, flags, statistics).  The two gradient loads as the data-gradient launches carry them
# (a residual: the skip tensor's share); the two activation loads with the statistics of the training forward -- without statistics most
# of these planes go to conv_small.
CONV_RECORD_MODES = {
    "grad_dec": (L.LOAD_GRAD_DEC, L.F_RESID, L.STATS_NONE),
    "grad_enc_relu": (L.LOAD_GRAD_ENC, L.F_RESID, L.STATS_NONE),        # constants (1, 0, 0): relu(conv) without a BatchNorm
    "affine_relu": (L.LOAD_AFFINE_RELU, L.F_BIAS, L.STATS_FWD),
    "plain": (L.LOAD_PLAIN, L.F_BIAS, L.STATS_FWD),
}
TCONV_RECORD_MODES = {"grad_dec": L.LOAD_GRAD_DEC, "affine_relu": L.LOAD_AFFINE_RELU, "plain": L.LOAD_PLAIN}


def conv_layouts(Cin, Cout, s, d):
    """Filter layouts (rcv_op_filter_layout) a conv record of this shape is run under: 0 plain, 2 Winograd, 3 / 5 split-bf16 -- at
    dilation 1 what test_gpu_kernels._conv_layouts enumerates; no Winograd and no split-bf16 kernel takes dilation 2."""
    if d != 1:
        return [0]
    return [0] + ([2] if (s == 1 and Cin % 16 == 0 and Cin >= 32 and Cout >= 64) else []) + \
        ([3] if (s == 1 and Cin % 32 == 0 and Cin >= 64 and Cout >= 64) or (Cin in (8, 16, 32) and Cout <= 32) else []) + \
        ([5] if (s == 2 and Cin % 16 == 0 and Cin >= 32 and Cout >= 64) else [])


def conv_record(shape, mode_name, layout, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    mode, flags, stats = CONV_RECORD_MODES[mode_name]
    return L.make_op(L.OP_CONV, flags, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s, dil=d,
                     inmode=mode, stats=stats, aux0=layout, **ptrs)


def tconv_record(shape, mode_name, layout, **ptrs):
    N, H, W, Cin, Cout = shape
    return L.make_op(L.OP_TCONV, L.F_BIAS, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=2 * H, wo=2 * W, stride=2, dil=1,
                     inmode=TCONV_KERNEL_MODES[mode_name], aux0=layout, **ptrs)


# ------------------------------------------------------------------------------------------ the plain kernel cases
# The shape tables and record builders of test_conv_kernels_vs_fp64, test_conv_nchw_image_input_vs_fp64,
# test_filter_gradient_kernels_vs_fp64, test_filter_gradient_nchw_image_vs_fp64, test_transposed_conv_kernels_vs_fp64 and
# test_tiny_plane_conv_vs_fp64 (tests/test_gpu_kernels.py): here, so that tests/plan_census.py plans the very records those tests run.
# (N, H, W, Cin, Cout, stride)
CONV_SHAPES = [(4, 15, 20, 64, 64, 1), (4, 15, 20, 128, 64, 1), (2, 30, 40, 128, 128, 1), (4, 30, 40, 64, 32, 1), (4, 15, 20, 64, 128, 1),
               (4, 30, 40, 32, 64, 2), (4, 30, 40, 32, 32, 1), (4, 60, 80, 16, 16, 1), (3, 5, 7, 64, 64, 1), (2, 37, 53, 32, 64, 1),
               (2, 120, 160, 8, 16, 2), (5, 9, 11, 128, 128, 1), (1, 60, 80, 64, 128, 2), (2, 48, 64, 16, 32, 2),
               (32, 30, 40, 128, 128, 1), (16, 60, 80, 64, 64, 1)]      # (the planes of the 640 x 480 step: the 320-pixel tile of conv_bf3 = its 32x32x16 form)
CONV_KERNEL_MODES = {"grad_enc": L.LOAD_GRAD_ENC, "affine": L.LOAD_AFFINE}


def conv_kernel_record(shape, mode_name, layout, **ptrs):
    N, H, W, Cin, Cout, s = shape
    return L.make_op(L.OP_CONV, L.F_RESID, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s, dil=1,
                     inmode=CONV_KERNEL_MODES[mode_name], aux0=layout, **ptrs)


# (N, H, W, Cin, Cout, stride, dilation): the NCHW image as the conv's input
NCHW_CONV_SHAPES = [(2, 48, 64, 3, 8, 1, 1), (2, 120, 160, 3, 16, 1, 1), (3, 37, 53, 4, 16, 1, 1), (2, 48, 64, 3, 16, 2, 1),
                    (2, 40, 56, 3, 8, 1, 2), (1, 33, 47, 3, 16, 2, 1), (2, 24, 40, 2, 32, 1, 2)]


def nchw_conv_record(shape, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    return L.make_op(L.OP_CONV, L.F_BIAS | L.F_RELU, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s,
                     dil=d, inmode=L.LOAD_NCHW, **ptrs)


TINY_CONV_SHAPES = [(2, 15, 20, 32, 64, 1, 2), (2, 15, 20, 64, 64, 1, 2), (2, 15, 20, 64, 32, 1, 2), (1, 7, 9, 128, 64, 1, 1),
                    (3, 9, 11, 16, 48, 2, 1), (1, 30, 40, 64, 128, 1, 1), (2, 5, 3, 20, 36, 1, 2)]
TINY_CONV_MODES = [("affine_relu", 0), ("affine", 3), ("plain", 1)]       # (load, bit 0: bias, bit 1: ReLU)


def tiny_conv_record(shape, mode_name, flags, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    mode = {"plain": L.LOAD_PLAIN, "affine": L.LOAD_AFFINE, "affine_relu": L.LOAD_AFFINE_RELU}[mode_name]
    return L.make_op(L.OP_CONV, (L.F_BIAS if flags & 1 else 0) | (L.F_RELU if flags & 2 else 0), n=N, h=H, w=W, cin=Cin, cout=Cout,
                     ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s, dil=d, inmode=mode, **ptrs)


# (N, H, W, Cin, Cout): ConvTranspose2d(k3, s2, p1, output_padding 1)
TCONV_SHAPES = [(2, 15, 20, 128, 64), (2, 30, 40, 64, 32), (2, 60, 80, 32, 16), (2, 120, 160, 16, 8), (3, 7, 9, 128, 64), (1, 33, 21, 64, 32),
                (2, 24, 32, 32, 16), (4, 8, 10, 64, 64), (2, 20, 28, 16, 16), (1, 5, 6, 128, 128)]
# as CENSUS_CONV_LABELS: tconv_dma<2,5,2,2,4> and tconvm_dma<2,5,2,2,4> are chosen by tile count (nothing smaller than 64 x 8 x 11
# resp. 64 x 20 x 27 selects them)
CENSUS_TCONV_LABELS = {
    ((64, 8, 11, 128, 64), 0): "tconv_dma<2,5,2,2,4>", ((64, 20, 27, 64, 16), 1): "tconvm_dma<2,5,2,2,4>",
    ((2, 16, 24, 16, 8), 1): "tconvms_mfma<2,3,16>", ((2, 8, 10, 32, 8), 1): "tconvms_mfma<2,3,32>",
    ((2, 30, 40, 32, 16), 4): "tconvn_bf3<32,4,5>",
}
TCONV_SHAPES += list(dict.fromkeys(sh for sh, _ in CENSUS_TCONV_LABELS))
TCONV_KERNEL_MODES = dict(TCONV_RECORD_MODES, grad_enc=L.LOAD_GRAD_ENC, affine=L.LOAD_AFFINE)

# (N, H, W, Cin, Cout, stride)
WGRAD_SHAPES = [(4, 15, 20, 64, 64, 1), (4, 30, 40, 32, 64, 2), (4, 15, 20, 64, 128, 1), (4, 15, 20, 128, 128, 1), (4, 30, 40, 32, 32, 1),
                (4, 60, 80, 16, 16, 1), (4, 120, 160, 8, 16, 2), (2, 15, 20, 64, 64, 1), (4, 16, 20, 64, 64, 1), (4, 15, 24, 64, 64, 1),
                (3, 5, 7, 64, 64, 1), (4, 10, 14, 128, 64, 1), (64, 15, 20, 64, 64, 1), (1, 30, 40, 64, 64, 1), (4, 7, 10, 128, 128, 1),
                (2, 37, 53, 16, 32, 1), (2, 48, 64, 8, 8, 1), (3, 33, 47, 32, 16, 1), (2, 60, 80, 32, 64, 2), (2, 120, 160, 16, 32, 2),
                (3, 14, 18, 64, 128, 2), (1, 96, 128, 8, 16, 2),
                # planes with at least one 8 x 16 tile per CU: the narrow layers' split-bf16 kernel (wgradn_bf3.hip), every channel-tile shape
                (8, 64, 128, 16, 16, 1), (8, 64, 128, 32, 32, 1), (8, 128, 128, 16, 16, 2), (8, 128, 128, 16, 32, 2), (6, 60, 100, 32, 16, 1),
                (5, 72, 112, 16, 32, 1), (8, 128, 128, 32, 32, 2), (6, 62, 100, 16, 24, 1), (8, 128, 128, 32, 16, 2),
                # eight gathered channels, stride 2: the pixel-pair view of wgradn_bf3
                (8, 128, 128, 8, 16, 2), (8, 128, 128, 8, 32, 2), (6, 126, 140, 8, 16, 2), (7, 100, 132, 8, 24, 2)]
WGRAD_KERNEL_MODES = [False, True, "dec"]


def wgrad_kernel_record(shape, modes, **ptrs):
    """The three record forms of test_filter_gradient_kernels_vs_fp64; None where the form does not exist for the shape ("dec": the
    transposed-conv layer, stride 2 only)."""
    N, H, W, Cin, Cout, s = shape
    dims = dict(n=N, h=H, w=W, cin=Cin, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, cout=Cout, dil=1)
    if modes == "dec":      # transposed-conv layer: gathered operand = the two-tensor gradient at the 2x plane, pointwise = the layer input
        if s != 2:
            return None
        return L.make_op(L.OP_WGRAD, 0, stride=2, inmode=L.LOAD_GRAD_DEC, inmode2=L.LOAD_AFFINE, **dims, **ptrs)
    if modes:               # gathered operand: BatchNorm apply of the producer; pointwise operand: BatchNorm + ReLU backward of (g, r)
        return L.make_op(L.OP_WGRAD, L.F_BIAS, stride=s, inmode=L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_ENC, **dims, **ptrs)
    return L.make_op(L.OP_WGRAD, L.F_BIAS, stride=s, inmode=L.LOAD_PLAIN, inmode2=L.LOAD_PLAIN, **dims, **ptrs)


# (N, H, W, Cin, Cout, stride, dilation): the NCHW image as the gathered operand
NCHW_WGRAD_SHAPES = [(2, 48, 64, 3, 8, 1, 1), (2, 40, 56, 3, 8, 1, 2), (2, 48, 64, 3, 16, 1, 1), (2, 37, 53, 4, 16, 1, 1),
                     (2, 48, 64, 3, 32, 1, 1), (2, 48, 64, 4, 8, 1, 1), (1, 96, 128, 3, 16, 2, 1), (3, 24, 40, 2, 8, 1, 1),
                     # wgrad_first beyond its first tile round (every other shape above gives a workgroup one tile): on 256 CUs 1040
                     # tiles over 347 workgroups -- three rounds, the last ragged (pinned by tests/test_plan_census.py)
                     (65, 64, 80, 3, 8, 1, 1)]
WGRAD_FIRST_MULTI_ROUND = ((65, 64, 80, 3, 8, 1, 1), ("wgrad_first<1>", 347, 1040))


def nchw_wgrad_record(shape, two, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    return L.make_op(L.OP_WGRAD, L.F_BIAS, n=N, h=H, w=W, cin=Cin, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, cout=Cout, stride=s, dil=d,
                     inmode=L.LOAD_NCHW, inmode2=L.LOAD_GRAD_ENC if two else L.LOAD_PLAIN, **ptrs)


def stats_record(c, layout, kind, flags, **ptrs):
    """The record of one epilogue-statistics case (tests/small_ops_cases.py conv_stats_dims / build_conv_stats)."""
    return L.make_op(L.OP_TCONV if c["transposed"] else L.OP_CONV, flags, n=c["N"], h=c["H"], w=c["W"], cin=c["Cin"], cout=c["Cout"],
                     ho=c["Ho"], wo=c["Wo"], stride=c["s"], dil=c["d"], inmode=L.LOAD_NCHW if c["nchw"] else L.LOAD_AFFINE, aux0=layout,
                     stats=kind, **ptrs)


def stats_layouts(family, c, merged_max_cout):
    """(filter layout, merged) an epilogue-statistics case of `family` runs under (test_epilogue_statistics_exact)."""
    if family == "conv":
        return [(layout, False) for layout in conv_layouts(c["Cin"], c["Cout"], c["s"], 1)]
    if family == "tconv":
        merged = 1 if c["Cout"] <= merged_max_cout else 0
        return [(layout, merged) for layout in tconv_layouts(c["Cin"], c["Cout"], merged_max_cout)]
    return [(0, False)]


# ------------------------------------------------------------------------------------------ flipped and scaled filters
# The records whose filter the packer flips (rcv_pack_job.flip = 1: the stride-1 data gradients of engine.py bwd_conv and of the 3x3
# classifier) or scales per output channel (rcv_pack_job.scale: inference BatchNorm folding, engine.py fwd_conv / fwd_up).
# Stride-1 data gradients: shapes read as the RECORD's channels (cin = the layer's Cout, cout = the layer's Cin)
DGRAD_SHAPES = [sh for sh in DILATED_CONV_SHAPES + STRIDE1_CONV_SHAPES if sh[5] == 1] + \
    [(3, 5, 7, 64, 64, 1, 1), (2, 37, 53, 128, 64, 1, 1), (2, 37, 53, 32, 16, 1, 1)]
DGRAD_MODES = {"grad_dec": L.LOAD_GRAD_DEC, "grad_enc": L.LOAD_GRAD_ENC, "grad_enc_relu": L.LOAD_GRAD_ENC}     # (the last: rows (1, 0, 0))
# (shape, layout) -> label as the planner answers for 256 CUs, under every load of DGRAD_MODES (dilation 2: DILATED_CONV_LABELS)
DGRAD_LABELS = {
    ((4, 30, 40, 64, 64, 1, 1), 0): "conv_dma<1,5,4,1,4>", ((4, 30, 40, 64, 64, 1, 1), 2): "conv_wino<64,80>",
    ((4, 30, 40, 64, 64, 1, 1), 3): "conv_bf3<64,160>",
    ((4, 30, 40, 32, 32, 1, 1), 0): "convs_mfma<2,3,32>", ((4, 30, 40, 32, 32, 1, 1), 3): "convn_bf3<32,2,3>",
    ((2, 37, 53, 16, 16, 1, 1), 0): "convs_mfma<1,5,16>", ((2, 37, 53, 16, 16, 1, 1), 3): "convn_bf3<16,1,5>",
    ((3, 5, 7, 64, 64, 1, 1), 0): "conv_dma<1,5,4,1,4>", ((3, 5, 7, 64, 64, 1, 1), 2): "conv_wino<64,80>",
    ((3, 5, 7, 64, 64, 1, 1), 3): "conv_bf3<64,160>",
    ((2, 37, 53, 128, 64, 1, 1), 0): "conv_dma<1,5,4,1,4>", ((2, 37, 53, 128, 64, 1, 1), 2): "conv_wino<64,80>",
    ((2, 37, 53, 128, 64, 1, 1), 3): "conv_bf3<64,160>",
    ((2, 37, 53, 32, 16, 1, 1), 0): "convs_mfma<1,3,32>", ((2, 37, 53, 32, 16, 1, 1), 3): "convn_bf3<32,1,5>",
}
DGRAD_LABELS.update({(sh, 0): lab for sh, lab in DILATED_CONV_LABELS.items()})


def dgrad_record(shape, mode_name, layout, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    return L.make_op(L.OP_CONV, L.F_RESID, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=H, wo=W, stride=1, dil=d, inmode=DGRAD_MODES[mode_name],
                     stats=L.STATS_NONE, aux0=layout, **ptrs)


# the 3x3 classifier's data gradient: the class gradient in 8 NHWC channels (zero beyond the classes) -> the classifier's input channels
CLS_DGRAD_PLANES = [(2, 37, 53), (1, 9, 11)]
CLS_DGRAD_CLASSES = [1, 3, 5, 8]
CLS_DGRAD_COUT = [8, 16]
CLS_DGRAD_LABELS = {((2, 37, 53), 8): "convs_mfma<1,5,8>", ((2, 37, 53), 16): "convs_mfma<1,5,8>",
                    ((1, 9, 11), 8): "convs_mfma<1,3,8>", ((1, 9, 11), 16): "convs_mfma<1,3,8>"}


def cls_dgrad_record(plane, cout, **ptrs):
    N, H, W = plane
    return L.make_op(L.OP_CONV, L.F_RESID, n=N, h=H, w=W, cin=8, cout=cout, ho=H, wo=W, stride=1, dil=1, inmode=L.LOAD_PLAIN, **ptrs)


# folded inference records: relu(op(x, w * scale) + bias) (+ the skip tensor behind a transposed conv); one conv shape per family
# (stride 1 wide and narrow, stride 2, dilation 2) and the image layer in the reference's own layout
FOLDED_CONV_CASES = [((4, 30, 40, 64, 64, 1, 1), "plain"), ((2, 37, 53, 16, 16, 1, 1), "plain"), ((2, 30, 40, 32, 64, 2, 1), "plain"),
                     ((2, 37, 53, 64, 128, 1, 2), "plain"), ((2, 48, 64, 3, 8, 1, 1), "nchw")]
FOLDED_TCONV_SHAPES = [(2, 15, 20, 128, 64), (2, 24, 32, 32, 16), (2, 20, 28, 16, 16), (1, 5, 6, 128, 128)]
# (shape, load, layout) / (shape, layout) -> label as the planner answers for 256 CUs
FOLDED_CONV_LABELS = {
    ((4, 30, 40, 64, 64, 1, 1), "plain", 0): "conv_dma<1,5,4,1,4>", ((4, 30, 40, 64, 64, 1, 1), "plain", 2): "conv_wino<64,80>",
    ((4, 30, 40, 64, 64, 1, 1), "plain", 3): "conv_bf3<64,160>",
    ((2, 37, 53, 16, 16, 1, 1), "plain", 0): "convs_mfma<1,5,16>", ((2, 37, 53, 16, 16, 1, 1), "plain", 3): "convn_bf3<16,1,5>",
    ((2, 30, 40, 32, 64, 2, 1), "plain", 0): "conv_small<1>", ((2, 30, 40, 32, 64, 2, 1), "plain", 5): "conv2_bf3<64,160>",
    ((2, 37, 53, 64, 128, 1, 2), "plain", 0): "conv_dma<1,5,4,1,4>", ((2, 48, 64, 3, 8, 1, 1), "nchw", 0): "conv_first<1>",
}
FOLDED_TCONV_LABELS = {
    ((2, 15, 20, 128, 64), 0): "tconva_dma<1,5,4,1,4>", ((2, 24, 32, 32, 16), 1): "tconvms_mfma<4,3,32>",
    ((2, 24, 32, 32, 16), 4): "tconvn_bf3<32,4,3>", ((2, 20, 28, 16, 16), 1): "tconvms_mfma<4,3,16>",
    ((1, 5, 6, 128, 128), 0): "tconva_dma<1,5,4,1,4>",
}


def folded_conv_record(shape, load, layout, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    return L.make_op(L.OP_CONV, L.F_BIAS | L.F_RELU, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, stride=s,
                     dil=d, inmode={"plain": L.LOAD_PLAIN, "nchw": L.LOAD_NCHW}[load], aux0=layout, **ptrs)


def tconv_layouts(Cin, Cout, merged_max_cout):
    """Filter layouts a transposed-conv record is run under (as test_transposed_conv_kernels_vs_fp64 enumerates them): 0 or 1 (merged
    parity, up to engine.MERGED_TCONV_MAX_COUT output channels), and 4 where the split-bf16 narrow kernel is built."""
    merged = 1 if Cout <= merged_max_cout else 0
    return [merged] + ([4] if merged and (Cin, (4 * Cout + 15) // 16 * 16) in ((16, 32), (32, 64)) else [])


def folded_tconv_record(shape, layout, **ptrs):
    N, H, W, Cin, Cout = shape
    return L.make_op(L.OP_TCONV, L.F_BIAS | L.F_RELU | L.F_RESID, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=2 * H, wo=2 * W, stride=2, dil=1,
                     inmode=L.LOAD_PLAIN, aux0=layout, **ptrs)


# ------------------------------------------------------------------------------------------ the layer shapes of the networks
NETWORK_PLANES = [(32, 480, 640), (64, 120, 160), (32, 240, 320), (2, 48, 64), (1, 32, 48), (3, 37, 53), (1, 9, 11), (5, 130, 70)]
NETWORK_CHANNELS = [(3, 8), (8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 64), (24, 40), (4, 12)]


def network_layer_records():
    """(what, record) for every conv / transposed-conv / filter-gradient record the ROBO-UNet, U-Net and PB_FCN graphs produce at the
    BASELINE sizes and at ragged / tiny planes; what: "conv", "wgrad", "wgrad_nchw" (the image as the gathered operand) or "tconv".
    The sweep of tests/test_lib_abi.py and of scripts/plan_dump.py."""
    for (n, H, W) in NETWORK_PLANES:
        for (ci, co) in NETWORK_CHANNELS:
            for s in (1, 2):
                for d in ((1, 2) if s == 1 else (1,)):
                    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
                    if ci >= 4:
                        for mode in (L.LOAD_AFFINE, L.LOAD_GRAD_ENC):
                            yield "conv", L.make_op(L.OP_CONV, L.F_BIAS, n=n, h=H, w=W, cin=ci, cout=co, ho=Ho, wo=Wo, stride=s, dil=d,
                                                    inmode=mode, stats=L.STATS_FWD)
                        yield "wgrad", L.make_op(L.OP_WGRAD, L.F_BIAS, n=n, h=H, w=W, cin=ci, ho=Ho, wo=Wo, cout=co, stride=s, dil=d,
                                                 inmode=L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_ENC)
                    elif d == 1 or s == 1:
                        yield "wgrad_nchw", L.make_op(L.OP_WGRAD, L.F_BIAS, n=n, h=H, w=W, cin=ci, ho=Ho, wo=Wo, cout=co, stride=s, dil=d,
                                                      inmode=L.LOAD_NCHW, inmode2=L.LOAD_GRAD_ENC)
            if ci >= 4 and co % 4 == 0:
                yield "tconv", L.make_op(L.OP_TCONV, L.F_BIAS, n=n, h=H, w=W, cin=ci, cout=co, ho=2 * H, wo=2 * W, stride=2, dil=1,
                                         inmode=L.LOAD_AFFINE, stats=L.STATS_FWD)


# ------------------------------------------------------------------------------------------ filter gradients
# (gathered, pointwise) load modes -> (RCV_LOAD_* of the gathered operand, of the pointwise operand, flags)
WGRAD_RECORD_PAIRS = {
    "affine_relu,grad_dec": (L.LOAD_AFFINE_RELU, L.LOAD_GRAD_DEC, 0),     # a bn_relu conv after a bn_relu producer: bias ahead of a BatchNorm
    "plain,grad_enc_relu": (L.LOAD_PLAIN, L.LOAD_GRAD_ENC, 0),           # ConvPool.conv1: constants (1, 0, 0)
    "affine,grad_dec": (L.LOAD_AFFINE, L.LOAD_GRAD_DEC, L.F_BIAS),       # a bn_relu conv after a relu_bn producer; here with the bias sums
}
# run-time-geometry wgrad_mfma tiles (no split-bf16 kernel takes dilation 2)
DILATED_WGRAD_SHAPES = DILATED_CONV_SHAPES + STRIDE2_DILATED_CONV_SHAPES + [(2, 37, 53, 128, 128, 1, 2)]
DILATED_WGRAD_LABELS = {"wgrad_mfma<2,2,2,2,1,f0>", "wgrad_mfma<2,2,1,2,2,f0>", "wgrad_mfma<1,1,1,1,4,f0>", "wgrad_mfma<1,1,1,1,4,f5>",
                        "wgrad_mfma<1,2,1,1,4,f0>", "wgrad_mfma<2,2,1,1,4,f0>", "wgrad_mfma<2,1,1,1,4,f0>"}
# dilation 1, each under flags 0 (the split-bf16 kernel where the planner has one) and under RCV_F_MFMA_FP32 (always wgrad_mfma);
# shape -> (label under flags 0, label under RCV_F_MFMA_FP32) as the planner answers for 256 CUs: the last two planes are too small for a
# split-bf16 kernel and stay on the fp32 matrix instruction either way
MATRIX_WGRAD_LABELS = {(4, 15, 20, 64, 64, 1, 1): ("wgrad_bf3<8>", "wgrad_mfma<2,2,2,2,1,f0>"),
                       (4, 15, 20, 128, 128, 1, 1): ("wgrad_bf3<8>", "wgrad_mfma<2,2,2,2,1,f0>"),
                       (8, 64, 128, 16, 16, 1, 1): ("wgradn_bf3<16,1>", "wgrad_mfma<1,1,1,1,4,f0>"),
                       (8, 128, 128, 16, 32, 2, 1): ("wgradn_bf3<8,2>", "wgrad_mfma<2,1,1,1,4,f0>"),
                       (4, 30, 40, 32, 64, 2, 1): ("wgrad_mfma<2,2,2,1,2,f0>", "wgrad_mfma<2,2,2,1,2,f0>"),
                       (3, 14, 18, 64, 128, 2, 1): ("wgrad_mfma<2,2,2,2,1,f0>", "wgrad_mfma<2,2,2,2,1,f0>")}
MATRIX_WGRAD_SHAPES = list(MATRIX_WGRAD_LABELS)


def wgrad_kernel(shape, matrix_flags):
    """The kernel family (label ahead of '<') a filter-gradient record of these cases runs on."""
    if shape not in MATRIX_WGRAD_LABELS:
        return "wgrad_mfma"
    return MATRIX_WGRAD_LABELS[shape][1 if matrix_flags & L.F_MFMA_FP32 else 0].split("<")[0]


def wgrad_record(shape, pair, matrix_flags=0, **ptrs):
    N, H, W, Cin, Cout, s, d = shape
    gmode, pmode, flags = WGRAD_RECORD_PAIRS[pair]
    return L.make_op(L.OP_WGRAD, flags | matrix_flags, n=N, h=H, w=W, cin=Cin, ho=(H - 1) // s + 1, wo=(W - 1) // s + 1, cout=Cout,
                     stride=s, dil=d, inmode=gmode, inmode2=pmode, **ptrs)


# ------------------------------------------------------------------------------------------ several tile rounds per workgroup
# The persistent kernels (convs_mfma / tconvms_mfma, convn_bf3 / tconvn_bf3, conv_first) beyond their first tile round: planes on
# which, on 256 CUs, a workgroup loops over three tiles or more with a ragged last round (conv_first, which keeps no buffer across
# tiles: over two) -- the prefetch of the next tile, the parity of the double-buffered staging, the tile index of the later rounds.
# (what, shape, filter layout, (label, workgroups, tiles) as the planner answers for 256 CUs).  what: "conv" (N, H, W, Cin, Cout,
# stride), "tconv" (N, H, W, Cin, Cout), "first" (the NCHW image).  tests/test_plan_census.py pins the last column and asserts the
# condition; tests/test_gpu_kernels.py::test_multi_round_records_vs_fp64 runs them and re-asserts it on the real handle.
# The smallest N on planes of 64 x 80, 96 x 128 and 100 x 140 (ragged against every tile) at which the condition holds; the first
# layer with N chosen for one and a half rounds.
MULTI_ROUND_CASES = [
    ("conv", (65, 64, 80, 8, 8, 1), 0, ("convs_mfma<1,5,8>", 347, 1040)),
    ("conv", (13, 96, 128, 8, 8, 1), 3, ("convn_bf3<8,1,5>", 256, 520)),
    ("conv", (65, 64, 80, 16, 16, 1), 0, ("convs_mfma<1,5,16>", 347, 1040)),
    ("conv", (13, 96, 128, 16, 16, 1), 3, ("convn_bf3<16,1,5>", 256, 520)),
    ("conv", (19, 64, 80, 32, 32, 1), 0, ("convs_mfma<2,3,32>", 178, 532)),
    ("conv", (19, 64, 80, 32, 32, 1), 3, ("convn_bf3<32,2,3>", 256, 532)),
    ("conv", (31, 100, 140, 16, 32, 2), 0, ("convs_mfma<2,2,16>", 352, 1054)),
    ("conv", (52, 64, 80, 16, 32, 2), 3, ("convn_bf3<16,2,3>", 256, 520)),
    ("conv", (52, 100, 140, 8, 16, 2), 0, ("convs_mfma<1,3,8>", 347, 1040)),
    ("conv", (43, 100, 140, 8, 16, 2), 3, ("convn_bf3<8,1,5>", 256, 516)),
    ("tconv", (65, 64, 80, 16, 8), 1, ("tconvms_mfma<2,5,16>", 347, 1040)),
    ("tconv", (12, 100, 140, 16, 8), 4, ("tconvn_bf3<16,2,5>", 256, 540)),
    ("tconv", (37, 64, 80, 32, 16), 1, ("tconvms_mfma<4,3,32>", 346, 1036)),
    ("tconv", (9, 96, 128, 32, 16), 4, ("tconvn_bf3<32,4,3>", 256, 576)),
    ("first", (73, 100, 140, 3, 8, 1), 0, ("conv_first<1>", 1024, 1533)),
]
MULTI_ROUND_MODES = {
    "affine_relu": (L.LOAD_AFFINE_RELU, L.F_BIAS, L.STATS_FWD),       # the training forward: bias, partial rows
    "grad_dec": (L.LOAD_GRAD_DEC, L.F_RESID, L.STATS_NONE),           # the data gradients: two-tensor load, residual
    "grad_enc": (L.LOAD_GRAD_ENC, L.F_RESID, L.STATS_NONE),
    "nchw": (L.LOAD_NCHW, L.F_BIAS, L.STATS_FWD),                     # the first layer (no other load, no residual)
}


def multi_round_modes(case):
    return ["nchw"] if case[0] == "first" else ["affine_relu", "grad_dec", "grad_enc"]


def multi_round_dims(case):
    """(N, H, W, Cin, Cout, Ho, Wo, stride) of a multi-round case."""
    what, shape = case[0], case[1]
    if what == "tconv":
        N, H, W, Cin, Cout = shape
        return N, H, W, Cin, Cout, 2 * H, 2 * W, 2
    N, H, W, Cin, Cout, s = shape
    return N, H, W, Cin, Cout, (H - 1) // s + 1, (W - 1) // s + 1, s


def multi_round_record(case, mode_name, stream=False, **ptrs):
    N, H, W, Cin, Cout, Ho, Wo, s = multi_round_dims(case)
    mode, flags, stats = MULTI_ROUND_MODES[mode_name]
    return L.make_op(L.OP_TCONV if case[0] == "tconv" else L.OP_CONV, flags | (L.F_STREAM_OUT if stream else 0), n=N, h=H, w=W, cin=Cin,
                     cout=Cout, ho=Ho, wo=Wo, stride=s, dil=1, inmode=mode, stats=stats, aux0=case[2], **ptrs)
