"""Kernel-level accuracy through the C ABI against PyTorch CPU in float64: one op record (+ its pack / reduce) per case, plain operands
and the load transforms of the step (BatchNorm apply, BatchNorm + ReLU backward), on planes that are large, tiny and ragged.

Bars (max error relative to the largest entry of the fp64 result): convolutions 3e-6 (direct) / 2e-6 (Winograd), filter gradients 5e-7,
bias gradients 5e-7.  Measured (scripts/experiments/conv_check.py, wgrad_check.py): <= 1.1e-6, <= 4.9e-7, <= 1.7e-7, <= 1.5e-7.

The records only PB_FCN, PB_FCN_2 and LabelProp emit in training -- dilation 2 on NHWC operands (also at stride 2), the loads of the
conv -> BatchNorm -> ReLU order (RCV_LOAD_AFFINE_RELU, RCV_LOAD_GRAD_DEC) and of relu(conv) without a BatchNorm (RCV_LOAD_PLAIN,
RCV_LOAD_GRAD_ENC with the rows (1, 0, 0)), the fp32-instruction filter gradients under RCV_F_MFMA_FP32 with these loads -- are the
cases of tests/conv_record_cases.py, at the same bars; measured <= 1.41e-6 (convolutions, dilation 2, 128 input channels), <= 3.3e-7
(Winograd), <= 1.35e-7 (filter gradients), <= 6.1e-8 (bias gradients); per kernel label in the docstrings of the tests.

The records whose filter the packer flips (rcv_pack_job.flip: the stride-1 data gradients, the 3x3 classifier's data gradient) or scales
per output channel (rcv_pack_job.scale: inference BatchNorm folding) run at the same bars, the folded ones also per channel against the
unscaled record; measured <= 1.86e-6 (data gradients), <= 1.27e-6 (folded).  The packer's output itself: tests/test_gpu_pack.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conv_record_cases as RC      # noqa: E402  (tests/conv_record_cases.py: the dilated and decoder-order records)
import small_ops_cases as K         # noqa: E402  (tests/small_ops_cases.py: the operands of the epilogue-statistics cases)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _load_fp64(mode, x, aux, c, L):
    X, A, C = x.double(), aux.double(), c.double()
    if mode == L.LOAD_GRAD_ENC:        # rcv.h: v = aux > 0 ? c0*x + c1 + c2*aux : 0
        return torch.where(A > 0, C[0] * X + C[1] + C[2] * A, torch.zeros((), dtype=torch.float64))
    if mode == L.LOAD_GRAD_DEC:        # v = c0*(aux*c3 + c4 > 0 ? x : 0) + c1 + c2*aux
        return C[0] * torch.where(A * C[3] + C[4] > 0, X, torch.zeros((), dtype=torch.float64)) + C[1] + C[2] * A
    if mode == L.LOAD_AFFINE:          # v = x*c0 + c1
        return X * C[0] + C[1]
    if mode == L.LOAD_AFFINE_RELU:     # v = max(x*c0 + c1, 0)
        return torch.clamp_min(X * C[0] + C[1], 0.0)
    return X


def _pack_dims(rows, cols, layout, merged=False):
    """rows_pad, cols_pad, floats of the packed filter for a layout of rcv_pack_job.merged (as engine._Lowering.add_pack sizes it)."""
    split = layout in (3, 4, 5)
    rp = (rows + 31) // 32 * 32 if (split and rows > 32) else ((rows + 7) // 8 * 8 if split else (rows + 3) // 4 * 4)
    if layout == 5:
        rp = (rows + 15) // 16 * 16
    cp = (cols * (4 if merged else 1) + 15) // 16 * 16
    taps = 16 if layout == 2 else (4 if merged else 9)
    ksteps = (rp // 16) * 5 if layout == 5 else (taps * rp + 31) // 32
    return rp, cp, (3 * ksteps * cp * 16 if split else taps * rp * cp)


CONV_SHAPES = RC.CONV_SHAPES      # (the tables and record builders of the plain cases: tests/conv_record_cases.py)


@pytest.mark.parametrize("N,H,W,Cin,Cout,s", CONV_SHAPES)
@pytest.mark.parametrize("mode_name", list(RC.CONV_KERNEL_MODES))
def test_conv_kernels_vs_fp64(N, H, W, Cin, Cout, s, mode_name):
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    mode = RC.CONV_KERNEL_MODES[mode_name]
    gen = torch.Generator().manual_seed(1000 + H * W + Cin)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, xa, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, resid = _rand(gen, Cout, Cin, 3, 3, scale=0.1), _rand(gen, N, Ho, Wo, Cout)
    ref = F.conv2d(_load_fp64(mode, x, xa, c, L).permute(0, 3, 1, 2), w.double(), stride=s, padding=1).permute(0, 2, 3, 1) + resid.double()
    xd, xad, cd, wd, rd = (v.to(DEV) for v in (x, xa, c, w, resid))
    # filter layouts (rcv_op_filter_layout): 0 plain, 2 Winograd, 3 split-bf16 (conv_bf3.hip: fp32 products as six bf16 MFMA products)
    # 3 on the wide stride-1 layers: conv_bf3.hip; on the 8 / 16 / 32 -> <= 32 channel layers (stride 1 | 2): convn_bf3.hip
    # (5: the stride-2 wide layers, conv2_bf3_kernel)
    for wino in RC.conv_layouts(Cin, Cout, s, 1):
        rp, cp, nfl = _pack_dims(Cin, Cout, wino)
        wp = torch.zeros(nfl, device=DEV)
        job = L.RcvPackJob()
        job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), Cout, Cin
        job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = 1, 0, rp, cp, wino
        table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
        out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
        pack = L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr())
        conv = RC.conv_kernel_record((N, H, W, Cin, Cout, s), mode_name, wino, p_in=xd.data_ptr(), p_in_aux=xad.data_ptr(),
                                     p_in_c=cd.data_ptr(), p_w=wp.data_ptr(), p_out=out.data_ptr(), p_resid=rd.data_ptr())
        lst = L.OpList([pack, conv])
        label = lst.labels(h)[1]
        assert label.startswith("conv_wino") == (wino == 2) and ("_bf3" in label) == (wino in (3, 5)), label
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(".%s %s: max error %.3e" % (label, (N, H, W, Cin, Cout), err))
        assert err <= (2e-6 if wino == 2 else 3e-6), (label, err)


def _relu_grad_rows(C):
    """The constants of RCV_LOAD_GRAD_ENC behind relu(conv) without a BatchNorm (engine.py bwd_conv): v = aux > 0 ? 1*x + 0 + 0*aux : 0."""
    c = torch.zeros(5, C)
    c[0] = 1.0
    return c


@pytest.mark.parametrize("shape", RC.CONV_RECORD_SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("mode_name", list(RC.CONV_RECORD_MODES))
def test_dilated_and_decoder_order_conv_records_vs_fp64(shape, mode_name):
    """The conv records of PB_FCN / PB_FCN_2 / LabelProp in training that the cases above do not build (tests/conv_record_cases.py):
    dilation 2 on NHWC operands -- conv_dma<1,5,4,1,4>, conv_mfma<1,5,2,2,8>, convs_mfma<1,5,16> / <1,5,8> / <1,3,32> / <2,3,32> (the
    run-time-pitch branch of convs_mfma), also at stride 2 -- and, at every shape and under every filter layout of _conv_layouts (so that
    conv_bf3, conv2_bf3, convn_bf3 and conv_wino see them too), the loads of the `bn_relu` and `relu` orders: RCV_LOAD_GRAD_DEC (random
    c0..c4) and RCV_LOAD_GRAD_ENC with the rows (1, 0, 0), both with a residual; RCV_LOAD_AFFINE_RELU and RCV_LOAD_PLAIN with the bias and
    RCV_STATS_FWD of the training forward (NaN-prefilled partial rows; without statistics most of these planes run on conv_small).  The
    masks are decided in float64 from the fp32 operands: the kernel's single fmaf has the sign of that exact expression.
    Bars: 3e-6 (2e-6 Winograd) of the largest entry of the fp64 result; the float64 sum of the partial rows within
    close(rtol=1e-4, floor=1.0) of the float64 sums.
    Measured (MI355X, largest over the four modes).  Dilation 2: conv_dma<1,5,4,1,4> 1.41e-6 (128 -> 64 channels, plain; 8.8e-7 at
    stride 2), conv_mfma<1,5,2,2,8> 1.02e-6, convs_mfma<1,5,16> 3.7e-7, <1,5,8> 2.3e-7, <1,3,32> 5.8e-7, <2,3,32> 7.0e-8, <2,2,16>
    (stride 2) 3.7e-7.  Dilation 1: conv_dma<1,5,4,1,4> 1.03e-6, conv_wino<64,80> 3.3e-7, conv_bf3<64,160> 8.3e-7, conv2_bf3<64,160>
    6.1e-7, convs_mfma<2,3,32> 5.9e-7, <1,5,16> 4.6e-7, <2,2,16> 3.8e-7, <1,3,8> 2.5e-7, convn_bf3<32,2,3> 5.8e-7, <16,2,3> 3.1e-7,
    <16,1,5> 2.8e-7, <8,1,3> 1.5e-7.  By mode: grad_dec 1.24e-6, grad_enc (1, 0, 0) 7.6e-7, affine_relu 1.13e-6, plain 1.41e-6."""
    from robocupvision_amd import _lib as L
    from test_gpu_blocks import close
    h = L.handle(0)
    N, H, W, Cin, Cout, s, d = shape
    mode, flags, stats = RC.CONV_RECORD_MODES[mode_name]
    gen = torch.Generator().manual_seed(4000 + H * W + Cin + 7 * d)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, xa, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, resid, bias = _rand(gen, Cout, Cin, 3, 3, scale=0.1), _rand(gen, N, Ho, Wo, Cout), _rand(gen, Cout)
    if mode_name == "grad_enc_relu":
        c = _relu_grad_rows(Cin)
    ref = F.conv2d(_load_fp64(mode, x, xa, c, L).permute(0, 3, 1, 2), w.double(), stride=s, padding=d, dilation=d).permute(0, 2, 3, 1)
    ref = ref + (resid.double() if flags & L.F_RESID else bias.double())
    ref_rows = torch.stack([ref.sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))])
    xd, xad, cd, wd, rd, bd = (v.to(DEV) for v in (x, xa, c, w, resid, bias))
    for layout in RC.conv_layouts(Cin, Cout, s, d):
        rp, cp, nfl = _pack_dims(Cin, Cout, layout)
        wp = torch.zeros(nfl, device=DEV)
        job = L.RcvPackJob()
        job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), Cout, Cin
        job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = 1, 0, rp, cp, layout
        table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
        out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
        pack = L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr())
        conv = RC.conv_record(shape, mode_name, layout, p_in=xd.data_ptr(), p_in_aux=xad.data_ptr(), p_in_c=cd.data_ptr(), p_w=wp.data_ptr(),
                             p_out=out.data_ptr(), p_resid=rd.data_ptr(), p_bias=bd.data_ptr())
        part = None
        if stats != L.STATS_NONE:
            nbytes = L.op_workspace(h, conv)
            n_part = conv.i[L.RCV_I_NPART]
            assert n_part > 0 and nbytes == n_part * 2 * Cout * 4
            part = torch.full((n_part, 2, Cout), float("nan"), device=DEV)
            conv.p[L.RCV_P_PART] = part.data_ptr()
        lst = L.OpList([pack, conv])
        label = lst.labels(h)[1]
        assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout in (3, 5)), label
        assert not label.startswith("conv_small"), label
        if shape in RC.DILATED_CONV_LABELS:      # (the tiling itself is pinned for 256 CUs by tests/test_lib_abi.py)
            assert label.split("<")[0] == RC.DILATED_CONV_LABELS[shape].split("<")[0], label
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(".%s %s %s: max error %.3e" % (label, shape, mode_name, err))
        assert err <= (2e-6 if layout == 2 else 3e-6), (label, err)
        if part is not None:
            close(part.double().cpu().sum(0), ref_rows, "%s %s %s partial rows" % (label, shape, mode_name), rtol=1e-4, floor=1.0)


@pytest.mark.parametrize("N,H,W,Cin,Cout,s,d", RC.NCHW_CONV_SHAPES)
def test_conv_nchw_image_input_vs_fp64(N, H, W, Cin, Cout, s, d):
    """RCV_LOAD_NCHW: the graph input in the reference's own layout (the 3-channel image) read by the first conv without an NHWC copy --
    on the first-layer kernel (8 output channels, stride 1) and on the narrow-layer kernel (the other shapes)."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(77 + H * W + Cin)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, w, b = _rand(gen, N, Cin, H, W), _rand(gen, Cout, Cin, 3, 3, scale=0.2), _rand(gen, Cout)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=d, dilation=d)).permute(0, 2, 3, 1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    rp, cp = (Cin + 3) // 4 * 4, (Cout + 15) // 16 * 16
    wp = torch.zeros(9 * rp * cp, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), Cout, Cin
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = 1, 0, rp, cp, 0
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
    pack = L.make_op(L.OP_PACK, 0, count=1, aux0=9 * rp * cp, p_in=table.data_ptr())
    conv = RC.nchw_conv_record((N, H, W, Cin, Cout, s, d), p_in=xd.data_ptr(), p_w=wp.data_ptr(), p_bias=bd.data_ptr(), p_out=out.data_ptr())
    lst = L.OpList([pack, conv])
    label = lst.labels(h)[1]
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 3e-6, (label, err)


WGRAD_SHAPES = RC.WGRAD_SHAPES


@pytest.mark.parametrize("N,H,W,Cin,Cout,s", WGRAD_SHAPES)
@pytest.mark.parametrize("modes", RC.WGRAD_KERNEL_MODES)
def test_filter_gradient_kernels_vs_fp64(N, H, W, Cin, Cout, s, modes):
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(2000 + H * W + Cout)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    G, P = _rand(gen, N, H, W, Cin), _rand(gen, N, Ho, Wo, Cout)
    gc, pc, Pa = torch.rand(5, Cin, generator=gen) + 0.5, _rand(gen, 5, Cout, scale=0.5), _rand(gen, N, Ho, Wo, Cout)
    Gd, Pd, gcd, pcd, Pad = (v.to(DEV) for v in (G, P, gc, pc, Pa))
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    if modes == "dec":    # transposed-conv layer: gathered operand = the two-tensor gradient at the 2x plane, pointwise = the layer input
        if s != 2:
            pytest.skip("the transposed-conv form is the stride-2 one")
        Ga = _rand(gen, N, H, W, Cin)
        gc = _rand(gen, 5, Cin, scale=0.5)
        Gad, gcd = Ga.to(DEV), gc.to(DEV)
        pc = torch.rand(5, Cout, generator=gen) + 0.5
        pcd = pc.to(DEV)
        op = RC.wgrad_kernel_record((N, H, W, Cin, Cout, s), modes, p_in=Gd.data_ptr(), p_in_aux=Gad.data_ptr(), p_in_c=gcd.data_ptr(),
                                    p_in2=Pd.data_ptr(), p_in2_c=pcd.data_ptr())
        x64, gy64 = _load_fp64(L.LOAD_GRAD_DEC, G, Ga, gc, L), _load_fp64(L.LOAD_AFFINE, P, P, pc, L)
    elif modes:      # gathered operand: BatchNorm apply of the producer; pointwise operand: BatchNorm + ReLU backward of (g, r)
        op = RC.wgrad_kernel_record((N, H, W, Cin, Cout, s), modes, p_in=Gd.data_ptr(), p_in_c=gcd.data_ptr(), p_in2=Pd.data_ptr(),
                                    p_in2_aux=Pad.data_ptr(), p_in2_c=pcd.data_ptr())
        x64, gy64 = _load_fp64(L.LOAD_AFFINE, G, G, gc, L), _load_fp64(L.LOAD_GRAD_ENC, P, Pa, pc, L)
    else:
        op = RC.wgrad_kernel_record((N, H, W, Cin, Cout, s), modes, p_in=Gd.data_ptr(), p_in2=Pd.data_ptr())
        x64, gy64 = G.double(), P.double()
    nb = L.op_workspace(h, op)
    part = torch.zeros(max(nb // 4, 4), device=DEV)
    op.p[L.RCV_P_PART] = part.data_ptr()
    has_bias = bool(op.flags & L.F_BIAS)
    red = L.make_op(L.OP_WGRAD_REDUCE, 0, cin=Cin, cout=Cout, nsplit=op.i[L.RCV_I_NSPLIT], p_part=part.data_ptr(), p_out=dw.data_ptr(),
                    p_bias=db.data_ptr() if has_bias else 0)
    lst = L.OpList([op, red])
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_weight(x64.permute(0, 3, 1, 2), (Cout, Cin, 3, 3), gy64.permute(0, 3, 1, 2), stride=s, padding=1)
    refb = gy64.sum((0, 1, 2))
    e = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
    eb = float((db.double().cpu() - refb).abs().max() / refb.abs().max()) if has_bias else 0.0
    print(".%s %s %s: max error %.3e (bias %.3e)" % (lst.labels(h)[0], (N, H, W, Cin, Cout, s), modes, e, eb))
    assert e <= 5e-7 and eb <= 5e-7, (lst.labels(h)[0], e, eb)


@pytest.mark.parametrize("shape", RC.DILATED_WGRAD_SHAPES + RC.MATRIX_WGRAD_SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("pair", list(RC.WGRAD_RECORD_PAIRS))
def test_dilated_and_decoder_order_filter_gradients_vs_fp64(shape, pair):
    """The filter-gradient records of PB_FCN / PB_FCN_2 / LabelProp that the cases above do not build (tests/conv_record_cases.py).
    (gathered, pointwise) loads: (RCV_LOAD_AFFINE_RELU, RCV_LOAD_GRAD_DEC) -- a conv -> BatchNorm -> ReLU layer behind another one --,
    (RCV_LOAD_PLAIN, RCV_LOAD_GRAD_ENC with the rows (1, 0, 0)) -- relu(conv) without a BatchNorm -- and (RCV_LOAD_AFFINE,
    RCV_LOAD_GRAD_DEC), the last with the bias sums.  Dilation 2 (stride 1 and 2) on the run-time-geometry tiles wgrad_mfma<2,2,2,2,1,f0>,
    <2,2,1,2,2,f0>, <1,1,1,1,4,f0>, <1,1,1,1,4,f5>, <1,2,1,1,4,f0>, <2,2,1,1,4,f0>, <2,1,1,1,4,f0>; dilation 1 twice, as the planner
    routes it (wgrad_bf3<8>, wgradn_bf3<16,1>, wgradn_bf3<8,2> where a split-bf16 kernel exists) and under RCV_F_MFMA_FP32 (the
    fp32-instruction kernels behind every shape the split-bf16 kernels decline).  Bars: 5e-7 of the largest entry of the fp64 result
    on dw and on db.
    Measured (MI355X, largest over the three pairs; dw / db): wgrad_mfma<2,2,2,2,1,f0> 1.13e-7 / 6.1e-8, <2,2,1,2,2,f0> 5.3e-8 / 4.8e-8,
    <1,1,1,1,4,f0> 9.3e-8 / 4.0e-8, <1,1,1,1,4,f5> 7.0e-8 / 2.2e-8, <1,2,1,1,4,f0> 7.6e-8 / 1.7e-8, <2,2,1,1,4,f0> 7.8e-8 / 3.4e-8,
    <2,1,1,1,4,f0> 7.8e-8 / 3.4e-8, <2,2,2,1,2,f0> 5.1e-8 / 2.8e-8; wgrad_bf3<8> 1.32e-7 / 6.1e-8, wgradn_bf3<16,1> 1.35e-7 / 4.0e-8,
    wgradn_bf3<8,2> 1.03e-7 / 2.6e-8."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    N, H, W, Cin, Cout, s, d = shape
    gmode, pmode, flags = RC.WGRAD_RECORD_PAIRS[pair]
    gen = torch.Generator().manual_seed(6000 + H * W + Cout + 7 * d)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    G, P, Pa = _rand(gen, N, H, W, Cin), _rand(gen, N, Ho, Wo, Cout), _rand(gen, N, Ho, Wo, Cout)
    gc, pc = torch.rand(5, Cin, generator=gen) + 0.5, _rand(gen, 5, Cout, scale=0.5)
    if gmode == L.LOAD_AFFINE_RELU:      # shifts of both signs: part of every channel is clamped
        gc[1] = _rand(gen, Cin, scale=0.5)
    if pair == "plain,grad_enc_relu":
        pc = _relu_grad_rows(Cout)
    x64, gy64 = _load_fp64(gmode, G, G, gc, L), _load_fp64(pmode, P, Pa, pc, L)
    ref = torch.nn.grad.conv2d_weight(x64.permute(0, 3, 1, 2), (Cout, Cin, 3, 3), gy64.permute(0, 3, 1, 2), stride=s, padding=d, dilation=d)
    refb = gy64.sum((0, 1, 2))
    Gd, Pd, Pad, gcd, pcd = (v.to(DEV) for v in (G, P, Pa, gc, pc))
    has_bias = bool(flags & L.F_BIAS)
    for matrix_flags in ((0,) if d != 1 else (0, L.F_MFMA_FP32)):
        dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
        db = torch.full((Cout,), float("nan"), device=DEV)
        op = RC.wgrad_record(shape, pair, matrix_flags, p_in=Gd.data_ptr(), p_in_c=gcd.data_ptr(), p_in2=Pd.data_ptr(),
                             p_in2_aux=Pad.data_ptr(), p_in2_c=pcd.data_ptr())
        nb = L.op_workspace(h, op)
        part = torch.zeros(max(nb // 4, 4), device=DEV)
        op.p[L.RCV_P_PART] = part.data_ptr()
        red = L.make_op(L.OP_WGRAD_REDUCE, 0, cin=Cin, cout=Cout, nsplit=op.i[L.RCV_I_NSPLIT], p_part=part.data_ptr(), p_out=dw.data_ptr(),
                        p_bias=db.data_ptr() if has_bias else 0)
        lst = L.OpList([op, red])
        label = lst.labels(h)[0]
        # a split-bf16 kernel exactly where the planner has one for the shape, never under RCV_F_MFMA_FP32, never at dilation 2
        want = RC.wgrad_kernel(shape, matrix_flags)
        assert label.split("<")[0] == want and ("_bf3" in label) == ("_bf3" in want), (label, want)
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        e = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
        eb = float((db.double().cpu() - refb).abs().max() / refb.abs().max()) if has_bias else 0.0
        print(".%s %s %s: max error %.3e (bias %.3e)" % (label, shape, pair, e, eb))
        assert e <= 5e-7 and eb <= 5e-7, (label, e, eb)


@pytest.mark.parametrize("N,H,W,Cin,Cout,s,d", RC.NCHW_WGRAD_SHAPES)
@pytest.mark.parametrize("two", [False, True])
def test_filter_gradient_nchw_image_vs_fp64(N, H, W, Cin, Cout, s, d, two):
    """Filter gradient of a first layer: the gathered operand is the NCHW image itself (RCV_LOAD_NCHW, <= 4 channels) -- the vector-ALU
    first-layer kernel (<= 3 channels into 8), the 2-block folded MFMA tile, and the 16-wide gathered tiles (4 channels, or more than 16
    output channels); the pointwise operand plain or the two-tensor BatchNorm + ReLU backward load."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(3000 + H * W + Cout + Cin)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    G, P = _rand(gen, N, Cin, H, W), _rand(gen, N, Ho, Wo, Cout)
    pc, Pa = _rand(gen, 5, Cout, scale=0.5), _rand(gen, N, Ho, Wo, Cout)
    Gd, Pd, pcd, Pad = (v.to(DEV) for v in (G, P, pc, Pa))
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    mode2 = L.LOAD_GRAD_ENC if two else L.LOAD_PLAIN
    op = RC.nchw_wgrad_record((N, H, W, Cin, Cout, s, d), two, p_in=Gd.data_ptr(), p_in2=Pd.data_ptr(), p_in2_aux=Pad.data_ptr(),
                              p_in2_c=pcd.data_ptr())
    gy64 = _load_fp64(mode2, P, Pa, pc, L)
    nb = L.op_workspace(h, op)
    part = torch.zeros(max(nb // 4, 4), device=DEV)
    op.p[L.RCV_P_PART] = part.data_ptr()
    red = L.make_op(L.OP_WGRAD_REDUCE, 0, cin=Cin, cout=Cout, nsplit=op.i[L.RCV_I_NSPLIT], p_part=part.data_ptr(), p_out=dw.data_ptr(), p_bias=db.data_ptr())
    lst = L.OpList([op, red])
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_weight(G.double(), (Cout, Cin, 3, 3), gy64.permute(0, 3, 1, 2), stride=s, padding=d, dilation=d)
    refb = gy64.sum((0, 1, 2))
    e = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
    eb = float((db.double().cpu() - refb).abs().max() / refb.abs().max())
    print(".%s %s: max error %.3e (bias %.3e)" % (lst.labels(h)[0], (N, H, W, Cin, Cout, s, d, two), e, eb))
    assert e <= 5e-7 and eb <= 5e-7, (lst.labels(h)[0], e, eb)


TCONV_SHAPES = RC.TCONV_SHAPES


@pytest.mark.parametrize("N,H,W,Cin,Cout", TCONV_SHAPES)
@pytest.mark.parametrize("mode_name", ["affine", "grad_enc"] + list(RC.TCONV_RECORD_MODES))
def test_transposed_conv_kernels_vs_fp64(N, H, W, Cin, Cout, mode_name):
    """ConvTranspose2d(k3, s2, p1, output_padding 1) in its three kernel forms (all-parity LDS-DMA tile, merged-parity narrow tile,
    phase-split fallback) -- the forward of the decoder blocks and the data gradient of the stride-2 convs: 3e-6 of the fp64 result.
    Load modes: BatchNorm apply and the BatchNorm + ReLU backward of the U-Net step; RCV_LOAD_GRAD_DEC (the data gradient of
    ConvPoolSimple(..., stride 2): conv -> BatchNorm -> ReLU), RCV_LOAD_AFFINE_RELU and RCV_LOAD_PLAIN (a decoder block behind such a conv,
    behind relu(conv)).  Measured under the three latter modes (MI355X): tconva_dma<1,5,4,1,4> 8.8e-7, tconva_dma<1,5,2,2,4> 6.2e-7,
    tconvms_mfma<4,3,32> 4.8e-7, <4,3,16> 2.6e-7, <2,5,16> 2.2e-7, tconvn_bf3<32,4,3> 2.8e-7, <16,2,5> 1.6e-7."""
    from robocupvision_amd import _lib as L
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT
    h = L.handle(0)
    mode = RC.TCONV_KERNEL_MODES[mode_name]
    gen = torch.Generator().manual_seed(3000 + H * W + Cin)
    x, xa, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, bias = _rand(gen, Cin, Cout, 3, 3, scale=0.1), _rand(gen, Cout)
    ref = F.conv_transpose2d(_load_fp64(mode, x, xa, c, L).permute(0, 3, 1, 2), w.double(), bias.double(), stride=2, padding=1,
                             output_padding=1).permute(0, 2, 3, 1)
    xd, xad, cd, wd, bd = (v.to(DEV) for v in (x, xa, c, w, bias))
    merged = 1 if Cout <= MERGED_TCONV_MAX_COUT else 0
    # merged layout as it is (fp32 kernels) and, where the split-bf16 narrow kernel is built, split into bf16 (layout 4: tconvn_bf3)
    for layout in RC.tconv_layouts(Cin, Cout, MERGED_TCONV_MAX_COUT):
        rp, cp, nfl = _pack_dims(Cin, Cout, layout, merged=bool(merged))
        wp = torch.zeros(nfl, device=DEV)
        job = L.RcvPackJob()
        job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), Cin, Cout
        job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = 0, 0, rp, cp, layout
        table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
        out = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=DEV)
        pack = L.make_op(L.OP_PACK, 0, count=1, aux0=9 * rp * cp, p_in=table.data_ptr())
        tconv = RC.tconv_record((N, H, W, Cin, Cout), mode_name, layout, p_in=xd.data_ptr(), p_in_aux=xad.data_ptr(), p_in_c=cd.data_ptr(),
                                p_w=wp.data_ptr(), p_bias=bd.data_ptr(), p_out=out.data_ptr())
        lst = L.OpList([pack, tconv])
        label = lst.labels(h)[1]
        assert ("_bf3" in label) == (layout == 4), label
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(".%s %s %s: max error %.3e" % (label, (N, H, W, Cin, Cout), mode_name, err))
        assert err <= 3e-6, (label, err)


@pytest.mark.parametrize("N,H,W,C", [(2, 8, 64, 8), (2, 6, 32, 16), (1, 4, 16, 32), (3, 10, 128, 8), (2, 6, 24, 8), (1, 4, 8, 64), (2, 4, 6, 16)])
@pytest.mark.parametrize("affine", [False, True])
def test_maxpool_backward_first_maximum_exact(N, H, W, C, affine):
    """RCV_OP_POOL_BWD: the pooled gradient goes to the FIRST maximum of each 2x2 window (window order (0,0), (0,1), (1,0), (1,1), as
    aten::max_pool2d_with_indices), bit for bit, on inputs full of ties -- through the row-mapped kernel (C/4 a power of two, W*C/4 a
    multiple of 64) and through the pixel-mapped one (the other shapes); with the producer's BatchNorm folded into the comparison
    (positive and negative scales) and a residual added to the result."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    gen = torch.Generator().manual_seed(5 + H * W + C)
    x = torch.randint(-3, 4, (N, H, W, C), generator=gen).float()          # few distinct values: most windows hold ties
    g = _rand(gen, N, H // 2, W // 2, C)
    resid = _rand(gen, N, H, W, C)
    c = torch.zeros(5, C)
    c[0] = torch.where(torch.arange(C) % 3 == 0, -0.5, 2.0) if affine else 1.0
    c[1] = _rand(gen, C) if affine else 0.0
    xv = (x * c[0] + c[1]).permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.max_pool2d(xv, 2, 2)
    y.backward(g.permute(0, 3, 1, 2).double())
    ref = (xv.grad.permute(0, 2, 3, 1) + resid.double()).float()
    xd, gd, rd, cd = x.to(DEV), g.to(DEV), resid.to(DEV), c.to(DEV)
    out = torch.full((N, H, W, C), float("nan"), device=DEV)
    op = L.make_op(L.OP_POOL_BWD, L.F_RESID, n=N, h=H, w=W, cout=C, inmode=L.LOAD_AFFINE if affine else L.LOAD_PLAIN, stats=L.STATS_NONE,
                   p_in=gd.data_ptr(), p_epi_aux=xd.data_ptr(), p_in_c=cd.data_ptr(), p_resid=rd.data_ptr(), p_out=out.data_ptr())
    L.OpList([op]).run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("N,H,W,Cin,Cout,s,d", RC.TINY_CONV_SHAPES)
@pytest.mark.parametrize("mode_name,flags", RC.TINY_CONV_MODES)
def test_tiny_plane_conv_vs_fp64(N, H, W, Cin, Cout, s, d, mode_name, flags):
    """conv_small.hip (inference on planes of a few hundred pixels: LabelProp's dilated convs for one frame pair, model.py:546-548): one
    MFMA block per workgroup, K split over its four waves, operands straight from global memory.  Zero padding applies AFTER the load
    transform (a padded tap contributes 0, not the BatchNorm shift)."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    mode = {"plain": L.LOAD_PLAIN, "affine": L.LOAD_AFFINE, "affine_relu": L.LOAD_AFFINE_RELU}[mode_name]
    gen = torch.Generator().manual_seed(31 + H * W + Cin + Cout)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, c = _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.7)
    w, b = _rand(gen, Cout, Cin, 3, 3, scale=0.1), _rand(gen, Cout)
    X = x.double()
    if mode != L.LOAD_PLAIN:
        X = X * c[0].double() + c[1].double()
    if mode == L.LOAD_AFFINE_RELU:
        X = F.relu(X)
    use_bias, use_relu = bool(flags & 1), bool(flags & 2)
    ref = F.conv2d(X.permute(0, 3, 1, 2), w.double(), b.double() if use_bias else None, stride=s, padding=d, dilation=d).permute(0, 2, 3, 1)
    if use_relu:
        ref = F.relu(ref)
    xd, cd, wd, bd = (v.to(DEV) for v in (x, c, w, b))
    rp, cp = (Cin + 3) // 4 * 4, (Cout + 15) // 16 * 16
    wp = torch.zeros(9 * rp * cp, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), Cout, Cin
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = 1, 0, rp, cp, 0
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
    pack = L.make_op(L.OP_PACK, 0, count=1, aux0=9 * rp * cp, p_in=table.data_ptr())
    conv = RC.tiny_conv_record((N, H, W, Cin, Cout, s, d), mode_name, flags, p_in=xd.data_ptr(), p_in_c=cd.data_ptr(), p_w=wp.data_ptr(),
                               p_bias=bd.data_ptr(), p_out=out.data_ptr())
    lst = L.OpList([pack, conv])
    label = lst.labels(h)[1]
    assert label.startswith("conv_small"), label
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 3e-6, (label, err)


# ------------------------------------------------------------------------------------------ flipped and scaled filters
def _packed_filter(L, wd, D0, D1, rows_from_d1, flip, rp, cp, nfl, layout, scale=None):
    """One RCV_OP_PACK record (a table of one job) for the parameter `wd` on the device; (record, buffers to keep alive)."""
    wp = torch.zeros(nfl, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), D0, D1
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = rows_from_d1, flip, rp, cp, layout
    job.scale = scale.data_ptr() if scale is not None else None
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    return L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr()), wp, table


@pytest.mark.parametrize("shape", RC.DGRAD_SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("mode_name", list(RC.DGRAD_MODES))
def test_stride1_data_gradient_records_vs_fp64(shape, mode_name):
    """The stride-1 data gradient as engine.py bwd_conv emits it: an RCV_OP_CONV record over the layer's OUTPUT channels whose filter
    is the layer's own parameter packed (D0 = cin, D1 = cout, rows_from_d1 = 0, flip = 1) -- the 180-degree-rotated filter, under every
    layout the record can ask for (0, Winograd, split-bf16), at dilation 1 and 2.  Shapes are the record's channels.  Loads:
    RCV_LOAD_GRAD_DEC and RCV_LOAD_GRAD_ENC with random constants, RCV_LOAD_GRAD_ENC with the rows (1, 0, 0); all with the residual.
    Reference: torch.nn.grad.conv2d_input in float64 on the transformed fp32 operands, plus the residual.  Bars 3e-6 (2e-6 Winograd).
    Measured (MI355X, largest over the three loads): dilation 1 conv_dma<1,5,4,1,4> 1.86e-6 (128 -> 64 channels, grad_dec),
    conv_wino<64,80> 4.0e-7, conv_bf3<64,160> 1.07e-6, convs_mfma<2,3,32> 5.0e-7, <1,3,32> 6.1e-7, <1,5,16> 3.4e-7, convn_bf3<32,2,3>
    4.5e-7, <32,1,5> 4.7e-7, <16,1,5> 2.7e-7; dilation 2 conv_dma<1,5,4,1,4> 1.32e-6, conv_mfma<1,5,2,2,8> 7.4e-7, convs_mfma<1,3,32>
    4.8e-7, <1,5,16> 2.9e-7, <1,5,8> 2.7e-7, <2,3,32> 7.0e-8.  By load: grad_dec 1.86e-6, grad_enc 1.04e-6, grad_enc (1, 0, 0) 8.2e-7."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    N, H, W, Cin, Cout, s, d = shape
    mode = RC.DGRAD_MODES[mode_name]
    gen = torch.Generator().manual_seed(6000 + H * W + Cin + 7 * d)
    g, ga, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, resid = _rand(gen, Cin, Cout, 3, 3, scale=0.1), _rand(gen, N, H, W, Cout)       # the layer's parameter: [its Cout][its Cin][3][3]
    if mode_name == "grad_enc_relu":
        c = _relu_grad_rows(Cin)
    ref = torch.nn.grad.conv2d_input((N, Cout, H, W), w.double(), _load_fp64(mode, g, ga, c, L).permute(0, 3, 1, 2).contiguous(), stride=1,
                                     padding=d, dilation=d).permute(0, 2, 3, 1) + resid.double()
    gd, gad, cd, wd, rd = (v.to(DEV) for v in (g, ga, c, w, resid))
    for layout in RC.conv_layouts(Cin, Cout, 1, d):
        rp, cp, nfl = _pack_dims(Cin, Cout, layout)
        pack, wp, table = _packed_filter(L, wd, Cin, Cout, 0, 1, rp, cp, nfl, layout)
        out = torch.full((N, H, W, Cout), float("nan"), device=DEV)
        conv = RC.dgrad_record(shape, mode_name, layout, p_in=gd.data_ptr(), p_in_aux=gad.data_ptr(), p_in_c=cd.data_ptr(), p_w=wp.data_ptr(),
                               p_out=out.data_ptr(), p_resid=rd.data_ptr())
        lst = L.OpList([pack, conv])
        label = lst.labels(h)[1]
        assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout == 3), label
        assert not label.startswith("conv_small"), label
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(".dgrad %s %s %s: max error %.3e" % (label, shape, mode_name, err))
        assert err <= (2e-6 if layout == 2 else 3e-6), (label, err)


@pytest.mark.parametrize("plane", RC.CLS_DGRAD_PLANES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("cout", RC.CLS_DGRAD_COUT)
@pytest.mark.parametrize("n_class", RC.CLS_DGRAD_CLASSES)
def test_classifier_data_gradient_record_vs_fp64(plane, cout, n_class):
    """The 3x3 classifier's data gradient (engine.py bwd_cls): the class gradient in 8 NHWC channels, zero beyond the classes as
    RCV_OP_NCHW_TO_NHWC leaves them, through the parameter [classes][cout][3][3] packed flipped with its 1..8 class rows padded to 8.
    RCV_LOAD_PLAIN, with the residual; 3e-6 of the largest entry.
    Measured (MI355X): convs_mfma<1,5,8> (37 x 53) 2.97e-7, convs_mfma<1,3,8> (9 x 11) 2.69e-7, both at 8 classes; 1.3e-7 at 1 class."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    N, H, W = plane
    gen = torch.Generator().manual_seed(6500 + H * W + cout + n_class)
    g = torch.zeros(N, H, W, 8)
    g[..., :n_class] = _rand(gen, N, H, W, n_class)
    w, resid = _rand(gen, n_class, cout, 3, 3, scale=0.2), _rand(gen, N, H, W, cout)
    ref = torch.nn.grad.conv2d_input((N, cout, H, W), w.double(), g[..., :n_class].double().permute(0, 3, 1, 2).contiguous(), stride=1,
                                     padding=1).permute(0, 2, 3, 1) + resid.double()
    gd, wd, rd = g.to(DEV), w.to(DEV), resid.to(DEV)
    rp, cp = 8, (cout + 15) // 16 * 16
    pack, wp, table = _packed_filter(L, wd, n_class, cout, 0, 1, rp, cp, 9 * rp * cp, 0)
    out = torch.full((N, H, W, cout), float("nan"), device=DEV)
    conv = RC.cls_dgrad_record(plane, cout, p_in=gd.data_ptr(), p_w=wp.data_ptr(), p_out=out.data_ptr(), p_resid=rd.data_ptr())
    lst = L.OpList([pack, conv])
    label = lst.labels(h)[1]
    lst.run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(".cls dgrad %s %s -> %d, %d classes: max error %.3e" % (label, plane, cout, n_class, err))
    assert err <= 3e-6, (label, err)


MULTI_ROUND_PARAMS = [(case, mode_name) for case in RC.MULTI_ROUND_CASES for mode_name in RC.multi_round_modes(case)]


@pytest.mark.parametrize("case,mode_name", MULTI_ROUND_PARAMS,
                         ids=["%s-%s-layout%d-%s" % (c[0], "x".join(map(str, c[1])), c[2], m) for c, m in MULTI_ROUND_PARAMS])
def test_multi_round_records_vs_fp64(case, mode_name):
    """The persistent kernels beyond their first tile round (tests/conv_record_cases.py MULTI_ROUND_CASES): on 256 CUs every workgroup
    of convs_mfma / tconvms_mfma, convn_bf3 / tconvn_bf3 loops over three tiles or more and the last round is ragged (conv_first:
    two rounds) -- the prefetch of the next tile while this one is contracted, the parity of convn_bf3's two staging buffers, the tile
    index of the later rounds, workgroups without a tile in the last round, and the BatchNorm sums carried across the tiles of a
    workgroup.  The condition is re-asserted on the device's own handle: should it no longer hold, the test fails.
    Forward: RCV_LOAD_AFFINE_RELU with the bias and RCV_STATS_FWD (the first layer: RCV_LOAD_NCHW); gradients: RCV_LOAD_GRAD_DEC and
    RCV_LOAD_GRAD_ENC with the residual.  Each record runs plain and with RCV_F_STREAM_OUT forced (the streaming store is a template
    instantiation of its own in these families): outputs and partial rows NaN-prefilled, torch.equal between the two runs, and per
    element against float64 at the bars of the tests above -- 3e-6 of the largest entry, the float64 sum of the partial rows within
    close(rtol=1e-4, floor=1.0).
    Measured (MI355X, largest over the three modes; plain and streaming runs bit-identical): convs_mfma<1,5,8> 2.6e-7, <1,5,16> 3.5e-7,
    <2,3,32> 5.1e-7, <2,2,16> 4.4e-7, <1,3,8> 2.4e-7; convn_bf3<8,1,5> 2.5e-7, <16,1,5> 3.4e-7, <32,2,3> 5.0e-7, <16,2,3> 2.7e-7;
    tconvms_mfma<2,5,16> 2.0e-7, <4,3,32> 3.7e-7; tconvn_bf3<16,2,5> 1.5e-7, <32,4,3> 3.4e-7; conv_first<1> 2.6e-7.  43 cases (14 shapes x 3 loads, the first layer's one), at most
    0.9 s each; the largest tensor is the 48 MB output of the 32 -> 16 transposed conv at 37 x 64 x 80 (tconvms_mfma<4,3,32> needs
    1036 tiles of 192 input pixels for three rounds)."""
    import plan_census as PC
    from robocupvision_amd import _lib as L
    from test_gpu_blocks import close
    h = L.handle(0)
    what, shape, layout, pinned = case
    N, H, W, Cin, Cout, Ho, Wo, s = RC.multi_round_dims(case)
    mode, flags, stats = RC.MULTI_ROUND_MODES[mode_name]
    gen = torch.Generator().manual_seed(8000 + H * W + Cin + 3 * layout)
    x = _rand(gen, N, Cin, H, W) if what == "first" else _rand(gen, N, H, W, Cin)
    xa, c = _rand(gen, *x.shape), _rand(gen, 5, Cin, scale=0.5)
    w = _rand(gen, Cin, Cout, 3, 3, scale=0.1) if what == "tconv" else _rand(gen, Cout, Cin, 3, 3, scale=0.1 if Cin > 4 else 0.2)
    resid, bias = _rand(gen, N, Ho, Wo, Cout), _rand(gen, Cout)
    x64 = x.double() if what == "first" else _load_fp64(mode, x, xa, c, L).permute(0, 3, 1, 2)
    if what == "tconv":
        ref = F.conv_transpose2d(x64, w.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    else:
        ref = F.conv2d(x64, w.double(), stride=s, padding=1).permute(0, 2, 3, 1)
    ref = ref + (resid.double() if flags & L.F_RESID else bias.double())
    ref_rows = torch.stack([ref.sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))])
    xd, xad, cd, wd, rd, bd = (v.to(DEV) for v in (x, xa, c, w, resid, bias))
    if what == "tconv":
        rp, cp, nfl = _pack_dims(Cin, Cout, layout, merged=True)
        pack, wp, table = _packed_filter(L, wd, Cin, Cout, 0, 0, rp, cp, nfl, layout)
    elif what == "first":
        rp, cp = (Cin + 3) // 4 * 4, (Cout + 15) // 16 * 16
        pack, wp, table = _packed_filter(L, wd, Cout, Cin, 1, 0, rp, cp, 9 * rp * cp, 0)
    else:
        rp, cp, nfl = _pack_dims(Cin, Cout, layout)
        pack, wp, table = _packed_filter(L, wd, Cout, Cin, 1, 0, rp, cp, nfl, layout)
    L.OpList([pack]).run(h, torch.cuda.current_stream().cuda_stream)
    got = []
    for stream in (False, True):
        out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
        op = RC.multi_round_record(case, mode_name, stream, p_in=xd.data_ptr(), p_in_aux=xad.data_ptr(), p_in_c=cd.data_ptr(),
                                   p_w=wp.data_ptr(), p_out=out.data_ptr(), p_resid=rd.data_ptr(), p_bias=bd.data_ptr())
        assert L.op_stream_hints(h, op) == (L.F_STREAM_OUT if stream else 0)
        grid, tiles = PC.assert_multi_round(op, h, L.load().rcv_num_cus(h), pinned)
        part = None
        if stats != L.STATS_NONE:
            nbytes = L.op_workspace(h, op)
            assert op.i[L.RCV_I_NPART] == grid and nbytes == grid * 2 * Cout * 4
            part = torch.full((grid, 2, Cout), float("nan"), device=DEV)
            op.p[L.RCV_P_PART] = part.data_ptr()
        lst = L.OpList([op])
        label = lst.labels(h)[0]
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(".%s %s %s%s: %d tiles over %d workgroups, max error %.3e" % (label, shape, mode_name, " streaming" if stream else "", tiles, grid, err))
        assert err <= 3e-6, (label, stream, err)        # (NaN, an unwritten element, fails here as well)
        if part is not None:
            assert not torch.isnan(part).any(), (label, "a workgroup left its partial row unwritten")
            close(part.double().cpu().sum(0), ref_rows, "%s %s %s partial rows" % (label, shape, mode_name), rtol=1e-4, floor=1.0)
        got.append((out, part))
    assert torch.equal(got[0][0], got[1][0]), (label, "the streaming store changes the output")
    assert got[0][1] is None or torch.equal(got[0][1], got[1][1]), (label, "the streaming store changes the partial rows")


def _folded_errors(out, pre, ref):
    """(max error relative to the largest entry; largest per-channel error, each channel relative to ITS largest |pre-ReLU reference|)."""
    dlt = (out.double().cpu() - ref).abs()
    C = ref.shape[-1]
    per_channel = dlt.reshape(-1, C).max(0)[0] / pre.abs().reshape(-1, C).max(0)[0]
    return float(dlt.max() / ref.abs().max()), float(per_channel.max())


def _signed_scale(gen, C):
    """+-[0.25, 4] per output channel: the range over which an eval-mode BatchNorm's gamma / sqrt(var + eps) moves, both signs."""
    return (0.25 + 3.75 * torch.rand(C, generator=gen)) * (torch.randint(0, 2, (C,), generator=gen) * 2 - 1).float()


@pytest.mark.parametrize("case", RC.FOLDED_CONV_CASES, ids=lambda c: "-".join(map(str, c[0])) + "-" + c[1])
def test_folded_inference_records_vs_fp64(case):
    """Inference BatchNorm folding at record level (engine.EVAL_FOLD_BN, fwd_conv): RCV_F_BIAS | RCV_F_RELU on a filter packed with a
    per-output-channel scale in +-[0.25, 4], under every filter layout of the shape; RCV_LOAD_PLAIN, and RCV_LOAD_NCHW on the image
    layer.  Reference: float64 relu(conv(x, w * scale) + bias).  Two criteria: the bar of the unscaled records relative to the tensor's
    largest entry (3e-6, 2e-6 Winograd), and per channel -- the error of channel c relative to the largest |pre-ReLU reference| of
    channel c, so that a small-scale channel cannot hide behind a large one: the worst channel within 1.5 x the same quantity of the
    unscaled record (scale = NULL, same kernel, layout and operands) + 2^-23.
    Measured (MI355X), worst channel scaled / unscaled: conv_dma<1,5,4,1,4> 1.27e-6 / 1.17e-6 (dilation 2: 1.14e-6 / 1.15e-6),
    conv_wino<64,80> 4.2e-7 / 4.6e-7, conv_bf3<64,160> 1.12e-6 / 1.09e-6, convs_mfma<1,5,16> 5.3e-7 / 4.9e-7, convn_bf3<16,1,5> 3.6e-7 /
    4.6e-7, conv_small<1> (stride 2) 2.8e-7 / 2.1e-7, conv2_bf3<64,160> 5.9e-7 / 5.1e-7, conv_first<1> 2.2e-7 / 2.8e-7; relative to the
    largest entry <= 1.19e-6 (conv_dma), 3.5e-7 (conv_wino)."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    shape, load = case
    N, H, W, Cin, Cout, s, d = shape
    gen = torch.Generator().manual_seed(7000 + H * W + Cin + 7 * d)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x = _rand(gen, N, Cin, H, W) if load == "nchw" else _rand(gen, N, H, W, Cin)
    w, bias, scale = _rand(gen, Cout, Cin, 3, 3, scale=0.1), _rand(gen, Cout), _signed_scale(gen, Cout)
    x64 = x.double() if load == "nchw" else x.double().permute(0, 3, 1, 2)
    refs = {}
    for name, w64 in (("scaled", w.double() * scale.double()[:, None, None, None]), ("unscaled", w.double())):
        pre = (F.conv2d(x64, w64, stride=s, padding=d, dilation=d) + bias.double()[None, :, None, None]).permute(0, 2, 3, 1)
        refs[name] = (pre, F.relu(pre))
    xd, wd, bd, sd = (v.to(DEV) for v in (x, w, bias, scale))
    for layout in RC.conv_layouts(Cin, Cout, s, d):
        rp, cp, nfl = _pack_dims(Cin, Cout, layout)
        res = {}
        for name, sc in (("scaled", sd), ("unscaled", None)):
            pack, wp, table = _packed_filter(L, wd, Cout, Cin, 1, 0, rp, cp, nfl, layout, scale=sc)
            out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
            conv = RC.folded_conv_record(shape, load, layout, p_in=xd.data_ptr(), p_w=wp.data_ptr(), p_bias=bd.data_ptr(), p_out=out.data_ptr())
            lst = L.OpList([pack, conv])
            label = lst.labels(h)[1]
            assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout in (3, 5)), label
            lst.run(h, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res[name] = _folded_errors(out, *refs[name])
        print(".folded %s %s %s: max error %.3e (unscaled %.3e); worst channel %.3e (unscaled %.3e)" %
              (label, shape, load, res["scaled"][0], res["unscaled"][0], res["scaled"][1], res["unscaled"][1]))
        assert res["scaled"][0] <= (2e-6 if layout == 2 else 3e-6), (label, res)
        assert res["scaled"][1] <= 1.5 * res["unscaled"][1] + 2.0 ** -23, (label, res)


@pytest.mark.parametrize("shape", RC.FOLDED_TCONV_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_folded_inference_transposed_records_vs_fp64(shape):
    """The folded decoder block (engine.py fwd_up): RCV_F_BIAS | RCV_F_RELU | RCV_F_RESID on a transposed-conv filter packed with a
    per-output-channel scale -- relu(convT(x, w * scale) + bias) + skip in one launch -- in layout 0 or 1 (merged parity) and 4 (its
    split-bf16 form) where test_transposed_conv_kernels_vs_fp64 enumerates it.  The two criteria of
    test_folded_inference_records_vs_fp64, at the bar of the unscaled transposed records (3e-6).
    Measured (MI355X), worst channel scaled / unscaled: tconva_dma<1,5,4,1,4> 8.7e-7 / 1.00e-6 (128 -> 128: 1.08e-6 / 1.70e-6),
    tconvms_mfma<4,3,32> 3.7e-7 / 3.4e-7, <4,3,16> 2.9e-7 / 3.2e-7, tconvn_bf3<32,4,3> 3.0e-7 / 3.7e-7; relative to the largest entry
    <= 8.0e-7."""
    from robocupvision_amd import _lib as L
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT
    h = L.handle(0)
    N, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(7500 + H * W + Cin)
    x, w, bias = _rand(gen, N, H, W, Cin), _rand(gen, Cin, Cout, 3, 3, scale=0.1), _rand(gen, Cout)
    resid, scale = _rand(gen, N, 2 * H, 2 * W, Cout), _signed_scale(gen, Cout)
    refs = {}
    for name, w64 in (("scaled", w.double() * scale.double()[None, :, None, None]), ("unscaled", w.double())):
        pre = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w64, bias.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
        refs[name] = (pre, F.relu(pre) + resid.double())
    xd, wd, bd, rd, sd = (v.to(DEV) for v in (x, w, bias, resid, scale))
    for layout in RC.tconv_layouts(Cin, Cout, MERGED_TCONV_MAX_COUT):
        rp, cp, nfl = _pack_dims(Cin, Cout, layout, merged=layout in (1, 4))
        res = {}
        for name, sc in (("scaled", sd), ("unscaled", None)):
            pack, wp, table = _packed_filter(L, wd, Cin, Cout, 0, 0, rp, cp, nfl, layout, scale=sc)
            out = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=DEV)
            tconv = RC.folded_tconv_record(shape, layout, p_in=xd.data_ptr(), p_w=wp.data_ptr(), p_bias=bd.data_ptr(), p_out=out.data_ptr(),
                                           p_resid=rd.data_ptr())
            lst = L.OpList([pack, tconv])
            label = lst.labels(h)[1]
            assert ("_bf3" in label) == (layout == 4), label
            lst.run(h, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res[name] = _folded_errors(out, *refs[name])
        print(".folded %s %s: max error %.3e (unscaled %.3e); worst channel %.3e (unscaled %.3e)" %
              (label, shape, res["scaled"][0], res["unscaled"][0], res["scaled"][1], res["unscaled"][1]))
        assert res["scaled"][0] <= 3e-6, (label, res)
        assert res["scaled"][1] <= 1.5 * res["unscaled"][1] + 2.0 ** -23, (label, res)


# ------------------------------------------------------------------------------------------ epilogue statistics
def _conv_layouts(Cin, Cout, s):
    """The filter layouts test_conv_kernels_vs_fp64 enumerates for a shape."""
    return RC.conv_layouts(Cin, Cout, s, 1)


def _stats_case_on_device(c, layout, merged, labels, variants=None, randn=False, multi_round=None):
    """Packs the filter of a small_ops_cases conv case in `layout` and runs the record once per statistics variant: the stored
    tensor and the float64 sum of ALL partial rows (NaN-prefilled: an unwritten row shows) must equal the float64 answer exactly --
    or, for random operands (randn), meet the accuracy bar of the tests above resp. close(rtol=1e-4, floor=1.0)."""
    import numpy as np
    import small_ops_cases as K
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    N, H, W, Cin, Cout, Ho, Wo = (c[k] for k in ("N", "H", "W", "Cin", "Cout", "Ho", "Wo"))
    tr = c["transposed"]
    dv = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("x", "c", "w", "bias", "res", "e", "ec")}
    if c["nchw"] or (layout == 0 and not tr and c["d"] != 1) or len(c["shape"]) > 6:
        rp, cp = (Cin + 3) // 4 * 4, (Cout + 15) // 16 * 16
        nfl = 9 * rp * cp
    else:
        rp, cp, nfl = _pack_dims(Cin, Cout, layout, merged=bool(merged))
    wp = torch.zeros(nfl, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = dv["w"].data_ptr(), wp.data_ptr(), (Cin if tr else Cout), (Cout if tr else Cin)
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = (0 if tr else 1), 0, rp, cp, layout
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    pack = L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr())
    for kind, flags in (variants or K.STATS_VARIANTS):
        out = torch.full((N, Ho, Wo, Cout), float("nan"), device=DEV)
        op = RC.stats_record(c, layout, kind, flags, p_in=dv["x"].data_ptr(), p_in_c=dv["c"].data_ptr(), p_w=wp.data_ptr(),
                             p_bias=dv["bias"].data_ptr(), p_resid=dv["res"].data_ptr(), p_epi_aux=dv["e"].data_ptr(),
                             p_epi_c=dv["ec"].data_ptr(), p_out=out.data_ptr())
        if multi_round is not None:       # the guard of a multi-round case: still three rounds, the last ragged, on THIS device
            import plan_census as PC
            PC.assert_multi_round(op, h, L.load().rcv_num_cus(h), multi_round)
        nbytes = L.op_workspace(h, op)
        n_part = op.i[L.RCV_I_NPART]
        assert n_part > 0 and nbytes == n_part * 2 * Cout * 4
        part = torch.full((n_part, 2, Cout), float("nan"), device=DEV)
        op.p[L.RCV_P_PART] = part.data_ptr()
        lst = L.OpList([pack, op])
        label = lst.labels(h)[1]
        if tr:
            assert ("_bf3" in label) == (layout == 4), label
        elif not c["nchw"] and len(c["shape"]) == 6:
            assert label.startswith("conv_wino") == (layout == 2) and ("_bf3" in label) == (layout in (3, 5)), label
        labels.add(label.split("<")[0])
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        v, ref, _ = K.conv_stats_reference(c, kind, flags)
        what = "%s %s layout %d statistics %d flags %d" % (label, c["shape"], layout, kind, flags)
        got = out.double().cpu()
        rows = part.double().cpu().sum(0)
        if randn:
            from test_gpu_blocks import close
            err = float((got - torch.from_numpy(v)).abs().max() / np.abs(v).max())
            print(".%s: max error %.3e" % (what, err))
            assert err <= (2e-6 if layout == 2 else 3e-6), (what, err)
            close(rows, torch.from_numpy(ref), what + " rows", rtol=1e-4, floor=1.0)
            continue
        bad = (got != torch.from_numpy(v)).nonzero()
        assert bad.numel() == 0, "%s: %d stored elements differ, first at %s" % (what, bad.shape[0], bad[0].tolist())
        bad = (rows != torch.from_numpy(ref)).nonzero()
        assert bad.numel() == 0, "%s: %d column sums differ, first (row, channel) %s: got %r, expected %r" % (
            what, bad.shape[0], bad[0].tolist(), float(rows[tuple(bad[0])]), float(ref[tuple(bad[0].tolist())]))


@pytest.mark.parametrize("family", ["conv", "tconv", "image", "tiny", "dilated"])
def test_epilogue_statistics_exact(family):
    """The per-workgroup partial rows of RCV_STATS_FWD (with F_BIAS|F_RELU, without flags, with F_BIAS|F_RESID), RCV_STATS_BWD_ENC and
    RCV_STATS_BWD_DEC (both with F_RESID; p[EPI_C] = (c0, c1, mean), pixels with e*c0 + c1 == 0 masked) of every conv / transposed
    conv kernel family, under every filter layout the accuracy tests above enumerate, on integer-grid operands (tests/small_ops_cases.py:
    activations and sparse filters in {-2..2}, +-2^k scales -- exact through split-bf16 and Winograd), ragged and tiny planes plus one
    per family with several tiles per workgroup.  Labels covered (every tiling the shape lists above reach but those of the two
    640 x 480 planes): conv_dma<1,5,4,1,4>, conv_mfma<1,5,2,2,8>, conv_wino<64,80>, conv_bf3<64,160>, conv2_bf3<64,160>,
    convs_mfma<2,3,32> / <1,5,16> / <1,3,16> / <1,3,8> / <1,5,8> / <2,2,16>, convn_bf3<32,2,3> / <16,1,5> / <8,1,5> / <16,2,3> (conv);
    tconva_dma<1,5,4,1,4> / <1,5,2,2,4>, tconvms_mfma<4,3,32> / <4,3,16> / <2,5,16>, tconvn_bf3<32,4,3> / <16,2,5> (tconv); conv_first<1> /
    <2> (RCV_STATS_FWD without a residual), convs_mfma<1,5,4> / <2,5,4> (NCHW image); the tiny dilated planes leave conv_small, which
    takes no statistics, for conv_dma<1,5,4,1,4>, conv_mfma<1,5,1,2,8> / <1,5,1,2,4>; dilation 2 on NHWC operands (ragged planes, several
    tiles per workgroup, stride 2, a 2 x 2 plane whose off-centre taps all lie in the padding): conv_dma<1,5,4,1,4>,
    conv_mfma<1,5,2,2,8>, convs_mfma<1,5,16> / <1,3,32> / <2,2,16> / <2,3,32> (dilated)."""
    import small_ops_cases as K
    from robocupvision_amd.engine import MERGED_TCONV_MAX_COUT
    labels = set()
    for shape in K.STATS_FAMILIES[family]:
        c = K.build_conv_stats(shape, transposed=family == "tconv", nchw=family == "image")
        for layout, merged in RC.stats_layouts(family, c, MERGED_TCONV_MAX_COUT):
            _stats_case_on_device(c, layout, merged, labels)
    print(".epilogue statistics %s: labels %s" % (family, sorted(labels)))
    expected = dict(conv={"conv_dma", "conv_mfma", "conv_wino", "conv_bf3", "conv2_bf3", "convs_mfma", "convn_bf3"},
                    tconv={"tconva_dma", "tconvms_mfma", "tconvn_bf3"}, image={"conv_first", "convs_mfma"}, tiny={"conv_dma", "conv_mfma"},
                    dilated={"conv_dma", "conv_mfma", "convs_mfma"})[family]
    assert labels == expected, (family, sorted(labels))


@pytest.mark.parametrize("ci", range(12))
def test_epilogue_statistics_randn(ci):
    """Random operands (dense filters), one case per kernel family, every statistics kind: the stored tensor at the bar of the accuracy
    tests above, the float64 sum of the partial rows within close(rtol=1e-4, floor=1.0) of the float64 restatement -- so that the exact
    cases do not hide a rounding-order regression of the partial sums.  The last case is a multi-round one (convn_bf3, 532 tiles over
    256 workgroups): sums carried across the tiles of a workgroup."""
    import small_ops_cases as K
    assert len(K.CONV_RANDN_CASES) == 12
    family, shape, layout, prefix = K.CONV_RANDN_CASES[ci]
    c = K.build_conv_stats(shape, transposed=family == "tconv", nchw=family == "image", randn=True)
    labels = set()
    _stats_case_on_device(c, layout, family == "tconv" and layout in (1, 4), labels, variants=K.randn_variants(prefix), randn=True,
                          multi_round=K.MULTI_ROUND_RANDN_PIN if K.CONV_RANDN_CASES[ci] == K.MULTI_ROUND_RANDN_CASE else None)
    assert labels == {prefix}, labels


@pytest.mark.parametrize("k", range(len(K.MULTI_ROUND_STATS_CASES)))
def test_epilogue_statistics_exact_beyond_the_first_tile_round(k):
    """test_epilogue_statistics_exact on one plane per persistent kernel family (convs_mfma, convn_bf3, tconvms_mfma, tconvn_bf3,
    conv_first) on which a workgroup loops over three tiles or more, the last round ragged (conv_first: two rounds): s1 / s2 stay in
    registers across all tiles of a workgroup, which writes ONE partial row.  Every partial row is exact in fp32
    (tests/test_small_ops.py asserts the bound row by row); the rows are added in float64 and must equal the exact integers."""
    import small_ops_cases as K
    case = K.MULTI_ROUND_STATS_CASES[k]
    c = K.build_conv_stats(case[1], transposed=case[0] == "tconv", nchw=case[0] == "image")
    labels = set()
    _stats_case_on_device(c, case[2], case[0] == "tconv", labels, variants=K.multi_round_stats_variants(case), multi_round=case[3])
    assert labels == {case[3][0].split("<")[0]}, labels
