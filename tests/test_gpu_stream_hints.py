"""GPU: a streaming hint changes where a cache line lives, never a bit (csrc/stream_hint.h).

One record of every kernel family that honours RCV_F_STREAM_OUT / RCV_F_STREAM_PW -- convs_mfma (gather and merged transposed form),
convn_bf3 (both forms; ragged tiles through the shared epilogue and, at 37 x 53, interior tiles through its own), conv_first, combine
and concat -- is run through the C ABI twice on the same seeded inputs: once with the flag forced, once plain (the shapes are far under
the size threshold, i.e. what RCV_STREAM_MIN_MB=0 does to the large ones).  Outputs and BatchNorm partial rows must be torch.equal.
The shapes are the smallest that still select each family, leave every tile ragged at the plane's border and run the residual and the
two-tensor epilogues.  The families that do not honour the flag (conv_dma, conv_mfma, conv_bf3, conv2_bf3, conv_wino, the filter
gradients) run the same way: the flag is accepted and changes nothing.  Last, one whole small training step (N = 2, 32 x 32) with
every tensor hinted (threshold one byte) and with every hint off: every parameter, gradient, buffer and logit equal."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conv_record_cases as RC      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def _pack(L, wd, D0, D1, rows_from_d1, rows, cols, layout, merged=False):
    from test_gpu_kernels import _pack_dims
    rp, cp, nfl = _pack_dims(rows, cols, layout, merged=merged)
    wp = torch.zeros(nfl, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = wd.data_ptr(), wp.data_ptr(), D0, D1
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = rows_from_d1, 0, rp, cp, layout
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    L.OpList([L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr())]).run(L.handle(0), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return wp


def _run_twice(L, make, out_shape, channels, force):
    """make(**pointer slots) -> record.  Runs it plain and with `force` or-ed into its flags; NaN-prefilled outputs and partial rows."""
    h = L.handle(0)
    got = []
    for flags in (0, force):
        out = torch.full(out_shape, float("nan"), device=DEV)
        op = make(p_out=out.data_ptr())
        op.flags |= flags
        assert L.op_stream_hints(h, op) == flags, (L.op_stream_hints(h, op), flags)
        part = None
        if op.i[L.RCV_I_STATS] != L.STATS_NONE:
            nbytes = L.op_workspace(h, op)
            assert nbytes == op.i[L.RCV_I_NPART] * 2 * channels * 4 > 0
            part = torch.full((op.i[L.RCV_I_NPART], 2, channels), float("nan"), device=DEV)
            op.p[L.RCV_P_PART] = part.data_ptr()
        lst = L.OpList([op])
        label = lst.labels(h)[0]
        lst.run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append((out, part, label))
    (o0, p0, l0), (o1, p1, l1) = got
    assert l0 == l1
    assert not torch.isnan(o0).any(), l0
    assert torch.equal(o0, o1), l0
    if p0 is not None:
        assert not torch.isnan(p0).any() and torch.equal(p0, p1), l0
    return l0


# (shape, filter layout, family the label must name, honours the flag)
CONV_CASES = [
    ((2, 12, 20, 8, 8, 1, 1), 0, "convs_mfma"), ((2, 12, 20, 16, 16, 1, 1), 0, "convs_mfma"), ((2, 16, 24, 8, 16, 2, 1), 0, "convs_mfma"),
    ((2, 12, 20, 32, 32, 1, 1), 0, "convs_mfma"),
    ((2, 12, 20, 8, 8, 1, 1), 3, "convn_bf3"), ((2, 12, 20, 16, 16, 1, 1), 3, "convn_bf3"), ((2, 16, 24, 8, 16, 2, 1), 3, "convn_bf3"),
    ((2, 37, 53, 16, 16, 1, 1), 3, "convn_bf3"),          # tiles inside the plane: the kernel's own epilogue
    # not hinted: the flag is accepted and ignored
    ((2, 8, 16, 32, 64, 2, 1), 0, "conv_dma"), ((2, 8, 16, 32, 64, 2, 1), 5, "conv2_bf3"), ((2, 6, 10, 64, 64, 1, 1), 0, "conv_dma"),
    ((2, 6, 10, 64, 64, 1, 1), 2, "conv_wino"), ((2, 6, 10, 128, 128, 1, 1), 3, "conv_bf3"),
]


@pytest.mark.parametrize("shape,layout,family", CONV_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("mode_name", ["grad_dec", "affine_relu"])
def test_conv_records_are_bitwise_the_same_with_the_hint(shape, layout, family, mode_name):
    """grad_dec: a two-tensor load with the residual epilogue, no statistics; affine_relu: bias and RCV_STATS_FWD partial rows."""
    from robocupvision_amd import _lib as L
    N, H, W, Cin, Cout, s, d = shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    gen = torch.Generator().manual_seed(9100 + H * W + Cin + layout)
    x, xa, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, resid, bias = _rand(gen, Cout, Cin, 3, 3, scale=0.1), _rand(gen, N, Ho, Wo, Cout), _rand(gen, Cout)
    wp = _pack(L, w, Cout, Cin, 1, Cin, Cout, layout)
    make = lambda **kw: RC.conv_record(shape, mode_name, layout, p_in=x.data_ptr(), p_in_aux=xa.data_ptr(), p_in_c=c.data_ptr(),
                                       p_w=wp.data_ptr(), p_resid=resid.data_ptr(), p_bias=bias.data_ptr(), **kw)
    label = _run_twice(L, make, (N, Ho, Wo, Cout), Cout, L.F_STREAM_OUT)
    assert label.split("<")[0] == family, label


@pytest.mark.parametrize("shape,layout,family", [((2, 8, 12, 16, 8), 1, "tconvms_mfma"), ((2, 8, 12, 16, 8), 4, "tconvn_bf3"),
                                                 ((2, 8, 12, 32, 16), 1, "tconvms_mfma"), ((2, 8, 12, 32, 16), 4, "tconvn_bf3"),
                                                 ((2, 4, 8, 64, 32), 1, "tconvm_dma")],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("mode_name", ["grad_dec", "plain"])
def test_transposed_conv_records_are_bitwise_the_same_with_the_hint(shape, layout, family, mode_name):
    """The merged transposed conv (16 -> 8 at 16 x 24 out, 32 -> 16) on both narrow families; 64 -> 32 runs on conv_dma, which ignores the flag."""
    from robocupvision_amd import _lib as L
    N, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(9200 + H * W + Cin + layout)
    x, xa, c = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    w, bias = _rand(gen, Cin, Cout, 3, 3, scale=0.1), _rand(gen, Cout)
    wp = _pack(L, w, Cin, Cout, 0, Cin, Cout, layout, merged=True)
    make = lambda **kw: RC.tconv_record(shape, mode_name, layout, p_in=x.data_ptr(), p_in_aux=xa.data_ptr(), p_in_c=c.data_ptr(),
                                        p_w=wp.data_ptr(), p_bias=bias.data_ptr(), **kw)
    label = _run_twice(L, make, (N, 2 * H, 2 * W, Cout), Cout, L.F_STREAM_OUT)
    assert label.split("<")[0] == family, label


@pytest.mark.parametrize("stats", [False, True])
def test_first_layer_is_bitwise_the_same_with_the_hint(stats):
    """3 -> 8 on the NCHW image at 10 x 12: one ragged 16 x 64 tile per image."""
    from robocupvision_amd import _lib as L
    N, H, W, Cin, Cout = 2, 10, 12, 3, 8
    gen = torch.Generator().manual_seed(9300)
    x, w, b = _rand(gen, N, Cin, H, W), _rand(gen, Cout, Cin, 3, 3, scale=0.2), _rand(gen, Cout)
    wp = _pack(L, w, Cout, Cin, 1, Cin, Cout, 0)
    make = lambda **kw: L.make_op(L.OP_CONV, L.F_BIAS | L.F_RELU, n=N, h=H, w=W, cin=Cin, cout=Cout, ho=H, wo=W, stride=1, dil=1,
                                  inmode=L.LOAD_NCHW, stats=L.STATS_FWD if stats else L.STATS_NONE, p_in=x.data_ptr(), p_w=wp.data_ptr(),
                                  p_bias=b.data_ptr(), **kw)
    assert _run_twice(L, make, (N, H, W, Cout), Cout, L.F_STREAM_OUT) == "conv_first<1>"


@pytest.mark.parametrize("mode2", ["plain", "affine", "affine_relu"])
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("force", ["out", "pw", "both"])
def test_combine_is_bitwise_the_same_with_the_hints(mode2, concat, force):
    """relu(t*c0+c1) + f(r) with each skip load mode, and the concat form; 2 x 12 x 20 x 8: the last workgroup is ragged."""
    from robocupvision_amd import _lib as L
    N, H, W, Cc = 2, 12, 20, 8
    gen = torch.Generator().manual_seed(9400)
    t, r, tc, rc = _rand(gen, N, H, W, Cc), _rand(gen, N, H, W, Cc), _rand(gen, 5, Cc, scale=0.5), _rand(gen, 5, Cc, scale=0.5)
    m2 = {"plain": L.LOAD_PLAIN, "affine": L.LOAD_AFFINE, "affine_relu": L.LOAD_AFFINE_RELU}[mode2]
    make = lambda **kw: L.make_op(L.OP_COMBINE, L.F_CONCAT if concat else 0, n=N, h=H, w=W, cout=Cc, inmode2=m2, p_in=t.data_ptr(),
                                  p_in_c=tc.data_ptr(), p_in2=r.data_ptr(), p_in2_c=rc.data_ptr(), **kw)
    bits = {"out": L.F_STREAM_OUT, "pw": L.F_STREAM_PW, "both": L.F_STREAM_OUT | L.F_STREAM_PW}[force]
    _run_twice(L, make, (N, H, W, Cc * (2 if concat else 1)), Cc, bits)


@pytest.mark.parametrize("shape,pair", [((2, 12, 20, 8, 8, 1, 1), "affine_relu,grad_dec"), ((2, 12, 20, 16, 16, 1, 1), "plain,grad_enc_relu"),
                                        ((2, 6, 10, 64, 64, 1, 1), "affine,grad_dec"), ((2, 8, 16, 32, 64, 2, 1), "affine,grad_dec")],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_filter_gradient_records_accept_the_flag(shape, pair):
    """No filter-gradient family honours RCV_F_STREAM_PW yet: the flag is accepted, reported by the query, and the partial filters
    (with and without the second tensor of the pointwise load, with and without the bias sums) are what they were."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    N, H, W, Cin, Cout, s, d = shape
    Hp, Wp = (H - 1) // s + 1, (W - 1) // s + 1
    gen = torch.Generator().manual_seed(9500 + Cin)
    g, ga, gc = _rand(gen, N, H, W, Cin), _rand(gen, N, H, W, Cin), _rand(gen, 5, Cin, scale=0.5)
    p, pa, pc = _rand(gen, N, Hp, Wp, Cout), _rand(gen, N, Hp, Wp, Cout), _rand(gen, 5, Cout, scale=0.5)
    parts = []
    for flags in (0, L.F_STREAM_PW):
        op = RC.wgrad_record(shape, pair, flags, p_in=g.data_ptr(), p_in_aux=ga.data_ptr(), p_in_c=gc.data_ptr(), p_in2=p.data_ptr(),
                             p_in2_aux=pa.data_ptr(), p_in2_c=pc.data_ptr())
        assert L.op_stream_hints(h, op) == flags
        nbytes = L.op_workspace(h, op)
        part = torch.full((nbytes // 4,), float("nan"), device=DEV)
        op.p[L.RCV_P_PART] = part.data_ptr()
        L.OpList([op]).run(h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        parts.append(part)
    assert torch.equal(torch.nan_to_num(parts[0], nan=-7.0), torch.nan_to_num(parts[1], nan=-7.0))
    assert not torch.isnan(parts[0]).all()


def test_whole_step_is_bitwise_the_same_with_every_hint_on_and_off():
    """Two Trainer steps of ROBO-UNet at 2 x 32 x 32 from the same seed, once with the handle's threshold at one byte (every record
    hinted) and once at 0 (every hint off): logits, parameters, gradients and buffers equal."""
    import robocupvision_amd.model as M
    from oracle import cpu_reference as O
    from robocupvision_amd import _lib as L
    from robocupvision_amd.train import Trainer
    lib, h = L.load(), L.handle(0)
    x, t = O.synthetic_batch(2, 32, 32, seed=11)
    x, t = x.to(DEV), t.to(DEV)
    big = L.make_op(L.OP_CONV, 0, n=2, h=32, w=32, cin=8, cout=8, ho=32, wo=32, stride=1, dil=1, inmode=L.LOAD_AFFINE, stats=L.STATS_FWD)
    runs = []
    try:
        for mb, want in ((1e-9, L.F_STREAM_OUT), (0.0, 0)):
            L.check(lib.rcv_set_stream_min_mb(h, mb), "rcv_set_stream_min_mb")
            assert L.op_stream_hints(h, big) == want
            torch.manual_seed(12345678)
            model = M.ROBO_UNet().to(DEV)
            tr = Trainer(model, class_weights=[1, 10, 30, 10, 2], lr=1e-3, decay=1e-6)
            for _ in range(2):
                pred = tr.step(x, t)
            torch.cuda.synchronize()
            state = {"logits": pred.detach().clone()}
            for k, p in model.named_parameters():
                state["param." + k] = p.detach().clone()
                if p.grad is not None:
                    state["grad." + k] = p.grad.detach().clone()
            for k, v in model.named_buffers():
                state["buffer." + k] = v.detach().clone()
            runs.append(state)
    finally:
        L.check(lib.rcv_set_stream_min_mb(h, float(os.environ.get("RCV_STREAM_MIN_MB", "128"))), "rcv_set_stream_min_mb")
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 40
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
