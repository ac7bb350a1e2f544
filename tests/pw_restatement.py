"""Float64 restatement of the pointwise (1x1) records and of the cross filters (rcv.h RCV_OP_PW, RCV_OP_PW_WGRAD, RCV_OP_CROSS_PACK,
RCV_OP_CROSS_GRAD; csrc/conv_pw.hip), written from the record documentation alone: plain tensor arithmetic, no conv call.  The CPU
tests (tests/test_rest.py) pin it to torch's float64 ``conv2d`` / ``conv_transpose2d``; the GPU tests (tests/test_gpu_pw.py) compare
the kernels with it.  Activations are NHWC [N,H,W,C]; constants are [5,C] rows c0..c4.  pw_reduce restates the summation ORDER of
RCV_OP_PW_WGRAD_REDUCE, for a bitwise comparison."""
import torch

LOAD_PLAIN, LOAD_AFFINE, LOAD_GRAD_ENC, LOAD_GRAD_DEC, LOAD_NCHW, LOAD_AFFINE_RELU = range(6)      # rcv.h RCV_LOAD_*
ZERO = torch.zeros((), dtype=torch.float64)


def load(mode, x, c=None, aux=None):
    """What a kernel sees of an operand (rcv.h RCV_LOAD_*), in float64 from the fp32 operands."""
    X = x.double()
    if mode == LOAD_PLAIN:
        return X
    C = c.double()
    if mode == LOAD_AFFINE:
        return X * C[0] + C[1]
    if mode == LOAD_AFFINE_RELU:
        return torch.clamp_min(X * C[0] + C[1], 0.0)
    A = aux.double()
    if mode == LOAD_GRAD_ENC:
        return torch.where(A > 0, C[0] * X + C[1] + C[2] * A, ZERO)
    if mode == LOAD_GRAD_DEC:
        return C[0] * torch.where(A * C[3] + C[4] > 0, X, ZERO) + C[1] + C[2] * A
    raise ValueError("load mode %r" % (mode,))


def pw_conv(v, w, transposed=False, scale=None, bias=None, relu=False, resid=None, matmul=False):
    """out[n][p][co] = sum_ci v[n][p][ci] * W[co][ci]; ``w`` is the parameter, [Cout][Cin] or with ``transposed`` [Cin][Cout];
    ``scale`` multiplies the filter per output channel; then bias, ReLU, residual, in the epilogue's order.
    ``matmul``: the same sum as one float64 matrix product, for tensors of 10^5 pixels and more, where the [.., Cout, Cin] product of
    the plain form takes gigabytes (tests/test_rest.py: bitwise the plain form on integers, within 1e-12 on randn)."""
    Wm = w.double().reshape(w.shape[0], w.shape[1])
    if transposed:
        Wm = Wm.t()
    if scale is not None:
        Wm = Wm * scale.double()[:, None]
    if matmul:
        out = (v.double().reshape(-1, v.shape[-1]) @ Wm.t()).reshape(*v.shape[:-1], Wm.shape[0])
    else:
        out = (v.double().unsqueeze(-2) * Wm).sum(-1)          # [N,H,W,1,Cin] * [Cout,Cin] -> [N,H,W,Cout]
    if bias is not None:
        out = out + bias.double()
    if relu:
        out = torch.clamp_min(out, 0.0)
    if resid is not None:
        out = out + resid.double()
    return out


def stats_rows(kind, v, e=None, epi_c=None):
    """The two rows a record's partial rows sum to (bn_sums.h): forward (sum v, sum v^2); backward ENC (sum v, sum v (e - mean));
    backward DEC the same of g = (e c0 + c1 > 0 ? v : 0).  kind: 1 / 2 / 3 = rcv.h RCV_STATS_FWD / _BWD_ENC / _BWD_DEC."""
    V = v.double()
    if kind == 1:
        return torch.stack([V.sum((0, 1, 2)), (V * V).sum((0, 1, 2))])
    E, Cc = e.double(), epi_c.double()
    if kind == 3:
        V = torch.where(E * Cc[0] + Cc[1] > 0, V, ZERO)
    return torch.stack([V.sum((0, 1, 2)), (V * (E - Cc[2])).sum((0, 1, 2))])


def pw_wgrad(x_loaded, dy_loaded, matmul=False):
    """dW[co][ci] = sum_p dy[p][co] * x[p][ci].  ``matmul``: as one float64 matrix product (see pw_conv)."""
    X = x_loaded.double().reshape(-1, x_loaded.shape[-1])
    G = dy_loaded.double().reshape(-1, dy_loaded.shape[-1])
    if matmul:
        return G.t() @ X
    return (G.unsqueeze(2) * X.unsqueeze(1)).sum(0)


def order_sensitive_rows(gen, nsplit, *shape):
    """fp32 partial rows [nsplit][*shape] on which the ORDER of a float64 summation shows in the fp32 result.  (On plain randn rows it
    does not: float64 rounds at 2^-53 of the running sum and the final rounding to fp32 hides that.)  Rows are randn; in about a third
    of the places the rows 2m and 2m + 1 hold +B and -B instead, B = randn * 2^40.  The big terms cancel in the end, but while a
    running sum holds one, what is added to it is rounded to about 2^-12: the result, of magnitude sqrt(nsplit), carries the
    summation order in its bits from 2^-12 down, well inside the 24 bits of an fp32 number."""
    part = torch.randn(nsplit, *shape, generator=gen)
    m = nsplit // 2
    if m:
        big = torch.randn(m, *shape, generator=gen) * 2.0 ** 40
        where = torch.rand(m, *shape, generator=gen) < 0.35
        part[0:2 * m:2] = torch.where(where, big, part[0:2 * m:2])
        part[1:2 * m:2] = torch.where(where, -big, part[1:2 * m:2])
    return part


def pw_reduce(part, swap=False):
    """RCV_OP_PW_WGRAD_REDUCE in its documented order: part [nsplit][...] fp32 -> lane l of 16 sums the rows l, l + 16, ... in float64,
    in that order; the 16 lane sums are added in lane order; the total is rounded to fp32 once.  ``swap`` adds rows l + 16 and l of
    every full group of four (l, l + 16, l + 32, l + 48) in the other order: a WRONG order, for the tests to show that their rows
    tell the two apart."""
    ns = part.shape[0]
    P = part.double()
    lanes = []
    for lane in range(16):
        u = torch.zeros(part.shape[1:], dtype=torch.float64)
        order = list(range(lane, ns, 16))
        if swap:
            for k in range(0, len(order) - 3, 4):
                order[k], order[k + 1] = order[k + 1], order[k]
        for s in order:
            u = u + P[s]
        lanes.append(u)
    t = lanes[0]
    for lane in range(1, 16):
        t = t + lanes[lane]
    return t.float()


def cross_pack(a, b, form):
    """Two 1-D filters -> the dense 3x3 filter with a cross of taps (rcv.h RCV_OP_CROSS_PACK).  form 0: a [C/2][Cin][3][1] fills the
    centre column of rows < C/2, b [C/2][Cin][1][3] the centre row of the others.  form 1: a [Cin][C][1][3] fills the centre row,
    b [Cin][C][3][1] the centre column, the centre tap is their sum."""
    if form == 0:
        half = a.shape[0]
        dense = torch.zeros(2 * half, a.shape[1], 3, 3, dtype=a.dtype)
        dense[:half, :, :, 1] = a[:, :, :, 0]
        dense[half:, :, 1, :] = b[:, :, 0, :]
        return dense
    dense = torch.zeros(a.shape[0], a.shape[1], 3, 3, dtype=a.dtype)
    dense[:, :, 1, :] = a[:, :, 0, :]
    dense[:, :, :, 1] += b[:, :, :, 0]
    return dense


def cross_grad(dense, form):
    """The gather that undoes cross_pack on a gradient; form 1 hands the centre tap's gradient to both filters."""
    if form == 0:
        half = dense.shape[0] // 2
        return dense[:half, :, :, 1:2].clone(), dense[half:, :, 1:2, :].clone()
    return dense[:, :, 1:2, :].clone(), dense[:, :, :, 1:2].clone()


def wgrad_rows(P, cin, cout, cus=256):
    """Partial rows of an RCV_OP_PW_WGRAD record (i[NSPLIT]) on a chip of ``cus`` compute units, restated from the launcher's rule: one
    row per chunk of 64 pixels, at most `per_cu` rows per compute unit, where all rows together stay below 8 MiB (1 <= per_cu <= 4)."""
    per_cu = min(max((8 << 20) // (cus * cin * cout * 4), 1), 4)
    return min(-(-P // 64), per_cu * cus)
