"""Float64 restatement of the 5x5 classifier records (include/rcv.h RCV_OP_PACK5 / _CONV5 / _WGRAD5 / _WGRAD5_REDUCE; csrc/conv5.hip),
written from the record descriptions: explicit taps over a zero-padded plane, no convolution routine.  tests/test_cls5_plan.py pins
every function here to torch.nn.functional.conv2d and its autograd in float64 on the CPU (wgrad5_reduce, the reduction's summation
order: tests/test_rest.py); tests/test_gpu_cls5.py compares the kernels with it."""
import torch

TAPS, COLS, CB = 25, 16, 8      # taps, columns of a packed filter, padded class channels (engine.CLS3_PAD)
LOAD_PLAIN, LOAD_AFFINE, LOAD_AFFINE_RELU = 0, 1, 5
STATS_NONE, STATS_BWD_ENC, STATS_BWD_DEC = 0, 2, 3


def load(mode, x, c=None):
    """RCV_LOAD_*: x NHWC, c = the constant rows [5][C]."""
    X = x.double()
    if mode == LOAD_AFFINE:
        return X * c[0].double() + c[1].double()
    if mode == LOAD_AFFINE_RELU:
        return torch.clamp_min(X * c[0].double() + c[1].double(), 0.0)
    assert mode == LOAD_PLAIN
    return X


def pack5(w, flip):
    """w [COUT][CIN][5][5] -> [25][rows][16], zero padded.  Forward: rows = CIN, out[t][ci][co] = w[co][ci][t]; flip (the data
    gradient's filter): rows = 8, out[t][co][ci] = w[co][ci][24 - t]."""
    Cout, Cin = w.shape[0], w.shape[1]
    wt = w.double().reshape(Cout, Cin, TAPS)
    out = torch.zeros(TAPS, CB if flip else Cin, COLS, dtype=torch.float64)
    for t in range(TAPS):
        if flip:
            out[t, :Cout, :Cin] = wt[:, :, TAPS - 1 - t]
        else:
            out[t, :Cin, :Cout] = wt[:, :, t].t()
    return out


def _padded(v):
    N, H, W, C = v.shape
    p = torch.zeros(N, H + 4, W + 4, C, dtype=torch.float64)
    p[:, 2:H + 2, 2:W + 2] = v
    return p


def conv5(v, packed, cout, bias=None, resid=None):
    """RCV_OP_CONV5 on the loaded operand v (NHWC, float64): out[n][y][x][co] = sum_t sum_r v[n][y + t // 5 - 2][x + t % 5 - 2][r] *
    packed[t][r][co] (+ bias[co]) (+ resid), taps outside the plane are zero."""
    N, H, W, _ = v.shape
    p = _padded(v)
    out = torch.zeros(N, H, W, cout, dtype=torch.float64)
    for t in range(TAPS):
        dy, dx = divmod(t, 5)
        out += p[:, dy:dy + H, dx:dx + W] @ packed[t][:, :cout]
    if bias is not None:
        out = out + bias.double()
    if resid is not None:
        out = out + resid.double()
    return out


def wgrad5(v, g):
    """RCV_OP_WGRAD5 + RCV_OP_WGRAD5_REDUCE: v = loaded conv input NHWC [..][CIN], g = output gradient NHWC [..][8] ->
    dW [8][CIN][5][5] (the reduction keeps the first COUT rows), db [8]."""
    N, H, W, Cin = v.shape
    p, G = _padded(v), g.double()
    dw = torch.zeros(CB, Cin, 5, 5, dtype=torch.float64)
    for t in range(TAPS):
        dy, dx = divmod(t, 5)
        dw[:, :, dy, dx] = torch.einsum("nyxo,nyxi->oi", G, p[:, dy:dy + H, dx:dx + W])
    return dw, G.sum((0, 1, 2))


def wgrad5_reduce(part, cin, classes):
    """RCV_OP_WGRAD5_REDUCE in its documented order: part [nsplit][25 * 8 * 16 + 8] fp32, a row = the filter part [tap][class][16
    columns, the first CIN used] then the bias part [8]; rows 0, 1, ... are added in float64 in that order and the sum is rounded to
    fp32 once -> dW [classes][CIN][5][5], db [classes]."""
    u = torch.zeros(part.shape[1], dtype=torch.float64)
    for s in range(part.shape[0]):
        u = u + part[s].double()
    u = u.float()
    dw = u[:TAPS * CB * COLS].reshape(TAPS, CB, COLS)[:, :classes, :cin].permute(1, 2, 0).reshape(classes, cin, 5, 5).contiguous()
    return dw, u[TAPS * CB * COLS:TAPS * CB * COLS + classes].clone()


def stats_rows(kind, out, e, epi_c):
    """The two statistics rows of a data-gradient writer summed over all partial rows: BWD_ENC (sum g, sum g (e - mean)); BWD_DEC the same
    with g masked by e * c0 + c1 > 0.  epi_c = [3][C]: c0, c1, mean."""
    E, C = e.double(), epi_c.double()
    g = out
    if kind == STATS_BWD_DEC:
        g = torch.where(E * C[0] + C[1] > 0, out, torch.zeros((), dtype=torch.float64))
    return torch.stack([g.sum((0, 1, 2)), (g * (E - C[2])).sum((0, 1, 2))])
