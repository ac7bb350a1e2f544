"""The filter packer (RCV_OP_PACK, struct rcv_pack_job of include/rcv.h) restated in numpy, and the way the conv / transposed-conv
kernels read a packed filter -- no device, no library.

pack()          src [D0][D1][3][3] -> the packed filter of layouts 0 (nine taps), 1 (merged parity), 2 (Winograd G g G^T) and 3 / 4 / 5
                (split-bf16), with the flip (tap t reads source tap 8 - t) and the per-output-channel scale of the job.
unpack_apply()  a packed filter applied to an NHWC float64 tensor: what a kernel that reads this layout computes, in exact arithmetic.
pack_dims()     rows_pad, cols_pad and the number of floats, as engine._Lowering.add_pack sizes a job.

dtype = float64 is the contract (src * scale carried without rounding: the split layouts then keep the float64 remainder in the third
plane, so that h + m + l is the product itself); dtype = float32 is the device's number format (one fp32 rounding of the product, three
bf16 values that hold it exactly, every plane returned as float32).

tests/test_pack.py compares unpack_apply(pack()) with the torch operations; tests/test_gpu_pack.py compares the device's packer with
pack(), and tests/test_gpu_kernels.py runs the records behind the flip and scale branches against float64."""
import numpy as np

# (record, rows_from_d1, flip, layouts, scaled too) -- the combinations engine.py emits (fwd_conv / fwd_up / bwd_conv / bwd_up / the
# 3x3 classifier); the first three names are those of the torch operation the packed filter stands for
COMBINATIONS = [
    ("conv", 1, 0, (0, 2, 3, 5), True),                 # conv forward: F.conv2d
    ("tconv", 0, 0, (0, 1, 4), True),                   # transposed forward, and the stride-2 data gradient: F.conv_transpose2d
    ("dgrad", 0, 1, (0, 2, 3), False),                  # stride-1 data gradient: torch.nn.grad.conv2d_input
    ("tconv_dgrad", 1, 0, (0, 3, 5), False),            # the transposed conv's data gradient: a stride-2 conv
    ("cls_dgrad", 0, 1, (0,), False),                   # 3x3 classifier data gradient: 1..8 class rows padded to 8
]
# (D0, D1) of the parameter tensor
CHANNEL_PAIRS = [(64, 64), (128, 64), (32, 64), (16, 16), (8, 16), (32, 16), (24, 40), (4, 12), (3, 8), (5, 16)]
CLS_ROWS_PAD = 8


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 -> nearest bfloat16 (ties to even), returned as float32 (what v_cvt_pk_bf16_f32 does for finite inputs)."""
    u = np.asarray(x).astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    h = bf16_rne(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_rne(r1)
    r2 = (r1 - m).astype(np.float32)
    return h, m, bf16_rne(r2), r1, r2


_bf16_rne, _split3 = bf16_rne, split3       # (the names tests/test_split_bf16.py has always used)


def pack_dims(rows, cols, layout, merged=False):
    """rows_pad, cols_pad, floats of the packed filter (engine._Lowering.add_pack)."""
    merged = bool(merged) or layout in (1, 4)
    split = layout in (3, 4, 5)
    if layout == 5:
        rp = -(-rows // 16) * 16
    elif split:
        rp = -(-rows // 32) * 32 if rows > 32 else -(-rows // 8) * 8
    else:
        rp = -(-rows // 4) * 4
    cp = -(-(cols * (4 if merged else 1)) // 16) * 16
    taps = 16 if layout == 2 else (4 if merged else 9)
    ksteps = (rp // 16) * 5 if layout == 5 else (taps * rp + 31) // 32
    return rp, cp, (3 * ksteps * cp * 16 if split else taps * rp * cp)


def _ksteps(layout, rows_pad):
    return (rows_pad // 16) * 5 if layout == 5 else ((4 if layout == 4 else 9) * rows_pad + 31) // 32


def _k_index(layout, taps, rows_pad):
    """(k-step, position inside the step) of (tap, row) in a split layout, each [taps][rows_pad]."""
    t, row = np.meshgrid(np.arange(taps), np.arange(rows_pad), indexing="ij")
    if layout == 5:         # 16-row chunks: k = tap * 16 + row % 16 inside chunk row / 16, five k-steps per chunk
        kk = t * 16 + (row & 15)
        return (row >> 4) * 5 + (kk >> 5), kk & 31
    kk = t * rows_pad + row
    return kk >> 5, kk & 31


G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _parity_tap(ph, t):
    """Source tap of parity phase ph = (py, px) and window tap t = (dy, dx) of the merged layout, or -1: output row 2y + py takes input
    row y + dy through filter row ky -- py = 0: (dy 0, ky 1); py = 1: (dy 0, ky 2), (dy 1, ky 0)."""
    py, px, dy, dx = ph >> 1, ph & 1, t >> 1, t & 1
    ky = (0 if dy else 2) if py else (-1 if dy else 1)
    kx = (0 if dx else 2) if px else (-1 if dx else 1)
    return ky * 3 + kx if ky >= 0 and kx >= 0 else -1


def pack(src, D0, D1, rows_from_d1, flip, rows_pad, cols_pad, layout, scale=None, dtype=np.float64):
    """Layouts 0 / 1 / 2: [9 | 4 | 16][rows_pad][cols_pad] of dtype.  Layouts 3 / 4 / 5: [3 planes][k-steps][cols_pad][32]."""
    src = np.asarray(src).reshape(D0, D1, 9)
    rows, cols = (D1, D0) if rows_from_d1 else (D0, D1)
    g = (src.transpose(1, 0, 2) if rows_from_d1 else src).astype(dtype)          # [row][col][tap]
    if scale is not None:
        g = (g * np.asarray(scale).astype(dtype)[None, :cols, None]).astype(dtype)
    par = layout in (1, 4)
    if flip and not par:
        g = g[:, :, ::-1]
    if layout == 2:
        g33 = g.reshape(rows, cols, 3, 3)
        half = dtype(0.5)

        def transform(a, axis):           # the rows of G along `axis`, in the kernel's order of operations
            g0, g1, g2 = (np.take(a, i, axis=axis) for i in range(3))
            return np.stack([g0, half * (g0 + g1 + g2), half * (g0 - g1 + g2), g2], axis=axis).astype(dtype)

        U = transform(transform(g33, 2), 3)                                     # [row][col][a][b]
        out = np.zeros((16, rows_pad, cols_pad), dtype)
        out[:, :rows, :cols] = U.transpose(2, 3, 0, 1).reshape(16, rows, cols)
        return out
    if par:
        V = np.zeros((4, rows_pad, cols_pad), dtype)
        for t in range(4):
            for ph in range(4):
                ts = _parity_tap(ph, t)
                if ts >= 0:
                    V[t, :rows, ph * cols:(ph + 1) * cols] = g[:, :, ts]
    else:
        V = np.zeros((9, rows_pad, cols_pad), dtype)
        V[:, :rows, :cols] = g.transpose(2, 0, 1)
    if layout in (0, 1):
        return V
    if dtype == np.float32:
        h, m, l, _, _ = split3(V)
    else:                                 # the contract: h + m + l IS the value (both differences are exact in float64)
        h = bf16_rne(V.astype(np.float32)).astype(np.float64)
        m = bf16_rne((V - h).astype(np.float32)).astype(np.float64)
        l = (V - h) - m
    taps = V.shape[0]
    ks, kp = _k_index(layout, taps, rows_pad)
    planes = np.zeros((3, _ksteps(layout, rows_pad), cols_pad, 32), dtype)
    for p, v in enumerate((h, m, l)):
        planes[p][ks[:, :, None], np.arange(cols_pad)[None, None, :], kp[:, :, None]] = v
    return planes


def decode_split(planes, layout, rows_pad, cols_pad):
    """h + m + l of a split layout, in float64, back as [9 | 4 taps][rows_pad][cols_pad] through the k-index map."""
    taps = 4 if layout == 4 else 9
    ks, kp = _k_index(layout, taps, rows_pad)
    s = np.asarray(planes, dtype=np.float64).sum(0)
    return s[ks[:, :, None], np.arange(cols_pad)[None, None, :], kp[:, :, None]]


def unpack_apply(P, x, rows, cols, rows_pad, cols_pad, layout, op, stride=1, dilation=1):
    """The packed filter P (pack()) applied to x, NHWC float64 [N][H][W][rows], the way the kernels read it; NHWC [..][cols].
    op "conv": 3x3, padding = dilation, the given stride (layouts 0, 2, 3, 5); op "tconv": k3 s2 p1 output_padding 1 (layouts 0, 1, 4).
    Layout 0: out = sum_t sum_row x[tap t][row] * P[t][row][col]; merged layouts: four parity phases from a 2x2 window; Winograd:
    F(2x2,3x3) input and output transforms around sixteen per-position products; split layouts: h + m + l decoded first."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, _ = x.shape
    if layout in (3, 4, 5):
        P = decode_split(P, layout, rows_pad, cols_pad)
    P = np.asarray(P, dtype=np.float64)
    assert P.shape[1:] == (rows_pad, cols_pad)
    if layout == 2:
        assert op == "conv" and stride == 1 and dilation == 1
        Hp, Wp = (H + 1) // 2 * 2, (W + 1) // 2 * 2
        xp = np.zeros((N, Hp + 2, Wp + 2, rows))
        xp[:, 1:H + 1, 1:W + 1] = x
        d = np.stack([np.stack([xp[:, a:a + Hp:2, b:b + Wp:2] for b in range(4)], axis=3) for a in range(4)], axis=3)   # [n][ty][tx][a][b][row]
        v = np.einsum("ia,nyxabr,jb->nyxijr", BT, d, BT)
        U = P[:, :rows, :cols].reshape(4, 4, rows, cols)
        m = np.einsum("nyxijr,ijrc->nyxijc", v, U)
        y = np.einsum("pi,nyxijc,qj->nyxpqc", AT, m, AT)
        return y.transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, cols)[:, :H, :W]
    if layout in (1, 4):
        assert op == "tconv"
        xp = np.zeros((N, H + 1, W + 1, rows))
        xp[:, :H, :W] = x
        out = np.zeros((N, 2 * H, 2 * W, cols))
        for ph in range(4):
            for t in range(4):
                out[:, ph >> 1::2, ph & 1::2] += xp[:, t >> 1:(t >> 1) + H, t & 1:(t & 1) + W] @ P[t, :rows, ph * cols:(ph + 1) * cols]
        return out
    if op == "tconv":             # output row 2 iy - 1 + ky takes input row iy through filter row ky
        buf = np.zeros((N, 2 * H + 1, 2 * W + 1, cols))
        for t in range(9):
            ky, kx = divmod(t, 3)
            buf[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += x @ P[t, :rows, :cols]
        return buf[:, 1:, 1:]
    assert op == "conv"
    s, dl = stride, dilation
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    xp = np.zeros((N, H + 2 * dl, W + 2 * dl, rows))
    xp[:, dl:dl + H, dl:dl + W] = x
    out = np.zeros((N, Ho, Wo, cols))
    for t in range(9):
        ty, tx = divmod(t, 3)
        out += xp[:, ty * dl:ty * dl + (Ho - 1) * s + 1:s, tx * dl:tx * dl + (Wo - 1) * s + 1:s] @ P[t, :rows, :cols]
    return out
