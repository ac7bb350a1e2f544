"""The contract of RCV_OP_FARNEBACK / RCV_OP_REMAP_LABELS (csrc/flow.hip) restated in numpy: Farnebäck's 2003 dense optical
flow with the parameter meanings of cv2.calcOpticalFlowFarneback (flags = 0, pyr_scale = 0.5), the label remap of transform.py:189-198 and
the propagation loop of test.py:135-140.  ``dtype`` = numpy.float64 is the contract; numpy.float32 runs the same operations in the device's
number format and is the yardstick for rounding.  Every constant (filter taps, the inverse normal matrix, resize ratios) is formed in
double and rounded to ``dtype`` once, as the library's host code does.

Conventions: planes are [H, W]; flow is [2, H, W], channel 0 = dx (columns), channel 1 = dy (rows); q(x) = p(x - d) gives flow +d."""
import numpy as np

BORDER_W = (0.14, 0.14, 0.4472, 0.4472, 0.4472)      # the weight of a pixel 0..4 pixels from an edge; 1 beyond
MIN_SIZE = 32                                        # no plane is smaller than this on either axis


# ---------------------------------------------------------------------------------------------------------------------------------
# planes
def n_coarse(H, W, levels):
    """How many planes below full resolution the flow is computed on."""
    k, s = 0, 1.0
    while k < levels:
        s *= 0.5
        if W * s < MIN_SIZE or H * s < MIN_SIZE:
            break
        k += 1
    return k


def plane_size(H, W, j):
    s = 0.5 ** j
    return int(np.round(H * s)), int(np.round(W * s))      # numpy rounds half to even


def blur_taps(j):
    """The separable kernel plane j's image is blurred with (double)."""
    sigma = (1.0 / 0.5 ** j - 1.0) / 2.0
    if sigma <= 0:
        return np.array([0.25, 0.5, 0.25])
    n = max(int(np.round(5.0 * sigma)) | 1, 3)
    x = np.arange(n) - (n - 1) / 2.0
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return k / k.sum()


def correlate(a, taps, axis, mode, dtype):
    """out[i] = sum_t taps[t] * a[i + t - r] along `axis`, taps summed in order t = 0, 1, ...; mode 'reflect' (101) or 'edge'."""
    taps = np.asarray(taps, dtype=np.float64).astype(dtype)
    r = (len(taps) - 1) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    ap = np.pad(a.astype(dtype), pad, mode=mode)
    n = a.shape[axis]
    out = np.zeros(a.shape, dtype=dtype)
    for t in range(len(taps)):
        out += taps[t] * np.take(ap, np.arange(t, t + n), axis=axis)
    return out


def _resize_axis(a, n_dst, axis, dtype):
    n_src = a.shape[axis]
    src = (np.arange(n_dst).astype(dtype) + dtype(0.5)) * dtype(n_src / n_dst) - dtype(0.5)
    i0 = np.floor(src)
    f = (src - i0).astype(dtype)
    i0 = i0.astype(np.int64)
    lo, hi = np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1)
    shape = [1] * a.ndim
    shape[axis] = n_dst
    f = f.reshape(shape)
    return np.take(a, lo, axis=axis) * (dtype(1) - f) + np.take(a, hi, axis=axis) * f


def resize(a, h, w, dtype):
    """Bilinear with pixel centres, indices clamped; columns first, then rows.  a: [..., H, W]."""
    a = a.astype(dtype)
    return _resize_axis(_resize_axis(a, w, a.ndim - 1, dtype), h, a.ndim - 2, dtype)


def plane_image(gray, j, dtype):
    H, W = gray.shape
    taps = blur_taps(j)
    b = correlate(correlate(gray.astype(dtype), taps, 1, "reflect", dtype), taps, 0, "reflect", dtype)
    h, w = plane_size(H, W, j)
    return resize(b, h, w, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# polynomial expansion
def poly_taps(n, sigma):
    """g, i*g, i*i*g for i = -n..n (double), g normalised to sum 1."""
    i = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-i * i / (2.0 * sigma * sigma))
    g /= g.sum()
    return g, i * g, i * i * g


def normal_matrix(n, sigma):
    """The 6x6 matrix of the weighted fit over the basis (1, i, j, i^2, j^2, ij), weights g(i) g(j) (double)."""
    g = poly_taps(n, sigma)[0]
    i = np.arange(-n, n + 1, dtype=np.float64)
    jj, ii = np.meshgrid(i, i, indexing="ij")         # jj: rows (y), ii: columns (x)
    w = np.outer(g, g)
    phi = np.stack([np.ones_like(ii), ii, jj, ii * ii, jj * jj, ii * jj])
    return np.einsum("ayx,byx,yx->ab", phi, phi, w)


def poly_exp(img, n, sigma, dtype):
    """R[5, H, W] = (b_x, b_y, a_xx, a_yy, a_xy) of the fit at every pixel; replicated borders; vertical pass, then horizontal."""
    g, xg, xxg = poly_taps(n, sigma)
    gi = np.linalg.inv(normal_matrix(n, sigma)).astype(dtype)
    img = img.astype(dtype)
    v0, v1, v2 = (correlate(img, t, 0, "edge", dtype) for t in (g, xg, xxg))
    m1 = correlate(v0, g, 1, "edge", dtype)
    mx = correlate(v0, xg, 1, "edge", dtype)
    my = correlate(v1, g, 1, "edge", dtype)
    mxx = correlate(v0, xxg, 1, "edge", dtype)
    myy = correlate(v2, g, 1, "edge", dtype)
    mxy = correlate(v1, xg, 1, "edge", dtype)
    # the other entries of rows 1..5 of the inverse are zero: odd moments of a symmetric weight vanish
    return np.stack([gi[1, 1] * mx, gi[2, 2] * my, gi[3, 0] * m1 + gi[3, 3] * mxx + gi[3, 4] * myy,
                     gi[4, 0] * m1 + gi[4, 3] * mxx + gi[4, 4] * myy, gi[5, 5] * mxy])


# ---------------------------------------------------------------------------------------------------------------------------------
# matrices, update
def warp(R1, fx, fy, dtype):
    """Bilinear sample of R1[C, H, W] at (fx, fy) [H, W] and the in-bounds mask (0 <= floor(fx) < W-1, 0 <= floor(fy) < H-1)."""
    H, W = R1.shape[1:]
    x1, y1 = np.floor(fx), np.floor(fy)
    ok = (x1 >= 0) & (x1 < W - 1) & (y1 >= 0) & (y1 < H - 1)
    a, b = (fx - x1).astype(dtype), (fy - y1).astype(dtype)
    xi, yi = np.where(ok, x1, 0).astype(np.int64), np.where(ok, y1, 0).astype(np.int64)
    one = dtype(1)
    top = R1[:, yi, xi] * (one - a) + R1[:, yi, xi + 1] * a
    bot = R1[:, yi + 1, xi] * (one - a) + R1[:, yi + 1, xi + 1] * a
    return top * (one - b) + bot * b, ok


def border_scale(H, W, dtype):
    def axis(n):
        d = np.arange(n)
        w = np.array(BORDER_W + (1.0,), dtype=np.float64).astype(dtype)
        return w[np.minimum(d, 5)] * w[np.minimum(n - 1 - d, 5)]
    wy, wx = axis(H), axis(W)
    # (w[x] * w[W-1-x]) * (w[y] * w[H-1-y])
    return (wx[None, :] * wy[:, None]).astype(dtype)


def matrices(R0, R1, flow, dtype, stats=None):
    """M[5, H, W] from the two expansions and the current flow.  stats["oob"] counts the pixels whose warp left the plane."""
    H, W = R0.shape[1:]
    dx, dy = flow[0].astype(dtype), flow[1].astype(dtype)
    ys, xs = np.meshgrid(np.arange(H).astype(dtype), np.arange(W).astype(dtype), indexing="ij")
    Rw, ok = warp(R1, xs + dx, ys + dy, dtype)
    if stats is not None:
        stats["oob"] = stats.get("oob", 0) + int((~ok).sum())
    own = np.concatenate([np.zeros_like(R0[:2]), R0[2:]])
    Rw = np.where(ok[None], Rw, own)
    half, quarter = dtype(0.5), dtype(0.25)
    bx, by = (R0[0] - Rw[0]) * half, (R0[1] - Rw[1]) * half
    axx, ayy, axy = (R0[2] + Rw[2]) * half, (R0[3] + Rw[3]) * half, (R0[4] + Rw[4]) * quarter
    bx = bx + (axx * dx + axy * dy)
    by = by + (axy * dx + ayy * dy)
    s = border_scale(H, W, dtype)
    bx, by, axx, ayy, axy = bx * s, by * s, axx * s, ayy * s, axy * s
    return np.stack([axx * axx + axy * axy, (axx + ayy) * axy, ayy * ayy + axy * axy, axx * bx + axy * by, axy * bx + ayy * by])


def box_mean(M, winsize, dtype):
    """Mean over winsize x winsize, replicated borders: rows summed first, then columns, then one multiply by 1 / winsize^2."""
    ones = np.ones(winsize)
    v = correlate(M, ones, M.ndim - 2, "edge", dtype)
    return correlate(v, ones, M.ndim - 1, "edge", dtype) * dtype(1.0 / (winsize * winsize))


def solve(Mb, dtype):
    idet = dtype(1) / (Mb[0] * Mb[2] - Mb[1] * Mb[1] + dtype(1e-3))
    return np.stack([(Mb[2] * Mb[3] - Mb[1] * Mb[4]) * idet, (Mb[0] * Mb[4] - Mb[1] * Mb[3]) * idet])


def farneback_flow(p, q, pyr_scale=0.5, levels=2, winsize=15, iterations=2, poly_n=7, poly_sigma=1.5, flags=0, dtype=np.float64, stats=None):
    """flow[2, H, W] in fp32 (rounded once from `dtype`) from prev p to next q, both uint8 [H, W]."""
    p, q = np.asarray(p), np.asarray(q)
    if p.dtype != np.uint8 or q.dtype != np.uint8 or p.ndim != 2 or p.shape != q.shape:
        raise ValueError("two uint8 [H, W] planes of one shape expected")
    if flags != 0 or pyr_scale != 0.5 or winsize % 2 != 1 or poly_n not in (5, 7):
        raise ValueError("outside the contract")
    dtype = np.dtype(dtype).type
    H, W = p.shape
    flow = None
    for j in range(n_coarse(H, W, levels), -1, -1):
        h, w = plane_size(H, W, j)
        R0 = poly_exp(plane_image(p, j, dtype), poly_n, poly_sigma, dtype)
        R1 = poly_exp(plane_image(q, j, dtype), poly_n, poly_sigma, dtype)
        flow = np.zeros((2, h, w), dtype=dtype) if flow is None else resize(flow, h, w, dtype) * dtype(2)
        M = matrices(R0, R1, flow, dtype, stats)
        for it in range(iterations):
            flow = solve(box_mean(M, winsize, dtype), dtype)
            if it + 1 < iterations:
                M = matrices(R0, R1, flow, dtype, stats)
    return flow.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# labels
def update_labels(lab, flow):
    """cv2.remap(lab, col + flow[0], row + flow[1], INTER_NEAREST, BORDER_CONSTANT, 0): fp32 coordinates, rint (half to even)."""
    lab = np.asarray(lab)
    H, W = lab.shape
    flow = np.asarray(flow, dtype=np.float32)
    rows, cols = np.indices((H, W)).astype(np.float32)
    sx, sy = np.rint(cols + flow[0]), np.rint(rows + flow[1])
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)        # false for NaN
    xi, yi = np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64)
    return np.where(ok, lab[yi, xi], 0).astype(lab.dtype)


def rgb_to_gray(rgb):
    """cv2.COLOR_RGB2GRAY on uint8 [..., 3]."""
    c = np.asarray(rgb).astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def propagate_labels(pred, gray, dtype=np.float64, **params):
    """test.py:135-140 for one sequence: pred [T, H, W] class maps, gray [T, H, W] uint8, T >= 2."""
    pred, gray = np.asarray(pred), np.asarray(gray)
    T = pred.shape[0]
    if T < 2 or gray.shape != pred.shape:
        raise ValueError("pred and gray [T, H, W] with T >= 2 expected")
    out = np.zeros_like(pred)
    out[0] = update_labels(pred[1], farneback_flow(gray[0], gray[1], dtype=dtype, **params))
    for i in range(1, T):
        out[i] = update_labels(out[i - 1], farneback_flow(gray[i], gray[i - 1], dtype=dtype, **params))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded scenes for the tests and the golden generator
def texture(rng, H, W, margin=8, sigma=2.0):
    """Smoothed noise stretched to 20..235, [H + 2 margin, W + 2 margin] float64: shifted crops of it have a known motion.  sigma = 2 leaves
    structure at every scale the 15-tap windows see; smoother scenes (sigma >= 3) leave windows near an edge the motion leaves through with
    too little of it, and the method (not an implementation of it) then misses by half a pixel there."""
    from scipy.ndimage import gaussian_filter
    t = gaussian_filter(rng.standard_normal((H + 2 * margin, W + 2 * margin)), sigma, mode="wrap")
    t = (t - t.min()) / (t.max() - t.min())
    return 20.0 + 215.0 * t


def crop_pair(canvas, H, W, d, margin=8):
    """p, q [H, W] cut from a [H + 2 margin, W + 2 margin] canvas with q(x) = p(x - d), d = (dx, dy) whole pixels, |d| <= margin."""
    dx, dy = d
    p = canvas[margin:margin + H, margin:margin + W]
    q = canvas[margin - dy:margin - dy + H, margin - dx:margin - dx + W]
    return np.ascontiguousarray(p), np.ascontiguousarray(q)


def shifted_pair(rng, H, W, d, margin=8):
    return crop_pair(np.rint(texture(rng, H, W, margin)).astype(np.uint8), H, W, d, margin)


def label_blobs(rng, H, W, num_class=5, sigma=4.0):
    """A class map uint8 [H, W] with a few large regions."""
    from scipy.ndimage import gaussian_filter
    f = np.stack([gaussian_filter(rng.standard_normal((H, W)), sigma) for _ in range(num_class)])
    return f.argmax(0).astype(np.uint8)


# the device cases of tests/test_gpu_farneback.py: name -> (H, W, shifts of the B pairs or None for two independent frames, parameters)
OTHER = dict(levels=3, poly_n=5, poly_sigma=1.1, winsize=9, iterations=3)
GPU_CASES = {
    "120x160_b2": (120, 160, [(3, -2), (-5, 4)], {}),          # the workload's plane
    "64x64": (64, 64, [(1, 1)], {}),                            # the smallest shape with a coarse plane
    "67x71": (67, 71, [(3, -2)], {}),                           # non-integer resize ratios, plane size rounded half to even (34 x 36)
    "48x64": (48, 64, [(1, 1)], {}),                            # one plane
    "33x47": (33, 47, [(1, 1)], {}),                            # one plane, odd
    "9x11": (9, 11, [(1, 0)], {}),                              # every pixel in the border zone, windows larger than the plane
    "128x132_other": (128, 132, [(-5, 4)], OTHER),              # three planes, the other parameter set
    "noise_64x80": (64, 80, None, {}),                          # independent frames: large chaotic flows, the warp leaves the plane
}


def gpu_case(name):
    """prev, next uint8 [B, H, W] and the parameters of a device case (seeded by the name's position in GPU_CASES)."""
    H, W, shifts, params = GPU_CASES[name]
    rng = np.random.default_rng(1000 + list(GPU_CASES).index(name))
    if shifts is None:
        p = np.rint(texture(rng, H, W, 0, sigma=2.0)).astype(np.uint8)[None]
        q = np.rint(texture(rng, H, W, 0, sigma=2.0)).astype(np.uint8)[None]
        return p, q, params
    pairs = [shifted_pair(rng, H, W, d) for d in shifts]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), params


def sequences(S=2, T=3, H=64, W=64, seed=77):
    """pred, gray uint8 [S, T, H, W]: a texture and a class map drifting by whole pixels from frame to frame."""
    rng = np.random.default_rng(seed)
    margin = 8
    pred, gray = np.zeros((S, T, H, W), np.uint8), np.zeros((S, T, H, W), np.uint8)
    for s in range(S):
        tex = np.rint(texture(rng, H, W, margin)).astype(np.uint8)
        lab = label_blobs(rng, H + 2 * margin, W + 2 * margin)
        step = [(2, -1), (-1, 2)][s % 2]
        for t in range(T):
            d = (step[0] * t, step[1] * t)
            gray[s, t] = crop_pair(tex, H, W, d, margin)[1]
            pred[s, t] = crop_pair(lab, H, W, d, margin)[1]
    return pred, gray
