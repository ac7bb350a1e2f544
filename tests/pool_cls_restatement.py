"""Float64 numpy restatement of the pooled classification head (RCV_OP_POOL_CLS_FWD / _BWD, csrc/pool_cls.hip) and the seeded
integer-grid cases of its exact GPU tests (tests/test_gpu_pool_cls.py).  Imports nothing from the library; pinned against float64
torch autograd by tests/test_pool_cls.py, which also asserts every case's preconditions without a GPU.

A case is the tuple (N, H, W, C, nC, k, load mode, statistics kind, resid, dropout): k = 2 / 4 a k x k max with stride k and floor
(nn.MaxPool2d(k)), k = 0 the plane mean (AdaptiveAvgPool2d(1)).  Tensors are NHWC, the logits and their gradient NCHW."""
import numpy as np

import small_ops_restatement as S

LOAD_PLAIN, LOAD_AFFINE, LOAD_AFFINE_RELU = S.LOAD_PLAIN, S.LOAD_AFFINE, S.LOAD_AFFINE_RELU
STATS_NONE, STATS_BWD_ENC, STATS_BWD_DEC = S.STATS_NONE, S.STATS_BWD_ENC, S.STATS_BWD_DEC
MAX_C, MAX_OUT = 512, 8


def load(r, cst, mode):
    if mode == LOAD_PLAIN:
        return r
    v = r * cst[0] + cst[1]
    return np.maximum(v, 0.0) if mode == LOAD_AFFINE_RELU else v


def pooled_plane(H, W, k):
    return (H // k, W // k) if k else (1, 1)


def windows(v, k):
    """[N,H,W,C] -> [N,Hp,Wp,k*k,C], the window in row-major order; the floor remainder is left out."""
    N, H, W, C = v.shape
    Hp, Wp = H // k, W // k
    return v[:, :Hp * k, :Wp * k, :].reshape(N, Hp, k, Wp, k, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, k * k, C)


def _parts(case, r, cst, w, b, scale, dl, res, keep):
    """Every intermediate of the head in float64 (see reference())."""
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    r64, c64 = r.astype(np.float64), cst.astype(np.float64)
    v = load(r64, c64, mode)
    Hp, Wp = pooled_plane(H, W, k)
    first = None
    if k:
        win = windows(v, k)
        pooled = win.max(axis=3)
        first = win.argmax(axis=3)               # numpy: the first occurrence of the maximum = row-major window order
    else:
        vk = v if keep is None else v * np.asarray(keep, np.float64).reshape(N, H, W, 1)
        pooled = vk.sum(axis=(1, 2)).reshape(N, 1, 1, C) / (H * W)
    s = np.ones((N, 1, 1, C)) if scale is None else scale.astype(np.float64).reshape(N, 1, 1, C)
    pd = pooled * s
    w2 = w.reshape(nC, C).astype(np.float64)
    dl64 = dl.astype(np.float64)
    dpool = np.einsum("noyx,oc->nyxc", dl64, w2) * s
    return r64, c64, v, pooled, first, s, pd, w2, dl64, dpool


def reference(case, r, cst, w, b, scale, dl, res, keep=None):
    """-> pooled [N,Hp,Wp,C] (before the dropout), logits [N,nC,Hp,Wp], dW [nC,C,1,1], db [nC], dy [N,H,W,C] = d loss / d load(r)
    (+ res), the statistics rows [2][C] (None for STATS_NONE), as pool_cls_scatter_kernel's header defines them:
    row 0 = sum v, row 1 = sum v (r - mu), v = dy (ENC) or dy where r c0 + c1 > 0 (DEC), c0 / c1 / mu = rows 0 / 1 / 2 of cst.
    keep: a boolean vector over the N*H*W source pixels; a pixel whose entry is False adds nothing to the plane mean (and so to the
    logits and dW) nor to the statistics rows -- what a kernel that lost the pixel would compute (the sensitivity checks)."""
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    r64, c64, v, pooled, first, s, pd, w2, dl64, dpool = _parts(case, r, cst, w, b, scale, dl, res, keep)
    Hp, Wp = pooled_plane(H, W, k)
    logits = np.einsum("nyxc,oc->noyx", pd, w2) + b.astype(np.float64).reshape(1, nC, 1, 1)
    dW = np.einsum("noyx,nyxc->oc", dl64, pd).reshape(nC, C, 1, 1)
    db = dl64.sum(axis=(0, 2, 3))
    dy = np.zeros((N, H, W, C))
    if k:
        for j in range(k * k):
            sel = (first == j)
            dy[:, j // k:Hp * k:k, j % k:Wp * k:k, :][:, :Hp, :Wp, :] = np.where(sel, dpool, 0.0)
    else:
        dy[:] = dpool / (H * W)
    if res is not None:
        dy += res.astype(np.float64)
    st = None
    if stats != STATS_NONE:
        g = dy if stats == STATS_BWD_ENC else np.where(r64 * c64[0] + c64[1] > 0, dy, 0.0)
        if keep is not None:
            g = g * np.asarray(keep, np.float64).reshape(N, H, W, 1)
        st = np.stack([g.sum(axis=(0, 1, 2)), (g * (r64 - c64[2])).sum(axis=(0, 1, 2))])
    return pooled, logits, dW, db, dy, st


def terms_abs(case, r, cst, w, b, scale, dl, res, unit=1.0):
    """name -> (sum of |terms| of every entry of a reduced quantity, its quantum): the integer-grid precondition (S.assert_exact).
    With the plane mean the pooled features are multiples of 1 / P (P = H W, a power of two) and the case builder scales the logits
    gradient by P, so that the gradient's share dpool / P of a pixel is an integer again.  unit: the grid's own step (1/2 where the
    source holds -2.5)."""
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    r64, c64, v, pooled, first, s, pd, w2, dl64, dpool = _parts(case, r, cst, w, b, scale, dl, res, None)
    P = 1 if k else H * W
    out = {}
    if not k:
        out["pooled"] = (np.abs(v).sum(axis=(1, 2)), 1.0)
    out["logits"] = (np.einsum("nyxc,oc->noyx", np.abs(pd), np.abs(w2)) + np.abs(b.astype(np.float64)).reshape(1, nC, 1, 1), 1.0 / P)
    out["dW"] = (np.einsum("noyx,nyxc->oc", np.abs(dl64), np.abs(pd)), 1.0)
    out["db"] = (np.abs(dl64).sum(axis=(0, 2, 3)), float(P))
    out["dpool"] = (np.einsum("noyx,oc->nyxc", np.abs(dl64), np.abs(w2)) * s, float(P))
    if stats != STATS_NONE:
        dy = reference(case, r, cst, w, b, scale, dl, res)[4]
        out["statistics"] = (S.stats_abs(stats, dy, r64, c64), 1.0)
    return {name: (t, q * unit) for name, (t, q) in out.items()}


# ------------------------------------------------------------------------------------------ launch geometry
def block(C):
    """pool_cls_block: the largest multiple of C / 4 within 256 threads (a thread keeps its channel quad across the passes)."""
    C4 = C // 4
    return (256 // C4) * C4


def pass_items(num_cus, C):
    """Work items (pixel x channel quad) of one grid pass of pool_cls_scatter_kernel: pool_cls_grid caps it at 4 workgroups per CU."""
    return 4 * num_cus * block(C)


def items(case):
    N, H, W, C = case[:4]
    return N * H * W * (C // 4)


# ------------------------------------------------------------------------------------------ the exact cases
CHANNELS = (4, 20, 64, 260, 512)
MODES = (LOAD_PLAIN, LOAD_AFFINE, LOAD_AFFINE_RELU)
KINDS = (STATS_BWD_ENC, STATS_BWD_DEC, STATS_NONE)


def small_cases():
    """The small planes: 2x9x11 (k = 2: one remainder row and column; k = 4: one row, three columns), one window exactly (1x2x2 with
    k = 2, 1x4x4 with k = 4), the 1x1 plane mean of three images, and plane means over 8 and 32 pixels -- every channel count with
    1 and 8 classes; the load mode, the statistics kind, the residual and the dropout rotate so that every k meets every mode, every
    kind, and both settings of the two flags."""
    planes = [(2, 9, 11, 2), (2, 9, 11, 4), (1, 2, 2, 2), (1, 4, 4, 4), (3, 1, 1, 0), (2, 2, 4, 0), (3, 4, 8, 0)]
    out = []
    for ci, C in enumerate(CHANNELS):
        for ni, nC in enumerate((1, 8)):
            for pi, (N, H, W, k) in enumerate(planes):
                j = ci + 2 * ni + pi
                out.append((N, H, W, C, nC, k, MODES[j % 3], KINDS[(j // 3 + pi) % 3], bool((j + ni) % 2), bool((j // 2 + ci) % 2)))
    out += [(2, 9, 11, 64, 5, 2, m, st, True, True) for m in MODES for st in KINDS]          # every mode x kind on the remainder plane
    out += [(2, 9, 11, 64, 5, 4, LOAD_AFFINE_RELU, STATS_BWD_DEC, False, False), (2, 4, 4, 64, 5, 0, LOAD_AFFINE, STATS_BWD_ENC, False, False)]
    return out


def big_cases(num_cus):
    """One case per channel count whose work items exceed one grid pass of the scatter kernel (the pixel counts: above 262 144 at
    C = 4, above 2048 at C = 512 on 256 CUs), k, mode, kind and class count rotating; the plane means run on planes of 2^j pixels
    and more images.  The last case is the one whose work-item count is no multiple of the block."""
    def max_plane(C, k, W):
        need = pass_items(num_cus, C) // (C // 4) + 1
        H = -(-need // W)
        return (1, H + (k - H % k) % k + 1, W)          # a remainder row on top of whole windows

    def mean_plane(C, H, W):
        need = pass_items(num_cus, C) // (C // 4) + 1
        return (-(-need // (H * W)), H, W)

    out = [max_plane(4, 2, 513) + (4, 8, 2, LOAD_AFFINE, STATS_BWD_ENC, True, False),
           mean_plane(20, 64, 64) + (20, 1, 0, LOAD_AFFINE_RELU, STATS_BWD_DEC, True, True),
           max_plane(64, 4, 67) + (64, 8, 4, LOAD_AFFINE_RELU, STATS_BWD_DEC, True, True),
           mean_plane(260, 16, 32) + (260, 8, 0, LOAD_AFFINE, STATS_BWD_ENC, True, True),
           max_plane(512, 2, 45) + (512, 1, 2, LOAD_PLAIN, STATS_BWD_DEC, True, False),
           mean_plane(4, 128, 128) + (4, 5, 0, LOAD_PLAIN, STATS_BWD_ENC, False, True),
           mean_plane(512, 16, 16) + (512, 8, 0, LOAD_AFFINE_RELU, STATS_BWD_DEC, True, True)]
    odd = max_plane(4, 2, 295) + (4, 1, 2, LOAD_AFFINE_RELU, STATS_BWD_DEC, True, True)
    if items(odd) % block(4) == 0:
        odd = (1, odd[1] + 2, odd[2] + 2) + odd[3:]
    out.append(odd)
    for c in out:
        assert items(c) > pass_items(num_cus, c[3]) and (c[5] or (c[1] * c[2]) & (c[1] * c[2] - 1) == 0), c
    assert items(out[-1]) % block(out[-1][3]) != 0
    return out


def build(case, second_item=0, seed=0, density=1.0):
    """Operands of a case on the integer grid: r, res, w, b in {-2..2} (r, res in {-1..1} on the large planes), load constants of
    S.grid_consts (scales +-1, +-2 -- positive ones under LOAD_PLAIN, where the scale row only feeds the DEC mask --, integer shifts
    and means), Dropout2d keep-scales in {0, 2}, dl on the grid times P (terms_abs).  second_item: the first work item of the second
    grid pass.  The two pixels of S.drop_masks are strict maxima of their windows in every channel with the DEC mask on and
    r != mean, their pooled pixel has dl = P for every class and their image keeps every channel (scale 2), the filter's column sums
    are non-zero and the residual there has the sign of the gradient: the gradient (with the residual, or inside a window) is
    non-zero there in every channel."""
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    npix = N * H * W
    rng = np.random.default_rng(41000 + 7 * seed + npix + 3 * C + 11 * nC + k + mode + 5 * stats)
    a = 1 if npix * C > 100000 else 2
    P = 1 if k else H * W
    Hp, Wp = pooled_plane(H, W, k)
    c = dict(case=case, npix=npix, P=P, second=second_item // (C // 4))
    c["r"] = S.grid(rng, (N, H, W, C), a, density)
    c["cst"] = S.grid_consts(rng, C)
    if mode == LOAD_PLAIN:
        c["cst"][0] = np.abs(c["cst"][0])
    c["w"] = S.grid(rng, (nC, C, 1, 1), 2)
    c["b"] = S.grid(rng, (nC,), 2)
    c["dl"] = S.grid(rng, (N, nC, Hp, Wp), a) * np.float32(P)
    c["res"] = S.grid(rng, (N, H, W, C), a, density) if resid else None
    c["scale"] = (2.0 * (rng.random((N, C)) < 0.5)).astype(np.float32) if drop else None
    w2 = c["w"].reshape(nC, C)
    col = w2.sum(0)
    w2[0, col == 0] += np.where(w2[0, col == 0] < 2, 1, -1)
    col = w2.sum(0)
    idx, _ = S.drop_masks(npix, c["second"])
    inside, seen = True, set()
    for i in idx:
        n, y, x = i // (H * W), (i // W) % H, i % W
        c["r"][n, y, x] = 5 * np.sign(c["cst"][0])
        if drop:
            c["scale"][n] = 2.0
        if resid:
            c["res"][n, y, x] = np.sign(col)
        if not k:
            c["dl"][n, :, 0, 0] = P
        elif y // k < Hp and x // k < Wp and (n, y // k, x // k) not in seen:
            c["dl"][n, :, y // k, x // k] = 1.0
            seen.add((n, y // k, x // k))
        else:                                        # in the floor remainder, or second in a window the other pixel already wins
            inside = False
    c["sensitive"] = bool(resid or inside)
    return c


def operands(c):
    return tuple(c[n] for n in ("r", "cst", "w", "b", "scale", "dl", "res"))


def reduced(c, keep=None):
    """What the sensitivity check looks at: both statistics rows, and dW for the plane mean."""
    _, _, dW, _, _, st = reference(c["case"], *operands(c), keep=keep)
    return (() if st is None else (st,)) + (() if c["case"][5] else (dW,))


def check(c, unit=1.0):
    """The preconditions of an exact case: every reduction's sum of |terms| is a multiple of its quantum below 2^24 of it; where the
    case can be (a residual, or both pixels inside a window), removing the last pixel or the first pixel of the second grid pass
    changes every entry of what reduced() returns."""
    for name, (t, q) in terms_abs(c["case"], *operands(c), unit=unit).items():
        S.assert_exact(t, q, "pool_cls %s %s" % (c["case"], name))
    full = reduced(c)
    if c["sensitive"] and full:
        idx, masks = S.drop_masks(c["npix"], c["second"])
        for i, keep in zip(idx, masks):
            for a, b in zip(full, reduced(c, keep)):
                assert np.all(a != b), "pool_cls %s: removing pixel %d leaves %d entries unchanged" % (c["case"], i, int((a == b).sum()))


# ------------------------------------------------------------------------------------------ ties
def build_ties(mode, k, C=64, nC=5):
    """A 2 x 3k x 3k plane on the integer grid (shifts of the first quarter of the channels -6: under LOAD_AFFINE_RELU most of their
    windows are all zero) whose first image holds, in every channel: window (0, 0) one value throughout; window (0, 1) every column a
    copy of its first; window (1, 0) a maximum that sits at position 1 and again in the LAST position only; window (1, 1) all -2.5
    (ReLU zero under LOAD_AFFINE_RELU: the first pixel wins).  -> the case dict of build()."""
    case = (2, 3 * k, 3 * k, C, nC, k, mode, STATS_BWD_DEC, True, False)
    c = build(case, seed=77)
    r, cst = c["r"], c["cst"]
    cst[0] = np.abs(cst[0])
    cst[1, : C // 4] = -6.0
    r[0, 0:k, 0:k, :] = r[0, 0, 0, :]
    r[0, 0:k, k:2 * k, :] = r[0, 0:k, k:k + 1, :]
    r[0, k:2 * k, 0:k, :] = -2.0
    r[0, k, 1, :] = 2.0
    r[0, 2 * k - 1, k - 1, :] = 2.0
    r[0, k:2 * k, k:2 * k, :] = -2.5
    c["sensitive"] = False                       # the constants changed under build()'s two pixels: no sensitivity claim here
    c["dl"][0, :, :2, :2] = 1.0                  # the four windows' gradients: the filter's column sums, non-zero in every channel
    return c
