"""Float64 numpy restatement of the operations around the 3x3 contractions of the training step -- load transforms, the three kinds
of epilogue statistics (include/rcv.h), BatchNorm bookkeeping, the 1x1 classifier, weighted cross entropy, the Dice loss, 2x2
max-pool, SGD, the Adam + L1 step with its running rounding bound, the filter-gradient reduction, the confusion counts -- and the
integer-grid operand generators the exact GPU tests use.  Imports nothing from the library; pinned against
torch float64 autograd by tests/test_small_ops.py.

Tensors are NHWC ([..., C]) unless a name says NCHW.  Every reduction takes `keep`, a boolean vector over the pixels (leading axes
flattened): a pixel whose entry is False contributes nothing (the sensitivity checks of the GPU tests drop single pixels)."""
import numpy as np

LOAD_PLAIN, LOAD_AFFINE, LOAD_GRAD_ENC, LOAD_GRAD_DEC, LOAD_NCHW, LOAD_AFFINE_RELU = range(6)
STATS_NONE, STATS_FWD, STATS_BWD_ENC, STATS_BWD_DEC = range(4)
F64 = np.float64


def _f(a):
    return np.asarray(a, F64)


# ------------------------------------------------------------------------------------------ load modes
def load(x, c=None, mode=LOAD_PLAIN, aux=None):
    """rcv.h RCV_LOAD_*: c = rows c0..c4 over the channels (last axis)."""
    x = _f(x)
    if mode in (LOAD_PLAIN, LOAD_NCHW):
        return x
    c = _f(c)
    if mode == LOAD_AFFINE:
        return x * c[0] + c[1]
    if mode == LOAD_AFFINE_RELU:
        return np.maximum(x * c[0] + c[1], 0.0)
    a = _f(aux)
    if mode == LOAD_GRAD_ENC:          # BN backward, then ReLU backward
        return np.where(a > 0, c[0] * x + c[1] + c[2] * a, 0.0)
    if mode == LOAD_GRAD_DEC:          # ReLU backward, then BN backward
        return c[0] * np.where(a * c[3] + c[4] > 0, x, 0.0) + c[1] + c[2] * a
    raise ValueError(mode)


def _pix(a, keep):
    """[..., C] -> [npix, C] with the dropped pixels zeroed."""
    a = _f(a).reshape(-1, np.shape(a)[-1])
    return a if keep is None else a * np.asarray(keep, F64)[:, None]


# ------------------------------------------------------------------------------------------ epilogue statistics
def stats(kind, v, e=None, ec=None, keep=None):
    """The column sums [2][C] the partial rows add up to.  v = the stored tensor; e = p[EPI_AUX]; ec rows = (c0, c1, mean).
    FWD: sum v, sum v^2.  BWD_ENC: sum v, sum v (e - mean).  BWD_DEC: the same of v m, m = (e c0 + c1 > 0)."""
    v = _f(v)
    if kind == STATS_FWD:
        return np.stack([_pix(v, keep).sum(0), _pix(v * v, keep).sum(0)])
    e, ec = _f(e), _f(ec)
    if kind == STATS_BWD_DEC:
        v = np.where(e * ec[0] + ec[1] > 0, v, 0.0)
    return np.stack([_pix(v, keep).sum(0), _pix(v * (e - ec[2]), keep).sum(0)])


def stats_abs(kind, v, e=None, ec=None):
    """Sum of |term| of every column sum of stats(): the scale of its rounding bound and the integer-grid precondition."""
    v = _f(v)
    if kind == STATS_FWD:
        return np.stack([_pix(np.abs(v), None).sum(0), _pix(v * v, None).sum(0)])
    e, ec = _f(e), _f(ec)
    if kind == STATS_BWD_DEC:
        v = np.where(e * ec[0] + ec[1] > 0, v, 0.0)
    return np.stack([_pix(np.abs(v), None).sum(0), _pix(np.abs(v * (e - ec[2])), None).sum(0)])


# ------------------------------------------------------------------------------------------ BatchNorm bookkeeping
def bn_finalize(rows, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True):
    """rows [n_part][2][C] (sum v, sum v^2) -> consts [5][C] (scale, shift, mean, 0, 0), mean, istd and the updated running
    statistics (unchanged, or None, unless training and present).  The variance is the biased one, clamped at 0; the running
    variance takes the unbiased one (count > 1)."""
    rows, gamma, beta = _f(rows), _f(gamma), _f(beta)
    s = rows.sum(0)
    mean = s[0] / count
    var = np.maximum(s[1] / count - mean * mean, 0.0)
    istd = 1.0 / np.sqrt(var + F64(eps))
    sc = gamma * istd
    consts = np.stack([sc, beta - mean * sc, mean, np.zeros_like(sc), np.zeros_like(sc)])
    rm, rv = running_mean, running_var
    if training and running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        rm = (1.0 - F64(momentum)) * _f(running_mean) + F64(momentum) * mean
        rv = (1.0 - F64(momentum)) * _f(running_var) + F64(momentum) * unbiased
    return dict(consts=consts, mean=mean, istd=istd, running_mean=rm, running_var=rv, var=var)


def bn_backward(rows, count, gamma, mean, istd, fwd_consts):
    """rows [n_part][2][C] (sum g, sum g (r - mean)) -> consts (A, B, C, fwd scale, fwd shift) with dr = A g + B + C r,
    dgamma, dbeta (aten::native_batch_norm_backward)."""
    rows, gamma, mean, istd, fc = _f(rows), _f(gamma), _f(mean), _f(istd), _f(fwd_consts)
    s = rows.sum(0)
    sgx = istd * s[1]
    A = gamma * istd
    Cc = -A * istd * sgx / count
    B = -A * s[0] / count - Cc * mean
    return dict(consts=np.stack([A, B, Cc, fc[0], fc[1]]), dgamma=sgx, dbeta=s[0])


def bn_eval(gamma, beta, running_mean, running_var, eps, conv_bias=None):
    """Running statistics -> consts [5][C]: scale, shift, 0, the conv bias seen through the BatchNorm (bias or 0) * scale + shift, 0."""
    gamma, beta, rm, rv = _f(gamma), _f(beta), _f(running_mean), _f(running_var)
    sc = gamma / np.sqrt(rv + F64(eps))
    sh = beta - rm * sc
    b = np.zeros_like(sc) if conv_bias is None else _f(conv_bias)
    return np.stack([sc, sh, np.zeros_like(sc), b * sc + sh, np.zeros_like(sc)])


# ------------------------------------------------------------------------------------------ 1x1 classifier
def fused_up(t, tc, r, rc, mode2):
    """The decoder output the fused classifier forms on the fly: relu(t c0 + c1) + f(r)."""
    return np.maximum(_f(t) * _f(tc)[0] + _f(tc)[1], 0.0) + load(r, rc, mode2)


def cls_forward(up, w, b=None):
    """up [N,H,W,K], w [C,K], b [C] -> logits NCHW."""
    up, w = _f(up), _f(w)
    lg = np.ascontiguousarray((up.reshape(-1, up.shape[-1]) @ w.T).reshape(up.shape[:3] + (w.shape[0],)).transpose(0, 3, 1, 2))
    return lg if b is None else lg + _f(b)[None, :, None, None]


def cls_backward(up, dlogits, w, keep=None):
    """-> d_up [N,H,W,K] (every pixel), dW [C,K], db [C] (over the kept pixels)."""
    up, dl, w = _f(up), np.ascontiguousarray(_f(dlogits).transpose(0, 2, 3, 1)), _f(w)
    d_up = (dl.reshape(-1, dl.shape[-1]) @ w).reshape(up.shape)
    dlp = _pix(dl, keep)
    return d_up, dlp.T @ up.reshape(-1, up.shape[-1]), dlp.sum(0)


def cls_backward_abs(up, dlogits):
    dl, up = np.abs(_f(dlogits)).transpose(0, 2, 3, 1), np.abs(_f(up))
    dlp = dl.reshape(-1, dl.shape[-1])
    return dlp.T @ up.reshape(-1, up.shape[-1]), dlp.sum(0)


# ------------------------------------------------------------------------------------------ losses
def _softmax(lg):
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    return e / e.sum(1, keepdims=True), (lg - m) - np.log(e.sum(1, keepdims=True))


def cross_entropy(logits, target, weights=None, grad_out=1.0):
    """Weighted CrossEntropyLoss2d; a label outside [0, C) is ignored (NLLLoss's ignore_index).
    -> loss, sum of weights, #(arg-max == label), d loss / d logits, arg-max (first maximum)."""
    lg, t = _f(logits), np.asarray(target)
    C = lg.shape[1]
    p, logp = _softmax(lg)
    onehot = t[:, None] == np.arange(C)[None, :, None, None]
    ok = (t >= 0) & (t < C)
    w = np.ones(C) if weights is None else _f(weights)
    wt = np.where(ok, w[np.clip(t, 0, C - 1)], 0.0)
    sw = wt.sum()
    loss = -(wt * (logp * onehot).sum(1)).sum() / sw
    am = lg.argmax(1)
    return dict(loss=loss, sum_w=sw, correct=int((am == t).sum()), dlogits=grad_out * (p - onehot) * wt[:, None] / sw, argmax=am)


def dice(logits, target, weights=None, eps=1e-7, grad_out=1.0):
    """DiceLoss, multi-class branch: loss = 1 - mean_c 2 w_c I_c / (S_c + N_c + eps); I_c = sum P_c [t == c], S_c = sum P_c,
    N_c = #[t == c].  A label outside [0, C) has an all-zero one-hot row: it adds to S_c only.
    -> loss, A_c, B_c (d loss / d P[p][c] = A_c [t_p == c] + B_c), #correct, d loss / d logits, arg-max."""
    lg, t = _f(logits), np.asarray(target)
    C = lg.shape[1]
    p, _ = _softmax(lg)
    onehot = (t[:, None] == np.arange(C)[None, :, None, None]).astype(F64)
    w = np.ones(C) if weights is None else _f(weights)
    I, K = (p * onehot).sum((0, 2, 3)), (p + onehot).sum((0, 2, 3)) + F64(eps)
    loss = 1.0 - (2.0 * w * I / K).mean()
    A, B = -(2.0 * w / C) / K, (2.0 * w / C) * I / (K * K)
    gq = B[None, :, None, None] + A[None, :, None, None] * onehot
    dl = grad_out * p * (gq - (p * gq).sum(1, keepdims=True))
    am = lg.argmax(1)
    return dict(loss=loss, A=A, B=B, correct=int((am == t).sum()), dlogits=dl, argmax=am)


# ------------------------------------------------------------------------------------------ 2x2 max-pool
def _windows(a):
    """[N,H,W,C] -> [N,H/2,W/2,4,C], window order (0,0), (0,1), (1,0), (1,1)."""
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def pool_forward(r, c=None, mode=LOAD_PLAIN):
    return _windows(load(r, c, mode)).max(3)


def pool_backward(dp, r, c=None, mode=LOAD_PLAIN, resid=None):
    """dy [N,H,W,C]: dp goes to the FIRST maximum of load(r) in each window (aten::max_pool2d_with_indices), + resid."""
    v = _windows(load(r, c, mode))
    N, Ho, Wo, _, C = v.shape
    first = v.argmax(3)                                    # numpy: the first of equal maxima
    sel = (first[:, :, :, None, :] == np.arange(4)[None, None, None, :, None]) * _f(dp)[:, :, :, None, :]
    dy = sel.reshape(N, Ho, Wo, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)
    return dy if resid is None else dy + _f(resid)


# ------------------------------------------------------------------------------------------ SGD
def sgd_step(p, g, buf, step, lr, momentum, wd, grad_scale=1.0, lr_elem=None):
    """torch.optim.SGD(momentum, weight_decay), dampening 0: -> (p, buf).  lr_elem == 0: the element (and its buffer) is untouched."""
    p, g, buf = _f(p), _f(g), _f(buf)
    lre = np.full(p.shape, F64(lr)) if lr_elem is None else _f(lr_elem)
    gr = g * F64(grad_scale) + F64(wd) * p
    b = gr if step == 1 else F64(momentum) * buf + gr
    live = lre != 0
    return np.where(live, p - lre * b, p), np.where(live, b, buf)


# ------------------------------------------------------------------------------------------ Adam + L1
U32 = 2.0 ** -24        # unit roundoff of fp32, round to nearest: |fl(x) - x| <= U32 |x|


def _w32(x):
    """A hyper-parameter as the record carries it: rounded to fp32, widened."""
    return F64(np.float32(x))


def adam_l1_step(p, g, m, v, t, lr, b1, b2, eps, decay, grad_scale=1.0, lr_elem=None, prune=None, round_bc=True):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on the gradient g * grad_scale + decay * sign(p) (the gradient of
    decay * sum|p|, sign(+-0) = 0), float64 from the fp32 operands, hyper-parameters rounded to fp32 and widened:
        gr = decay sign(p) + g gs  (0 where prune);  m' = b1 m + (1 - b1) gr;  v' = b2 v + ((1 - b2) gr) gr;
        p' = p - (lre / bc1) (m' / (sqrt(v') / bc2_sqrt + eps)),  bc1 = 1 - b1^t,  bc2_sqrt = sqrt(1 - b2^t), both rounded to fp32
    (round_bc=False leaves them unrounded: the comparison with torch.optim.Adam only).  lr_elem == 0: the element and its moments
    are returned untouched.

    -> (p', m', v'), (ep, em, ev): the values and a running first-order bound on the error of an fp32 evaluation in this order of
    operations: each fp32 operation adds U32 |its result| (for a sum: of the rounded sum, the terms' own errors having been
    carried), earlier errors go through each operation by its derivative, bc1 and bc2_sqrt carry one rounding each of their own
    (a double pow may differ in the last place), 1 - b1 and 1 - b2 their actual fp32 error (0 for b >= 1/2), and the square root
    passes ev on as sqrt(v' + ev) - sqrt(v') (no division by sqrt(v'): v' = 0 is not singular).  A contraction into an fma only
    removes a rounding."""
    p, g, m, v = _f(p), _f(g), _f(m), _f(v)
    lr, b1, b2, eps, decay, gs = (_w32(x) for x in (lr, b1, b2, eps, decay, grad_scale))
    bc1, bc2s = 1.0 - b1 ** F64(t), np.sqrt(1.0 - b2 ** F64(t))
    if round_bc:
        bc1, bc2s = _w32(bc1), _w32(bc2s)
    o1, o2 = 1.0 - b1, 1.0 - b2
    eo1, eo2 = abs(_w32(o1) - o1), abs(_w32(o2) - o2)
    lre = np.full(p.shape, lr) if lr_elem is None else _f(lr_elem)
    A = np.abs
    a = g * gs
    gr = decay * np.sign(p) + a                                      # fmaf(decay, sg, fl(g gs)): 2 roundings
    egr = U32 * A(a) + U32 * A(gr)
    if prune is not None:
        pr = np.asarray(prune) != 0
        gr, egr = np.where(pr, 0.0, gr), np.where(pr, 0.0, egr)
    t1, t2 = b1 * m, o1 * gr
    m1 = t1 + t2
    em = U32 * A(t1) + (o1 * egr + eo1 * A(gr) + U32 * A(t2)) + U32 * A(m1)
    s1 = o2 * gr
    es1 = o2 * egr + eo2 * A(gr) + U32 * A(s1)
    s2, t3 = s1 * gr, b2 * v
    v1 = t3 + s2
    ev = U32 * A(t3) + (A(gr) * es1 + A(s1) * egr + U32 * A(s2)) + U32 * A(v1)
    sq = np.sqrt(v1)
    esq = (np.sqrt(v1 + ev) - sq) + U32 * sq
    q = sq / bc2s
    eq = esq / bc2s + q * U32 + U32 * q                              # bc2_sqrt's own rounding, the quotient's
    den = q + eps
    eden = eq + U32 * den
    step = lre / bc1
    estep = A(step) * U32 + U32 * A(step)                            # bc1's own rounding, the quotient's
    r = m1 / den
    er = em / den + A(r) * eden / den + U32 * A(r)
    w = step * r
    ew = A(step) * er + A(r) * estep + U32 * A(w)
    p1 = p - w
    ep = ew + U32 * A(p1)
    live = lre != 0
    z = np.zeros_like(p)
    return ((np.where(live, p1, p), np.where(live, m1, m), np.where(live, v1, v)),
            (np.where(live, ep, z), np.where(live, em, z), np.where(live, ev, z)))


# ------------------------------------------------------------------------------------------ filter-gradient reduction
def wgrad_reduce(part, part_bias, CB, CA):
    """part [nsplit][9][CBP][CAP], part_bias [nsplit][CBP] or None -> dW [CB][CA][3][3], db [CB] (None): float64 sums over the
    splits; the pad rows / columns (cb >= CB, ca >= CA) are not looked at."""
    s = _f(part)[:, :, :CB, :CA].sum(0)                              # [9][CB][CA]
    dw = np.ascontiguousarray(s.transpose(1, 2, 0)).reshape(CB, CA, 3, 3)
    return dw, (None if part_bias is None else _f(part_bias)[:, :CB].sum(0))


# ------------------------------------------------------------------------------------------ confusion counts
def confusion(pred, target, C):
    """counts[n][pred][label] (int64) over the pixels with pred < C and 0 <= label < C, the label taken as the int64 it is."""
    pred, target = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    N = pred.shape[0]
    pn, tn = pred.reshape(N, -1), target.reshape(N, -1)
    ok = (pn < C) & (tn >= 0) & (tn < C)
    image = np.broadcast_to(np.arange(N)[:, None], pn.shape)
    return np.bincount(((image * C + pn) * C + tn)[ok], minlength=N * C * C).reshape(N, C, C)     # one bin per (image, pred, label)


# ------------------------------------------------------------------------------------------ the integer grid
# Operands of the exact cases: activations / gradients / filters in {-amp..amp}, scales +-2^k, shifts and means small integers.
# Every product and every partial sum of a reduction is then an integer multiple of a power of two q below 2^24 q: exact in fp32 in
# ANY summation order, so the float64 result equals the kernel's bit for bit.
def grid(rng, shape, amp=2, density=1.0):
    a = rng.integers(-amp, amp + 1, shape).astype(np.float32)
    if density < 1.0:
        a *= rng.random(shape) < density
    return a


def grid_consts(rng, C, rows=5, scales=(1.0, -1.0, 2.0, -2.0), shift=1):
    """rows [rows][C]: row 0 = +-2^k scales, the others integers in [-shift, shift]."""
    c = rng.integers(-shift, shift + 1, (rows, C)).astype(np.float32)
    c[0] = rng.choice(np.asarray(scales, np.float32), C)
    return c


def sparse_filter(rng, Cout, Cin, taps=4, transposed=False):
    """[Cout][Cin][3][3] (or [Cin][Cout][3][3]) with at most `taps` non-zero entries per output channel, values in {-2..2}: the
    Winograd transform G g G^T of such a filter holds multiples of 1/4 only.  Every output channel has exactly ONE centre tap, with
    a positive weight (an input pixel whose eight neighbours are zero then reaches every output channel), the others lie off centre."""
    w = np.zeros((Cout, Cin, 9), np.float32)
    off = np.array([0, 1, 2, 3, 5, 6, 7, 8])
    for co in range(Cout):
        w[co, rng.integers(Cin), 4] = rng.choice(np.asarray([1.0, 2.0], np.float32))
        for _ in range(taps - 1):
            w[co, rng.integers(Cin), rng.choice(off)] = rng.choice(np.asarray([-2.0, -1.0, 1.0, 2.0], np.float32))
    w = w.reshape(Cout, Cin, 3, 3)
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)) if transposed else w


def winograd_filter(w):
    """U = G g G^T of F(2x2, 3x3) for a [Cout][Cin][3][3] filter, float64."""
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], F64)
    return np.einsum("ai,ocij,bj->ocab", G, _f(w), G)


def assert_exact(terms_abs_sum, q=1.0, what=""):
    """The integer-grid precondition: every column's sum of |term| is an integer multiple of q below 2^24 q."""
    s = _f(terms_abs_sum) / q
    assert np.all(s == np.round(s)), "%s: terms are no multiples of %g" % (what, q)
    assert np.all(s < 2.0 ** 24), "%s: sum of |terms| %.0f q reaches 2^24 q" % (what, float(s.max()))


def drop_masks(npix, second_pass_first):
    """The two single-pixel removals of the sensitivity check: the last pixel, and the first pixel of the second grid pass (the
    middle pixel where the plane fits one pass)."""
    idx = [npix - 1, second_pass_first if 0 < second_pass_first < npix - 1 else npix // 2]
    out = []
    for i in idx:
        k = np.ones(npix, bool)
        k[i] = False
        out.append(k)
    return idx, out
