"""Float64 restatement of RCV_OP_CLS_LABEL (csrc/cls_label.hip): the classifier tails of the four networks in their inference form --
class of a pixel = the FIRST maximum of its logits in class order, colour = palette[class] -- in the three source forms of the record
(features through the 1x1 classifier, the padded logits of the 3x3 classifier, a class map).  NumPy only; tests/test_segment.py pins it
to torch on the CPU, tests/test_gpu_segment.py compares the kernels with it.

The five palette rows are stated here (transform.py:139-156 cannot be imported where skimage and cv2 are absent)."""
import numpy as np

PLAIN, AFFINE, AFFINE_RELU = 0, 1, 5          # RCV_LOAD_* of the skip tensor
PALETTE5 = np.array([[0, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255]], np.uint8)
U = 2.0 ** -24


def palette8(rows=PALETTE5):
    """uint8 [8,3]: the palette as the device holds it (missing rows black)."""
    p = np.zeros((8, 3), np.uint8)
    p[:len(rows)] = rows
    return p


def form_input(t, tc=None, r=None, rc=None, mode2=PLAIN):
    """The classifier's input [.., CIN] in float64.  Plain: t itself.  Fused decoder output (RCV_F_FUSED_UP): relu(t * c0 + c1) plus
    f(r) on the first r.shape[-1] channels; tc = [>=2][CIN] rows (c0, c1), rc = [>=2][rch] rows of the skip's affine."""
    v = np.asarray(t, np.float64)
    if tc is None:
        return v
    tc = np.asarray(tc, np.float64)
    v = np.maximum(v * tc[0] + tc[1], 0.0)
    if r is not None:
        b = np.asarray(r, np.float64)
        if mode2 != PLAIN:
            rc = np.asarray(rc, np.float64)
            b = b * rc[0] + rc[1]
            if mode2 == AFFINE_RELU:
                b = np.maximum(b, 0.0)
        v = v.copy()
        v[..., :b.shape[-1]] += b
    return v


def logits_features(v, w, bias=None):
    """Source form 0: [.., CIN] x [COUT][CIN] (+ bias) -> [.., COUT]."""
    lg = np.asarray(v, np.float64) @ np.asarray(w, np.float64).T
    return lg if bias is None else lg + np.asarray(bias, np.float64)


def logits_padded(z, cout, bias=None):
    """Source form 1: the first `cout` of the floats of every pixel (+ bias)."""
    lg = np.asarray(z, np.float64)[..., :cout]
    return lg if bias is None else lg + np.asarray(bias, np.float64)


def first_argmax(lg):
    """uint8 [..]: the first maximum over the last axis, by the kernels' rule `lg[c] > mx` from -inf in class order: a NaN never
    wins, a pixel without any logit above -inf (all NaN) is class 0."""
    lg = np.asarray(lg, np.float64)
    return np.argmax(np.where(np.isnan(lg), -np.inf, lg), axis=-1).astype(np.uint8)          # np.argmax: the first of equal maxima


def first_argmax_loop(lg):
    """The same rule written as the kernels' loop (tests pin first_argmax to it)."""
    lg = np.asarray(lg, np.float64)
    flat = lg.reshape(-1, lg.shape[-1])
    out = np.zeros(len(flat), np.uint8)
    for i, row in enumerate(flat):
        mx, am = -np.inf, 0
        for c, x in enumerate(row):
            if x > mx:
                mx, am = x, c
        out[i] = am
    return out.reshape(lg.shape[:-1])


def colour_image(classes, palette=None):
    """uint8 [.., 3] = palette[class]; a class outside the palette's eight rows is black (source form 2 and the colour output)."""
    pal = palette8() if palette is None else palette8(np.asarray(palette, np.uint8))
    cls = np.asarray(classes).astype(np.int64)
    out = np.zeros(cls.shape + (3,), np.uint8)
    ok = (cls >= 0) & (cls < 8)
    out[ok] = pal[cls[ok]]
    return out


def colorize_five_masks(gray, n=5):
    """transform.py:158-170 literally: one boolean mask per colour-map row, three channel assignments each -> uint8 [3,H,W]."""
    gray = np.asarray(gray)
    cmap = np.zeros((n, 3), np.uint8)
    cmap[:min(n, 5)] = PALETTE5[:min(n, 5)]
    color_image = np.zeros((3,) + gray.shape, np.uint8)
    for label in range(0, len(cmap)):
        mask = gray == label
        color_image[0][mask] = cmap[label][0]
        color_image[1][mask] = cmap[label][1]
        color_image[2][mask] = cmap[label][2]
    return color_image


def top2_margin(lg):
    """Float64 gap between the two largest logits of every pixel (inf for one class)."""
    lg = np.asarray(lg, np.float64)
    if lg.shape[-1] < 2:
        return np.full(lg.shape[:-1], np.inf)
    s = np.sort(lg, axis=-1)
    return s[..., -1] - s[..., -2]


def margin_bound(v, w, bias, cin):
    """The fp32 dot-product bound of a pixel's logits: every logit is a chain of `cin` fused multiply-adds on an input that took at
    most three roundings to form (affine, skip affine, sum): |error| <= (cin + 3) 2^-24 (sum_k |v_k| |W_ck| + |b_c|); two logits can
    move towards each other, hence the factor 2.  A pixel whose float64 top-2 margin is at most this may change class in fp32."""
    mag = np.abs(np.asarray(v, np.float64)) @ np.abs(np.asarray(w, np.float64)).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, np.float64))
    return 2.0 * (cin + 3) * U * mag.max(axis=-1)


def exact_case(rng, shape, cin, cout, fused, mode2=PLAIN, rch=None):
    """Integer-grid operands (features in {-3..3}, weights and bias in {-2..2}, fused constants +-2^k and small integers): every logit
    is a multiple of 1/2 of a few hundred at most, exact in fp32 in any order.  From three classes on the last class repeats the first
    one's weights and bias (from four on the last but one repeats the second): wherever such a class leads, two logits tie exactly
    and the first must win; further ties come from the small grid by chance."""
    n = int(np.prod(shape))
    d = dict(t=rng.integers(-3, 4, (n, cin)).astype(np.float32), w=rng.integers(-2, 3, (cout, cin)).astype(np.float32),
             bias=rng.integers(-2, 3, cout).astype(np.float32), tc=None, r=None, rc=None, mode2=mode2)
    for twin in range(max(0, min(2, cout - 2))):
        d["w"][cout - 1 - twin] = d["w"][twin]
        d["bias"][cout - 1 - twin] = d["bias"][twin]
    if fused:
        rch = cin if rch is None else rch
        pw = lambda k: (2.0 ** rng.integers(-1, 2, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
        d["tc"] = np.stack([pw(cin), rng.integers(-2, 3, cin).astype(np.float32)] + [np.zeros(cin, np.float32)] * 3)
        d["r"] = rng.integers(-3, 4, (n, rch)).astype(np.float32)
        d["rc"] = np.stack([pw(rch), rng.integers(-2, 3, rch).astype(np.float32)] + [np.zeros(rch, np.float32)] * 3)
    return d


def random_case(rng, shape, cin, cout, fused, mode2=AFFINE, rch=None):
    """t, r ~ N(0,1); scale ~ U(0.5,1.5), shift ~ N(0,0.5); W ~ N(0,0.5), b ~ N(0,0.1)."""
    n = int(np.prod(shape))
    d = dict(t=rng.standard_normal((n, cin)).astype(np.float32), w=(0.5 * rng.standard_normal((cout, cin))).astype(np.float32),
             bias=(0.1 * rng.standard_normal(cout)).astype(np.float32), tc=None, r=None, rc=None, mode2=mode2)
    if fused:
        rch = cin if rch is None else rch
        rows = lambda k: np.stack([rng.uniform(0.5, 1.5, k), 0.5 * rng.standard_normal(k)] + [np.zeros(k)] * 3).astype(np.float32)
        d["tc"] = rows(cin)
        d["r"] = rng.standard_normal((n, rch)).astype(np.float32)
        d["rc"] = rows(rch)
    return d


def case_logits(d):
    """(input v, float64 logits) of a case dict."""
    v = form_input(d["t"], d["tc"], d["r"], d["rc"], d["mode2"])
    return v, logits_features(v, d["w"], d["bias"])
