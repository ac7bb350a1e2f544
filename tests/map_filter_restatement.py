"""RCV_OP_MAP_FILTER (include/rcv.h, csrc/map_filter.hip) and the five public functions of ``infer.py`` that use it, restated in
numpy the literal way: one pass over the window's offsets per count, a plain comparison per class, no packing.

A value v of a map is a class when 0 <= v < C, else void.  For a window k the offsets on each axis are -(k // 2) ... k - 1 - k // 2;
pixels outside the image are not in the window (labelExtraction.py:76,79's ``continue``); h[c] counts the in-image pixels of class c,
n the in-image pixels.  ``majority_literal`` is labelExtraction.py:70-89 itself, loop for loop, for small planes."""
import numpy as np

VOID_BIT = 1 << 8      # close_finish's over set: the bit of the void pixels


def is_class(m, C):
    m = np.asarray(m)
    return (m.astype(np.int64) >= 0) & (m.astype(np.int64) < C)


def _window_sum(planes, k):
    """planes int64 [..., H, W] -> the sum over the in-image pixels of every pixel's window."""
    H, W = planes.shape[-2:]
    out = np.zeros_like(planes)
    r0 = k // 2
    for i in range(-r0, k - r0):
        ya, yb = max(0, -i), min(H, H - i)
        if ya >= yb:
            continue
        for j in range(-r0, k - r0):
            xa, xb = max(0, -j), min(W, W - j)
            if xa >= xb:
                continue
            out[..., ya:yb, xa:xb] += planes[..., ya + i:yb + i, xa + j:xb + j]
    return out


def window_counts(m, C, k):
    """h int64 [C, N, H, W], n int64 [N, H, W] of a class map [N, H, W]."""
    m = np.asarray(m).astype(np.int64)
    h = _window_sum(np.stack([(m == c).astype(np.int64) for c in range(C)]), k)
    return h, _window_sum(np.ones_like(m), k)


def bit_counts(b, C, k):
    """The same per bit of a bit map: [C, N, H, W] and n."""
    b = np.asarray(b).astype(np.int64)
    return _window_sum(np.stack([(b >> c) & 1 for c in range(C)]), k), _window_sum(np.ones_like(b), k)


def _own(h, m, C):
    isc = is_class(m, C)
    v = np.where(isc, np.asarray(m).astype(np.int64), 0)
    return isc, v, np.take_along_axis(h, v[None], 0)[0] * isc


def _in_set(S, v):
    return ((S >> v) & 1).astype(bool)


def _majority_branches(h, m, C, min_major, min_own, fill_void):
    isc, _, own = _own(h, m, C)
    looked = isc | bool(fill_void)
    major = looked & (h.max(0) >= min_major)
    few = looked & ~major & isc & (own < min_own)
    return major, few, looked & ~major & ~few


def majority_branches(m, C, k, min_major, min_own, fill_void=False):
    """The three branches of the rule as masks: (by majority, by too few of its own, kept), over the pixels the rule looks at."""
    return _majority_branches(window_counts(m, C, k)[0], m, C, min_major, min_own, fill_void)


def majority(m, C, k, min_major, min_own, fill_void=False):
    m = np.asarray(m)
    h, _ = window_counts(m, C, k)
    major, few, _ = _majority_branches(h, m, C, min_major, min_own, fill_void)
    return np.where(major | few, h.argmax(0), m).astype(m.dtype)      # argmax: the first, i.e. lowest, class attaining the maximum


def majority_literal(mask, C=5, k=4, min_major=15, min_own=7):
    """labelExtraction.py:70-89 for one plane of classes (no void), any size and window: the loops as written there."""
    mask = np.asarray(mask)
    H, W = mask.shape
    new = np.empty((H, W), dtype=mask.dtype)
    r0 = k // 2
    for row in range(H):
        for col in range(W):
            hist = np.zeros(C)
            for i in range(-r0, k - r0, 1):
                if row + i < 0 or row + i >= H:
                    continue
                for j in range(-r0, k - r0, 1):
                    if col + j < 0 or col + j >= W:
                        continue
                    hist[mask[(row + i, col + j)]] += 1
            if np.amax(hist) >= min_major or hist[mask[(row, col)]] < min_own:
                new[(row, col)] = np.argmax(hist)
            else:
                new[(row, col)] = mask[(row, col)]
    return new


def erode(m, C, k, S, fill):
    m = np.asarray(m)
    h, n = window_counts(m, C, k)
    isc, v, own = _own(h, m, C)
    return np.where(isc & _in_set(S, v) & (own < n), fill, m).astype(m.dtype)


def erode_bits(m, C, k, S):
    h, n = window_counts(m, C, k)
    isc, v, own = _own(h, m, C)
    return np.where(isc & _in_set(S, v) & (own == n), 1 << v, 0).astype(np.uint8)


def dilate_bits(m, C, k, S):
    h, _ = window_counts(m, C, k)
    out = np.zeros(h.shape[1:], dtype=np.int64)
    for c in range(C):
        if (S >> c) & 1:
            out |= np.where(h[c] > 0, 1 << c, 0)
    return out.astype(np.uint8)


def open_finish(bits, m, C, k, S, fill):
    m = np.asarray(m)
    h, _ = bit_counts(np.asarray(bits).astype(np.int64) & S, C, k)
    isc, v, lane = _own(h, m, C)
    return np.where(isc & _in_set(S, v) & (lane == 0), fill, m).astype(m.dtype)


def close_finish(bits, m, C, k, S, O):
    m = np.asarray(m)
    h, n = bit_counts(np.asarray(bits).astype(np.int64) & S, C, k)
    isc = is_class(m, C)
    v = np.where(isc, m.astype(np.int64), 8)
    claim = _in_set(O, v)
    out = m.astype(np.int64).copy()
    done = np.zeros(m.shape, dtype=bool)
    for c in range(C):
        if (S >> c) & 1:
            take = ~done & (h[c] == n) & (claim | (isc & (v == c)))
            out[take] = c
            done |= take
    return out.astype(m.dtype)


# ------------------------------------------------------------------------------------------------------------ the public functions
def _set(classes, default):
    bits = 0
    for c in (default if classes is None else classes):
        bits |= 1 << c
    return bits


def majority_filter(m, num_class=5, window=4, min_major=15, min_own=7, fill_void=False):
    return majority(m, num_class, window, min_major, min_own, fill_void)


def erode_map(m, num_class, classes=None, window=3, fill=0):
    return erode(m, num_class, window, _set(classes, range(num_class)), fill)


def open_map(m, num_class, classes=None, window=3, fill=0):
    S = _set(classes, range(num_class))
    return open_finish(erode_bits(m, num_class, window, S), m, num_class, window, S, fill)


def close_map(m, num_class, classes=None, window=3, over=(0,), over_void=True):
    S = _set(classes, range(1, num_class))
    return close_finish(dilate_bits(m, num_class, window, S), m, num_class, window, S, _set(over, ()) | (VOID_BIT if over_void else 0))


def trim_pseudo_labels(pseudo, num_class, window=3):
    return erode_map(pseudo, num_class, None, window, fill=-100)


def changed(before, after):
    """int [N]: the pixels of every image whose value changed."""
    return (np.asarray(before).astype(np.int64) != np.asarray(after).astype(np.int64)).reshape(len(before), -1).sum(1)


# ------------------------------------------------------------------------------------------------------------------- test data
def void_values(dtype):
    """Values that are no class of any map of up to 8 classes: 255 and bytes >= C for uint8; -100, 255, 8 ... and one beyond 32 bits."""
    return [255, 8, 200] if np.dtype(dtype) == np.uint8 else [-100, 255, 8, -1, (1 << 32) + 1]


def blobby_map(rng, N, H, W, C, dtype, p_noise=0.04, p_void=0.03):
    """Class maps with structure: rectangles and discs of random classes over background 0, a fraction of speckle pixels of random
    class, a fraction of void pixels -- single ones and a few void rectangles (the -100 holes of a pseudo-label map)."""
    out = np.zeros((N, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for n in range(N):
        for _ in range(max(3, H * W // 150)):
            c = int(rng.integers(0, C))
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            ry, rx = int(rng.integers(1, max(2, H // 3))), int(rng.integers(1, max(2, W // 3)))
            if rng.random() < 0.5:
                sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
            else:
                sel = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            out[n][sel] = c
    noise = rng.random(out.shape) < p_noise
    out[noise] = rng.integers(0, C, size=int(noise.sum()))
    voids = np.array(void_values(dtype), dtype=np.int64)
    voids = np.concatenate([voids, np.arange(C, 8)]) if C < 8 else voids
    hole = rng.random(out.shape) < p_void
    for n in range(N):
        for _ in range(2):
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            hole[n, cy:cy + int(rng.integers(1, 6)), cx:cx + int(rng.integers(1, 6))] = True
    out[hole] = voids[rng.integers(0, len(voids), size=int(hole.sum()))]
    return out.astype(dtype)
