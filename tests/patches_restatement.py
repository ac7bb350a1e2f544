"""NumPy restatement of the object-patch contract (RCV_OP_OBJECT_PATCHES, ``object_patches``): the box of every found object, cut out
of the full-resolution frame and brought to the patch classifiers' input.  A helper of the tests, not a test: tests/test_patches.py
pins steps 1-3 to live Pillow (``Image.resize((Sw, Sh), BILINEAR, box=...)``, byte for byte) and step 4 to
tests/rgb_prep_restatement.py; tests/test_gpu_patches.py pins the kernel to this file, bitwise.

Slot (n, c, k) of ``rows`` int32 [N][C-1][M][8] / ``counts`` int32 [N][C-1][4] (the layout of ``infer.Objects``; only rows[..., 0:4] =
x, y, w, h and counts[..., 3] = emitted are read) is valid iff k < min(counts[n][c][3], M).  For a valid slot:
  1. the box in class-map pixels (map H x W), every value clamped where it is used: x0 = clamp(x - margin, 0, W - 1),
     x1 = clamp(x + w + margin, x0 + 1, W); y0, y1 likewise with H;
  2. the box in frame pixels (frame Hs x Ws), float64, one division each: fx0 = (x0 Ws) / W, fx1 = (x1 Ws) / W, fy0 = (y0 Hs) / H,
     fy1 = (y1 Hs) / H;
  3. Pillow's 8-bit BILINEAR resize of that box of frame n to Sh x Sw: per axis precompute_coeffs with the box offset (``box_coeffs``),
     the horizontal pass first, the vertical pass second, each from 2^21, int32 sums, >> 22, clipped to a byte;
  4. rgb2yuv + ToTensor + Normalize([.5, 0, 0], [.5, .5, .5]) in float64, rounded once to float32 (rgb_prep_restatement.to_yuv).
An invalid slot is zero in every output."""
import numpy as np

from rgb_prep_restatement import to_yuv

PRECISION_BITS = 22


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def map_box(x, y, w, h, margin, H, W):
    """Step 1: (x0, y0, x1, y1) in class-map pixels, never empty, never outside the map, whatever the row holds."""
    x, y, w, h, margin = int(x), int(y), int(w), int(h), int(margin)
    x0 = clamp(x - margin, 0, W - 1)
    x1 = clamp(x + w + margin, x0 + 1, W)
    y0 = clamp(y - margin, 0, H - 1)
    y1 = clamp(y + h + margin, y0 + 1, H)
    return x0, y0, x1, y1


def frame_box(mb, H, W, Hs, Ws):
    """Step 2: (fx0, fy0, fx1, fy1), Python floats; int * int / int is one correctly rounded division."""
    x0, y0, x1, y1 = mb
    return x0 * Ws / W, y0 * Hs / H, x1 * Ws / W, y1 * Hs / H


def box_coeffs(in_size, in0, in1, out_size):
    """Pillow's precompute_coeffs(inSize, in0, in1, outSize) + normalize_coeffs_8bpc for the BILINEAR filter: per output index the
    first tap, the tap count and the 22-bit integer coefficients (lists of Python ints)."""
    scale = (in1 - in0) / out_size
    support = max(scale, 1.0)
    ss = 1.0 / support
    first, count, coef = [], [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        first.append(xmin)
        count.append(n)
        coef.append([int(0.5 + (v / ww if ww != 0.0 else v) * (1 << PRECISION_BITS)) for v in w])
    return first, count, coef


def resize_box(frame, fbox, size):
    """Step 3: uint8 [Hs][Ws][3], (fx0, fy0, fx1, fy1), (Sh, Sw) -> uint8 [Sh][Sw][3]."""
    Hs, Ws = frame.shape[:2]
    Sh, Sw = size
    fx0, fy0, fx1, fy1 = fbox
    xf, xn, xc = box_coeffs(Ws, fx0, fx1, Sw)
    yf, yn, yc = box_coeffs(Hs, fy0, fy1, Sh)
    r0, r1 = yf[0], yf[-1] + yn[-1]                      # the source rows the vertical pass reads
    src = frame[r0:r1].astype(np.int64)
    tmp = np.zeros((r1 - r0, Sw, 3), np.int64)
    for x in range(Sw):
        acc = (src[:, xf[x]:xf[x] + xn[x], :] * np.asarray(xc[x], np.int64)[None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
        tmp[:, x, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    out = np.zeros((Sh, Sw, 3), np.uint8)
    for y in range(Sh):
        a = yf[y] - r0
        acc = (tmp[a:a + yn[y]] * np.asarray(yc[y], np.int64)[:, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))
        out[y] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pillow_resize_box(frame, fbox, size):
    """The same through Pillow's own call."""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(frame)).resize((size[1], size[0]), Image.BILINEAR, box=tuple(fbox)))


def valid_slots(counts, M):
    """bool [N][C-1][M]: k < min(counts[..., 3], M)."""
    emitted = np.minimum(np.asarray(counts)[..., 3].astype(np.int64), M)
    return np.arange(M)[None, None, :] < emitted[..., None]


def object_patches(frames, rows, counts, map_size=None, size=(32, 32), margin=0, resize=resize_box):
    """frames uint8 [N][Hs][Ws][3], rows [N][C-1][M][8], counts [N][C-1][4] -> (images float32 [P][3][Sh][Sw], bytes uint8
    [P][Sh][Sw][3], valid bool [N][C-1][M]); P = N (C-1) M in the order of rows."""
    frames, rows, counts = np.asarray(frames), np.asarray(rows), np.asarray(counts)
    N, Hs, Ws, _ = frames.shape
    _, Cm1, M, _ = rows.shape
    H, W = (Hs, Ws) if map_size is None else map_size
    Sh, Sw = size
    valid = valid_slots(counts, M)
    P = N * Cm1 * M
    images = np.zeros((P, 3, Sh, Sw), np.float32)
    byts = np.zeros((P, Sh, Sw, 3), np.uint8)
    for n in range(N):
        for c in range(Cm1):
            for k in range(M):
                if not valid[n, c, k]:
                    continue
                p = (n * Cm1 + c) * M + k
                x, y, w, h = (int(v) for v in rows[n, c, k, 0:4])
                byts[p] = resize(frames[n], frame_box(map_box(x, y, w, h, margin, H, W), H, W, Hs, Ws), (Sh, Sw))
                images[p] = to_yuv(byts[p])
    return images, byts, valid


def edge_boxes(H, W):
    """(x, y, w, h) in a map of H x W (H >= 16, W >= 16): the whole map, 1 x 1, the four corners, the four edges, a 1 x H and a W x 1
    strip, and a 3 x 5 box (an up-scale for every patch size used here)."""
    return [(0, 0, W, H), (5, 7, 1, 1),
            (0, 0, 3, 4), (W - 3, 0, 3, 4), (0, H - 4, 3, 4), (W - 3, H - 4, 3, 4),
            (0, 9, 2, 5), (W - 2, 9, 2, 5), (10, 0, 6, 2), (10, H - 2, 6, 2),
            (11, 0, 1, H), (0, 13, W, 1), (8, 9, 3, 5)]


def random_boxes(rng, n, H, W):
    out = []
    for _ in range(n):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
    return out


def hand_built(H, W, N=2, Cm1=4, M=3, seed=5):
    """rows int32 [N][Cm1][M][8] and counts int32 [N][Cm1][4] made by hand: the edge boxes first, seeded boxes after them; the emitted
    counts cycle through M, M - 1, ..., 0 and one count is ABOVE M (min(count, M) decides); the rows past a count hold a different
    in-range box (they must give zeros); columns 4..7 hold junk that nobody may read."""
    rng = np.random.default_rng(seed)
    boxes = edge_boxes(H, W) + random_boxes(rng, N * Cm1 * M, H, W)
    rows = rng.integers(-1000, 1000, size=(N, Cm1, M, 8)).astype(np.int32)
    counts = rng.integers(0, 50, size=(N, Cm1, 4)).astype(np.int32)
    i = 0
    for n in range(N):
        for c in range(Cm1):
            emitted = (M - (n * Cm1 + c)) % (M + 1)
            counts[n, c, 3] = emitted
            for k in range(M):
                rows[n, c, k, 0:4] = boxes[i % len(boxes)] if k < emitted else boxes[-1 - (i % 7)]
                i += 1 if k < emitted else 0
    counts[N - 1, Cm1 - 1, 3] = M + 2
    for k in range(M):
        rows[N - 1, Cm1 - 1, k, 0:4] = boxes[(i + k) % len(boxes)]
    return rows, counts


def seeded_frames(seed, N, Hs, Ws):
    """uint8 [N][Hs][Ws][3]: smooth ramps plus noise, so that neighbouring taps differ and a wrong coefficient shows."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    base = np.stack([(xx * 255) // max(Ws - 1, 1), (yy * 255) // max(Hs - 1, 1), ((xx + yy) * 7) % 256], -1)[None]
    noise = rng.integers(-60, 61, size=(N, Hs, Ws, 3))
    return np.clip(base + noise, 0, 255).astype(np.uint8)
