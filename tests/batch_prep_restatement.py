"""NumPy / torch-CPU restatement of the reference's per-image batch preparation (dataset.py:107-133 ``SSYUVDataset.__getitem__``,
dataset.py:19-39 ``ColorJitter``, transform.py:26-49 ``maskLabel``).  A helper of the tests, not a test: tests/test_batch_prep.py pins
it to live Pillow and to the goldens, tests/test_gpu_batch_prep.py pins the kernel to it.

The resize restates Pillow's 8-bit path (checked against Pillow 12.2.0): ``precompute_coeffs`` in double, the coefficients as 22-bit
integers rounded half away from zero, a horizontal pass rounded to uint8 and then a vertical pass, each ``(acc + 2^21) >> 22`` clipped
to 0..255; a pass whose two sizes are equal is skipped.  Mode-``I`` labels take the NEAREST index rule of the affine scaler:
``xo = a0 * 0.5; tab[x] = int(xo); xo += a0`` with the additions accumulated in double."""
import math

import numpy as np
import torch

PRECISION_BITS = 22
MEAN = {False: [0.36269532, 0.41144562, 0.282713], True: [0.34190056, 0.4833289, 0.48565758]}      # dataset.py:74  (key: finetune)
STD = {False: [0.31111388, 0.21010718, 0.34060917], True: [0.47421749, 0.13846053, 0.1714848]}     # dataset.py:75

# (Hs, Ws) -> (H, W): the pairs on which the restatement was compared with Image.resize byte for byte
SHAPE_PAIRS = [((480, 640), (120, 160)), ((480, 640), (240, 320)), ((480, 640), (96, 128)), ((480, 640), (100, 150)),
               ((17, 640), (17, 160)), ((97, 131), (40, 33)), ((50, 70), (75, 100)), ((33, 47), (32, 46)), ((61, 19), (7, 3))]

FLAG_SETS = [(bool(k & 1), bool(k & 2), bool(k & 4), bool(k & 8)) for k in range(16)]      # (no_ball, no_robot, no_goal, no_line)


def bilinear_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter over the whole axis: (first[out], count[out],
    coef[out][ksize]) with int32 coefficients (zero beyond count)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        first[xx], count[xx] = xmin, xmax
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return first, count, coef


def nearest_index(in_size, out_size):
    """The source index of every output index of Pillow's NEAREST resize (ImagingScaleAffine)."""
    a0 = float(in_size) / out_size
    tab = np.zeros(out_size, np.int32)
    xo = a0 * 0.5
    for x in range(out_size):
        tab[x] = int(xo)
        xo += a0
    assert tab.min() >= 0 and tab.max() < in_size
    return tab


def _pass(img, first, count, coef, axis):
    """One integer pass over `axis` (0 = vertical, 1 = horizontal) of a uint8 [H][W][C] image."""
    src = img.astype(np.int64)
    n = len(first)
    shape = list(img.shape)
    shape[axis] = n
    out = np.zeros(shape, np.uint8)
    for o in range(n):
        acc = np.full(shape[:axis] + shape[axis + 1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(int(count[o])):
            acc = acc + np.take(src, int(first[o]) + k, axis=axis) * int(coef[o, k])
        v = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        if axis == 0:
            out[o] = v
        else:
            out[:, o] = v
    return out


def resize_bilinear(img, size):
    """Image.resize(size[::-1], BILINEAR) of a uint8 [Hs][Ws][C] image; size = (H, W)."""
    H, W = size
    if img.shape[1] != W:
        img = _pass(img, *bilinear_coeffs(img.shape[1], W), axis=1)
    if img.shape[0] != H:
        img = _pass(img, *bilinear_coeffs(img.shape[0], H), axis=0)
    return img


def resize_nearest(lab, size):
    """Image.resize(size[::-1], NEAREST) of a [Hs][Ws] label plane."""
    H, W = size
    if lab.shape == (H, W):
        return lab
    return lab[nearest_index(lab.shape[0], H)][:, nearest_index(lab.shape[1], W)]


def norm_table(finetune=False):
    """to_tensor + Normalize of every byte value, per channel: float32 [3][256], made with the same torch calls."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN[bool(finetune)], dtype=torch.float32)
    std = torch.as_tensor(STD[bool(finetune)], dtype=torch.float32)
    return ((v[None, :] - mean[:, None]) / std[:, None]).contiguous()


def mask_label(label, nb, nr, ng, nl):
    """transform.py:26-49 on an integer array, statement for statement (a copy is returned)."""
    label = label.copy()
    bNum, rNum, gNum, lNum = 1, 2, 3, 4
    if nb:
        label[label == bNum] = 0
        label[label > bNum] -= 1
        rNum, gNum, lNum = 1, 2, 3
    if nr:
        label[label == rNum] = 0
        label[label > rNum] -= 1
        gNum, lNum = 1, 2
    if ng:
        label[label == gNum] = 0
        label[label > gNum] -= 1
        lNum = 1
    if nl:
        label[label == lNum] = 0
    return label


def prepare_image(frame, label, size, finetune=False, train=False, row=None, flags=(False, False, False, False), exact_uv=False):
    """One image through the pipeline: uint8 [Hs][Ws][3], integer [Hs][Ws] -> (float32 [3][H][W], int64 [H][W]).  `row` = the
    parameter row {flip, b, c, m00, m01, m10, m11, uv_off} of ``draw_jitter``.  exact_uv: U / V come back as float64, the exact products
    summed in double (the value both the fused and the unfused fp32 forms are within 2^-23 (|m0 U| + |m1 V|) of)."""
    H, W = size
    if frame.shape[:2] != (H, W):
        frame = resize_bilinear(frame, size)
        label = resize_nearest(label, size)
    tab = norm_table(finetune).numpy()
    img = np.stack([tab[c][frame[:, :, c]] for c in range(3)])
    lab = label.astype(np.int64)
    uv64 = None
    if train:
        row = np.asarray(row, np.float32)
        if row[0] != 0:
            img = img[:, :, ::-1]
            lab = lab[:, ::-1]
        img = img.copy()
        img[0] = (img[0] + row[1]) * row[2]
        if row[7] == 0:
            u, v = img[1].copy(), img[2].copy()
            if exact_uv:
                u64, v64 = u.astype(np.float64), v.astype(np.float64)
                uv64 = np.stack([float(row[3]) * u64 + float(row[4]) * v64, float(row[5]) * u64 + float(row[6]) * v64])
            img[1] = row[3] * u + row[4] * v
            img[2] = row[5] * u + row[6] * v
        elif exact_uv:
            uv64 = img[1:].astype(np.float64)
    lab = mask_label(np.ascontiguousarray(lab), *flags)
    if exact_uv:
        return np.ascontiguousarray(img), lab, uv64
    return np.ascontiguousarray(img), lab


def uv_bound(frame_resized, finetune, row, flip):
    """|m0 U| + |m1 V| per output element of channels 1 and 2 (float64 [2][H][W]): the scale of the U / V tolerance."""
    tab = norm_table(finetune).numpy().astype(np.float64)
    u, v = np.abs(tab[1][frame_resized[:, :, 1]]), np.abs(tab[2][frame_resized[:, :, 2]])
    if flip:
        u, v = u[:, ::-1], v[:, ::-1]
    row = np.asarray(row, np.float32).astype(np.float64)
    return np.stack([abs(row[3]) * u + abs(row[4]) * v, abs(row[5]) * u + abs(row[6]) * v])


def prepare_batch(frames, labels, size, finetune=False, train=False, params=None, flags=(False, False, False, False)):
    """The batch the loader + train.py:43-46 hand to the network: (float32 [B][3][H][W], int64 [B][H][W])."""
    outs = [prepare_image(frames[b], labels[b], size, finetune, train, None if params is None else params[b], flags)
            for b in range(len(frames))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def synthetic_frames(B, Hs, Ws, seed, full_range_labels=False, cover_size=None):
    """Seeded frames (smooth gradients + blocks + noise, all byte values occur) and label planes (classes 0..4 in blobs, or every
    value 0..255 when full_range_labels, see cover_size): (uint8 [B][Hs][Ws][3], int32 [B][Hs][Ws])."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    frames = np.zeros((B, Hs, Ws, 3), np.uint8)
    labels = np.zeros((B, Hs, Ws), np.int32)
    for b in range(B):
        for c in range(3):
            g = (xx * rng.randint(1, 7) + yy * rng.randint(1, 7) + rng.randint(0, 256)) % 256
            blocks = rng.randint(0, 256, size=((Hs + 7) // 8, (Ws + 7) // 8))
            blk = np.kron(blocks, np.ones((8, 8), np.int64))[:Hs, :Ws]
            noise = rng.randint(0, 256, size=(Hs, Ws))
            pick = rng.randint(0, 3, size=(Hs, Ws))
            frames[b, :, :, c] = np.where(pick == 0, g, np.where(pick == 1, blk, noise)).astype(np.uint8)
        if full_range_labels:
            labels[b] = rng.randint(0, 256, size=(Hs, Ws))
            # every value occurs, in the plane and (where it has 256 pixels) in the plane's NEAREST resize to cover_size
            H, W = cover_size or (Hs, Ws)
            ys, xs = (np.arange(Hs), np.arange(Ws)) if (H, W) == (Hs, Ws) else (nearest_index(Hs, H), nearest_index(Ws, W))
            perm = np.concatenate([rng.permutation(256) for _ in range((H * W + 255) // 256)])[:H * W].reshape(H, W)
            labels[b][np.ix_(ys, xs)] = perm
        else:
            cells = rng.randint(0, 5, size=((Hs + 4) // 5, (Ws + 4) // 5))
            labels[b] = np.kron(cells, np.ones((5, 5), np.int64))[:Hs, :Ws]
    return frames, labels
