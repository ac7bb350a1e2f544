"""NumPy restatement of the two records that read a device-resident store through an index for the RGB loader (RCV_OP_RGB_PREP_IDX,
RCV_OP_LP_PAIR_PREP), in terms of tests/rgb_prep_restatement.py and tests/labelprop_restatement.py.  A helper of the tests, not a
test: tests/test_rgb_resident.py pins it to the batch restatement (and shows that the pair form tells three wrong variants apart),
tests/test_gpu_rgb_resident.py pins the kernels to it.

``prepare_rgb_indexed`` is the batch restatement whose image ``b`` is ``store[index[b]]``, image by image (no fancy indexing: the test
compares it with the batch restatement on ``store[index]``).  ``prepare_lp_pairs`` takes both frames and both label planes of pair ``p``
through ``prepare_image`` with ONE row -- the same mirrors for all four planes, the same colour operations on both frames, the contrast
mean of each frame on its own (``prepare_image`` works on one image) -- and assembles them with ``assemble_np``.  An index (a pair with
either index) outside ``[0, N)`` gives zeros and is counted once."""
import numpy as np

import labelprop_restatement as LR
import rgb_prep_restatement as R

NO_FLAGS = (False, False, False, False)


def prepare_rgb_indexed(frames, labels, index, size, train=False, params=None, flags=NO_FLAGS, pillow=False):
    """(float32 [B][3][H][W], int64 [B][H][W], number of indices outside the store); B = len(index), params has B rows."""
    H, W = size
    N = len(frames)
    imgs = np.zeros((len(index), 3, H, W), np.float32)
    tgt = np.zeros((len(index), H, W), np.int64)
    bad = 0
    for b, src in enumerate(int(v) for v in index):
        if not 0 <= src < N:
            bad += 1
            continue
        imgs[b], tgt[b] = R.prepare_image(frames[src], labels[src], size, train, None if params is None else params[b], flags, pillow)
    return imgs, tgt, bad


def prepare_lp_pairs(frames, labels, pairs, train=False, params=None, pillow=False, variant=None):
    """Store uint8 [N][H][W][3] / integer [N][H][W], pairs [B][2], params [B][12] (one row per pair) -> (inputs float32 [2B][8][H][W],
    targets int64 [2B][H][W], pairs refused).  ``variant`` names a deliberately WRONG form (the tests show that equality tells each from
    the right one): "pooled_mean" -- the contrast mean of both frames together; "own_label" -- class channels from the frame's own label
    instead of the other frame's; "vflip_a_only" -- the vertical flip applied to frame a only."""
    N, H, W, _ = frames.shape
    B = len(pairs)
    x = np.zeros((2 * B, 8, H, W), np.float32)
    t = np.zeros((2 * B, H, W), np.int64)
    bad = 0
    for p, (ia, ib) in enumerate((int(v[0]), int(v[1])) for v in pairs):
        if not (0 <= ia < N and 0 <= ib < N):
            bad += 1
            continue
        row = None if params is None else np.asarray(params[p], np.float32)
        row_b = row
        if variant == "vflip_a_only" and train:
            row_b = row.copy()
            row_b[1] = 0
        if variant == "pooled_mean" and train:
            # both frames as ONE image of 2H rows: the contrast mean is taken over both (flips first, so the halves stay where they are)
            both = np.concatenate([_flipped(frames[ia], row), _flipped(frames[ib], row)])
            plain = row.copy()
            plain[0] = plain[1] = 0
            y = R.prepare_image(both, None, (2 * H, W), True, plain, NO_FLAGS, pillow)[0]
            imgs = np.stack([y[:, :H], y[:, H:]])
            tg = np.stack([_flipped(labels[ia], row), _flipped(labels[ib], row)]).astype(np.int64)
        else:
            ia_out = R.prepare_image(frames[ia], labels[ia], (H, W), train, row, NO_FLAGS, pillow)
            ib_out = R.prepare_image(frames[ib], labels[ib], (H, W), train, row_b, NO_FLAGS, pillow)
            imgs, tg = np.stack([ia_out[0], ib_out[0]]), np.stack([ia_out[1], ib_out[1]])
        xs, ts = LR.assemble_np(imgs[None], tg[None])
        if variant == "own_label":
            xs[[0, 1], 3:] = xs[[1, 0], 3:]
        x[2 * p:2 * p + 2], t[2 * p:2 * p + 2] = xs, ts
    return x, t, bad


def _flipped(a, row):
    if row[0] != 0:
        a = a[:, ::-1]
    if row[1] != 0:
        a = a[::-1]
    return np.ascontiguousarray(a)
