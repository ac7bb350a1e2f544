"""NumPy restatement of the two records a device-resident dataset runs on (RCV_OP_RESIZE_U8, RCV_OP_BATCH_PREP_IDX), in terms of
tests/batch_prep_restatement.py.  A helper of the tests, not a test: tests/test_resident.py pins it to live Pillow and to the batch
restatement, tests/test_gpu_resident.py pins the kernels to it.

``resize_u8`` is the resize stage of the batch restatement and nothing else: the bytes its normalisation lookup reads, and the labels
gathered and not masked.  ``prepare_batch_indexed`` is the batch restatement whose image ``b`` is ``store[index[b]]``, image by image
(no fancy indexing: the test compares it with the batch restatement on ``store[index]``); an index outside ``[0, N)`` gives a zero
image with zero targets and is counted."""
import numpy as np

import batch_prep_restatement as R

# (Hs, Ws) -> (H, W): 9 taps per column (staged) across a column tile and a row tile; 5 taps (through the cache); rows of 111 bytes;
# no resize (a copy)
SHAPES = [((44, 280), (11, 70)), ((22, 140), (11, 70)), ((45, 37), (13, 10)), ((11, 70), (11, 70))]


def resize_u8(frames, labels, size, label_dtype=None):
    """uint8 [B][Hs][Ws][3], integer [B][Hs][Ws] (or None) -> (uint8 [B][H][W][3], labels [B][H][W] of label_dtype or the input's)."""
    H, W = size
    out = np.stack([f if f.shape[:2] == (H, W) else R.resize_bilinear(f, size) for f in frames])
    if labels is None:
        return out, None
    lab = np.stack([R.resize_nearest(p, size) for p in labels])
    return out, lab.astype(label_dtype or labels.dtype)


def prepare_batch_indexed(frames, labels, index, size, finetune=False, train=False, params=None, flags=(False, False, False, False)):
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
        imgs[b], tgt[b] = R.prepare_image(frames[src], labels[src], size, finetune, train, None if params is None else params[b], flags)
    return imgs, tgt, bad
