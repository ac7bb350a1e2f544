"""numpy / float64 restatement of the three prune rules of RCV_OP_PRUNE (include/rcv.h; the reference's model.py:45-57 pruneModelNew,
:621-642 pruneModel, :644-672 pruneModel2), with the points the reference leaves open fixed as the project fixes them:

  rule 0  thresh = fp32(max|w| * fp32(ratio));  zero |w| < thresh;  mask = |w| < thresh afterwards
  rule 1  thresh0 = fp32(sqrt(sum((w - mean)^2) / (n - 1))), mean and sum in float64, two passes; then the reference's search
          (num = #(|w| < thresh) / #(w != 0) * 100; num < lower: thresh = fp32(thresh * fp32(1.025)); num > upper: fp32(thresh *
          fp32(0.975))), cut off after MAX_ITER steps (status 1, tensor untouched); no non-zero weight: status 2
  rule 2  zero the `amount` smallest |w|, compared as bit patterns; among equal magnitudes the LOWEST flat indices go;
          mask = (w == 0) afterwards

Every function takes a float32 array of any shape and returns copies; nothing here is shared with the code under test."""
import os

import numpy as np

MAX_ITER = 4096
ST_OK, ST_NO_END, ST_ALL_ZERO = 0, 1, 2

# the tensor list of tests/golden/prune.npz and tests/test_gpu_prune.py: 16 elements (pruneModel2's r = 0), 216 (< lT), a 1-D tensor
# that no rule may touch, 1023 / 1025 / 2049 elements (either side of a 1024-thread workgroup, not multiples of 4), 12 000 (> hT)
SHAPES = [(4, 4), (8, 3, 3, 3), (37,), (1023, 1), (1025, 1), (3, 683), (30, 400)]
RATIO0 = 0.1
LOWER, UPPER = 73, 77
RATIO2, RATIO2B, LT, HT = 0.3, 0.38, 300, 2000


def rule0(w, ratio):
    w = np.array(w, dtype=np.float32)
    thresh = np.float32(np.max(np.abs(w))) * np.float32(ratio)
    assert thresh.dtype == np.float32
    below = np.abs(w) < thresh
    n_below, n_nonzero = int(below.sum()), int((w != 0).sum())
    w[below] = 0
    return w, np.abs(w) < thresh, thresh, n_below, n_nonzero


def std32(w):
    d = np.asarray(w, dtype=np.float64).reshape(-1)
    mean = d.sum() / d.size
    return np.float32(np.sqrt(((d - mean) ** 2).sum() / (d.size - 1)))


def rule1(w, lower, upper, max_iter=MAX_ITER):
    """-> (w, mask, thresh, n_below, n_nonzero, steps, status)"""
    w = np.array(w, dtype=np.float32)
    assert w.size >= 2
    thresh = std32(w)
    up, down = np.float32(1.025), np.float32(0.975)
    a = np.abs(w)
    n_nonzero = int((w != 0).sum())
    steps, n_below = 0, 0
    status = ST_NO_END
    while steps < max_iter:
        n_below = int((a < thresh).sum())
        if n_nonzero == 0:
            status = ST_ALL_ZERO
            break
        num = float(n_below) / float(n_nonzero) * 100
        if num < lower:
            thresh = np.float32(thresh * up)
        elif num > upper:
            thresh = np.float32(thresh * down)
        else:
            status = ST_OK
            break
        steps += 1
    if status != ST_OK:
        return w, None, thresh, n_below, n_nonzero, steps, status
    w[a < thresh] = 0
    return w, np.abs(w) < thresh, thresh, n_below, n_nonzero, steps, status


def amount_for(n, ratio, lT, hT):
    """model.py:649-660"""
    r = ratio
    if n < 100:
        r = 0
    elif n < lT:
        r = ratio * 0.8
    if n > hT:
        r = ratio * 1.05
    return int(n * r)


def rule2(w, amount):
    w = np.array(w, dtype=np.float32)
    flat = w.reshape(-1)
    assert 0 <= amount <= flat.size
    keys = flat.view(np.uint32) & np.uint32(0x7FFFFFFF)
    order = np.argsort(keys, kind="stable")          # equal keys stay in index order: the lowest indices come first
    flat[order[:amount]] = 0
    return w, w == 0


def tie_free(rng, shape):
    """Seeded normal fp32 values, no two of equal magnitude and none zero (so that torch.topk's answer is unique)."""
    n = int(np.prod(shape))
    v = rng.standard_normal(n).astype(np.float32)
    while True:
        a = np.abs(v)
        _, first = np.unique(a, return_index=True)
        dup = np.ones(n, dtype=bool)
        dup[first] = False
        dup |= a == 0
        if not dup.any():
            return v.reshape(shape)
        v[dup] = rng.standard_normal(int(dup.sum())).astype(np.float32)


def grid_weights(seed, shape):
    """Heavy ties: every value from a grid of 16 magnitudes (both signs, some exact zeros)."""
    rng = np.random.default_rng(seed)
    grid = np.concatenate([[0.0], np.linspace(0.05, 0.75, 15)]).astype(np.float32)
    v = grid[rng.integers(0, 16, size=int(np.prod(shape)))] * rng.choice(np.float32([-1, 1]), size=int(np.prod(shape)))
    return v.astype(np.float32).reshape(shape)


def oscillating_tensor():
    """A two-value tensor on which pruneModel's search never ends: 100 weights of magnitude 1 and 100 of magnitude 1.01 (signs
    alternate, so the mean is 0).  #(|w| < t) / 200 is 0 %, 50 % or 100 %, never inside [73, 77]: the threshold climbs until it
    passes 1.01, steps back below it, and so on."""
    v = np.empty(200, dtype=np.float32)
    v[:100] = 1.0
    v[100:] = 1.01
    v[::2] *= -1
    return v.reshape(20, 10)


def load_golden():
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", "prune.npz"))
