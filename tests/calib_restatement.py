"""RCV_OP_CLS_CALIB (include/rcv.h, csrc/cls_calib.hip) and ``metrics.calibration_report`` restated in numpy, from what
RCV_OP_CLS_PROBA stores: the uint8 class of a pixel, its fp32 confidence, and the int64 target.

  bin   = #{ j : cf >= edges[j] } on fp32 values, in 0..K
  q     = trunc(fp32(cf * 2^26)) -- the product of an fp32 and a power of two is exact
  table[bin][cls][t] += 1, table[bin][cls][C + 1] += q      where 0 <= t < C on the int64 value
  table[bin][cls][C] += 1, table[bin][cls][C + 2] += q      otherwise, and without targets
  a NaN confidence and a class byte >= C count nowhere.

``table(..., variant=...)`` states the wrong rules a test must tell apart from the right one."""
import numpy as np

Q_SCALE = 2 ** 26
VARIANTS = ("gt", "round", "transposed", "outside_in_label_column", "low32", "nan_in_bin0")


def bin_index(conf, edges, strict=False):
    """int64 per pixel (flattened); the comparison of a NaN is false, so a NaN lands in bin 0 here (``table`` drops it)."""
    cf = np.asarray(conf, np.float32).reshape(-1)
    e = np.asarray(edges, np.float32).reshape(-1)
    assert cf.dtype == np.float32 and e.dtype == np.float32 and 1 <= e.size <= 32
    with np.errstate(invalid="ignore"):
        hit = (cf[:, None] > e[None, :]) if strict else (cf[:, None] >= e[None, :])
    return hit.sum(1).astype(np.int64)


def fixed_point(conf, rounding=False):
    """uint64 per pixel: trunc(fp32(cf * 2^26)); NaN -> 0 (never counted)."""
    cf = np.asarray(conf, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        prod = cf * np.float32(Q_SCALE)
    assert prod.dtype == np.float32
    prod = np.where(np.isnan(prod), np.float32(0), prod).astype(np.float64)
    return (np.floor(prod + 0.5) if rounding else np.floor(prod)).astype(np.uint64)          # (confidences are >= 0: floor truncates)


def table(cls_u8, conf, targets, edges, C, variant=None):
    """int64 [K + 1][C][C + 3] of one pass over the pixels (any shape; ``targets`` None: no pixel has a label)."""
    assert variant is None or variant in VARIANTS
    cls = np.asarray(cls_u8).reshape(-1).astype(np.int64)
    cf = np.asarray(conf, np.float32).reshape(-1)
    K = int(np.asarray(edges).size)
    t = np.full(cls.shape, -1, np.int64) if targets is None else np.asarray(targets, np.int64).reshape(-1)
    assert cls.shape == cf.shape == t.shape
    b = bin_index(cf, edges, strict=variant == "gt")
    q = fixed_point(cf, rounding=variant == "round").astype(np.int64)
    if variant == "low32":
        t = (t & 0xFFFFFFFF).astype(np.uint32).astype(np.int32).astype(np.int64)          # what a 32-bit read of the target sees
    counted = cls < C
    if variant != "nan_in_bin0":
        counted &= ~np.isnan(cf)
    lab = (t >= 0) & (t < C)
    if variant == "outside_in_label_column":
        col = np.where(lab, t, np.clip(t, 0, C - 1))
        lab = np.ones_like(lab)
    else:
        col = np.where(lab, t, C)
    out = np.zeros((K + 1, C, C + 3), np.int64)
    m = counted
    if variant == "transposed":
        both = m & lab
        np.add.at(out, (b[both], t[both], cls[both]), 1)
        np.add.at(out, (b[both], t[both], C + 1), q[both])
        m = m & ~lab
    np.add.at(out, (b[m], cls[m], col[m]), 1)
    np.add.at(out, (b[m], cls[m], np.where(lab[m], C + 1, C + 2)), q[m])
    return out


HAND_EDGES = np.array([0.0, 0.1, 0.5, 0.9, 1.0], np.float32)


def handmade_maps(shape, C, edges=HAND_EDGES, seed=68):
    """A class map, a confidence map and targets that hold every case the rules speak of: confidences equal to an edge and one ulp
    below it, 0, 1, NaN, small ones whose fixed-point image has a fraction of a half or more (fp32(0.1) * 2^26 = 6710886.5), class
    bytes >= C, and the targets -100, -1, C and 2^32 + c among labels that agree with the class about two times in three."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    e = np.asarray(edges, np.float32)
    special = [np.float32(0.0), np.float32(1.0), np.float32(np.nan), np.float32(0.1), np.float32(0.07), np.float32(0.3)]
    special += list(e) + [np.nextafter(v, np.float32(-1.0)) for v in e if v > 0]
    special = np.array(special, np.float32)
    conf = rng.uniform(0.0, 1.0, n).astype(np.float32)
    pick = rng.random(n) < 0.5
    conf[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    conf[: special.size] = special                                     # every special value at least once, whatever the draw
    cls = rng.integers(0, C, n).astype(np.uint8)
    bad = rng.random(n) < 0.04
    cls[bad] = np.array([C, 255], np.uint8)[rng.integers(0, 2, int(bad.sum()))]
    t = np.where(rng.random(n) < 0.66, cls.astype(np.int64) % C, rng.integers(0, C, n))
    odd = rng.random(n) < 0.2
    t[odd] = np.array([-100, -1, C, 2 ** 32, 2 ** 32 + C - 1], np.int64)[rng.integers(0, 5, int(odd.sum()))]
    # the special confidences meet a class inside the range, labelled and unlabelled alike
    k = special.size
    cls[:k] = np.arange(k) % C
    t[:k] = np.where(np.arange(k) % 3 == 0, -100, (np.arange(k) + np.arange(k) // 2) % C)
    cls[k:k + 3], conf[k:k + 3], t[k:k + 3] = (C, 255, 0), (0.95, 0.95, 0.95), (0, 0, 2 ** 32)
    if n > k + 8:
        cls[k + 3:k + 8] = 0
        conf[k + 3:k + 8] = np.float32(0.1)
        t[k + 3:k + 8] = (C - 1, -100, C, 2 ** 32 + C - 1, 0)
    return cls.reshape(shape), conf.reshape(shape), t.reshape(shape)


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(a, np.float64) / np.asarray(b, np.float64)


def report(tab, edges):
    """The figures of ``metrics.calibration_report`` as numpy arrays, from the table alone (0 / 0 = NaN)."""
    tab = np.asarray(tab, np.int64)
    K, C = tab.shape[0] - 1, tab.shape[1]
    e = np.asarray(edges, np.float32).astype(np.float64)
    assert tab.shape == (K + 1, C, C + 3) and e.shape == (K,)
    conf = tab[:, :, :C]                                           # [bin][pred][label]
    n_bc = conf.sum(2)
    ok_bc = np.stack([conf[:, c, c] for c in range(C)], 1)
    # edge j keeps the bins j + 1 .. K: sums from the top
    above = lambda a: np.flip(np.cumsum(np.flip(a, 0), 0), 0)[1:]
    kept, correct, unl = above(n_bc), above(ok_bc), above(tab[:, :, C])
    n = int(n_bc.sum())
    out = {"kept": kept, "correct": correct, "kept_unlabelled": unl, "precision": _div(correct, kept), "coverage": _div(kept, n_bc.sum(0)[None]),
           "all_kept": kept.sum(1), "all_correct": correct.sum(1), "all_kept_unlabelled": unl.sum(1),
           "all_precision": _div(correct.sum(1), kept.sum(1)), "all_coverage": _div(kept.sum(1), n), "kept_confusion": above(conf),
           "labelled": n, "unlabelled": int(tab[:, :, C].sum())}
    count = n_bc.sum(1)
    acc = _div(ok_bc.sum(1), count)
    mean = _div(tab[:, :, C + 1].sum(1) / float(Q_SCALE), count)
    out.update(bin_count=count, bin_accuracy=acc, bin_mean_confidence=mean, class_bin_count=n_bc, class_bin_accuracy=_div(ok_bc, n_bc),
               class_bin_mean_confidence=_div(tab[:, :, C + 1] / float(Q_SCALE), n_bc))
    nz = count > 0
    out["ece"] = float((count[nz] / n * np.abs(acc[nz] - mean[nz])).sum()) if n else float("nan")
    return out


def threshold(rep, edges, precision, cls=None):
    row = rep["all_precision"] if cls is None else rep["precision"][:, cls]
    for j, p in enumerate(row):
        if p >= precision:
            return float(np.float32(edges[j]))
    return None
