"""The contract of RCV_OP_OBJECTS (include/rcv.h rcv_find_objects) restated in numpy and plain Python, the literal way:
components and their order from objdet_restatement._label (8-connected, numbered per (image, class) by first 2x2 block), boxes as
objdet_restatement._rect gives them (cv2.boundingRect), then per class

    A    = components with area > min_area                       (strict, DBConvert.py:55)
    amax = the largest area in A, 0 if A is empty
    Q    = members of A with float(area) >= float(amax) * ratio  (one fp64 multiply, one compare)
    emit = the first min(|Q|, cap) of Q sorted by (-area, rank)

find_objects returns (rows int64 [N][C-1][M][8] = {x, y, w, h, area, rank, 2x+w, 2y+h}, zero past the emitted count,
counts int64 [N][C-1][4] = {components, |A|, |Q|, emitted})."""
import numpy as np

import objdet_restatement as R


def boxes(lab, n):
    """_rect of every component of a label plane at once: int arrays x, y, w, h, area, each [n]."""
    ys, xs = np.nonzero(lab >= 0)
    ids = lab[ys, xs]
    area = np.bincount(ids, minlength=n)
    x0 = np.full(n, 1 << 30); x1 = np.full(n, -1); y0 = np.full(n, 1 << 30); y1 = np.full(n, -1)
    np.minimum.at(x0, ids, xs); np.maximum.at(x1, ids, xs); np.minimum.at(y0, ids, ys); np.maximum.at(y1, ids, ys)
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1, area


def components(plane, c):
    """Every component of class c of one plane in rank order: a list of (x, y, w, h, area)."""
    lab, n = R._label(np.asarray(plane) == c)
    if n == 0:
        return []
    x, y, w, h, area = boxes(lab, n)
    return [(int(x[k]), int(y[k]), int(w[k]), int(h[k]), int(area[k])) for k in range(n)]


def _seq(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def find_objects(maps, C, min_area=0, min_ratio=0.0, max_objects=8):
    maps = np.asarray(maps)
    N = maps.shape[0]
    min_area, min_ratio, cap = _seq(min_area, C - 1), _seq(min_ratio, C - 1), _seq(max_objects, C - 1)
    M = max([1] + cap) if isinstance(max_objects, (list, tuple)) else max_objects
    rows = np.zeros((N, C - 1, M, 8), dtype=np.int64)
    counts = np.zeros((N, C - 1, 4), dtype=np.int64)
    for n in range(N):
        for c in range(1, C):
            comps = components(maps[n], c)
            A = [k for k in range(len(comps)) if comps[k][4] > min_area[c - 1]]
            amax = max([comps[k][4] for k in A], default=0)
            Q = [k for k in A if float(comps[k][4]) >= float(amax) * min_ratio[c - 1]]
            Q.sort(key=lambda k: (-comps[k][4], k))
            emit = Q[:cap[c - 1]]
            for r, k in enumerate(emit):
                x, y, w, h, area = comps[k]
                rows[n, c - 1, r] = [x, y, w, h, area, k, 2 * x + w, 2 * y + h]
            counts[n, c - 1] = [len(comps), len(A), len(Q), len(emit)]
    return rows, counts
