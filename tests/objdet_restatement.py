"""Two independent restatements of the object-detection contract of RCV_OP_OBJECT_MATCH (test.py:28-89, getPrecRecall), numpy and
pure Python only.  Both number the components of a plane by their first 2x2 block in raster order (block index
(y>>1)*ceil(W/2) + (x>>1)), the order OpenCV's block-based 8-connectivity labelling is understood to produce.

literal(): flood fill, full-plane masks per (pred, target) pair and the reference's own loop shape -- tiny planes only.
fast():    vectorised union-find labelling, pair counts with np.unique, per-pred vector tests -- planes up to 480x640.
Both return int64 counts [N][C-1][2+2K] = {nPred, nTrue, nCorrIoU[K], nCorrDist[K]}; scores() turns the counts of a list of
batches into test.py's float64 sums (prec/recall over c, then b; one value per batch)."""
import numpy as np


def _block_index(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (y >> 1) * ((W + 1) // 2) + (x >> 1)


# ------------------------------------------------------------------------------------------------------------------ literal
def _flood_components(mask):
    """8-connected components of a bool plane as lists of (y, x), in first-block order."""
    H, W = mask.shape
    seen = np.zeros_like(mask, dtype=bool)
    blk = _block_index(H, W)
    comps = []
    for y0 in range(H):
        for x0 in range(W):
            if not mask[y0, x0] or seen[y0, x0]:
                continue
            stack, pix = [(y0, x0)], []
            seen[y0, x0] = True
            while stack:
                y, x = stack.pop()
                pix.append((y, x))
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ny, nx = y + dy, x + dx
                        if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
            comps.append(pix)
    comps.sort(key=lambda pix: min(int(blk[y, x]) for y, x in pix))
    return comps


def _rect(m):
    ys, xs = np.nonzero(m)
    x, y = int(xs.min()), int(ys.min())
    return x, y, int(xs.max()) - x + 1, int(ys.max()) - y + 1       # cv2.boundingRect


def literal(pred, target, C, iou_thr, dist_thr):
    pred, target = np.asarray(pred, dtype=np.int64), np.asarray(target, dtype=np.int64)
    N, H, W = pred.shape
    K = len(iou_thr)
    out = np.zeros((N, C - 1, 2 + 2 * K), dtype=np.int64)
    for c in range(1, C):
        for b in range(N):
            masks = []
            for plane in (pred[b], target[b]):
                ms = []
                for pix in _flood_components(plane == c):
                    m = np.zeros((H, W), dtype=bool)
                    for y, x in pix:
                        m[y, x] = True
                    ms.append(m)
                masks.append(ms)
            P, T = masks
            out[b, c - 1, 0], out[b, c - 1, 1] = len(P), len(T)
            for k in range(K):
                usedI, usedD = [False] * len(T), [False] * len(T)
                nI = nD = 0
                for pm in P:
                    px, py, pw, ph = _rect(pm)
                    pc = (px + pw / 2, py + ph / 2)
                    foundI = foundD = False
                    for j, tm in enumerate(T):
                        tx, ty, tw, th = _rect(tm)
                        tc = (tx + tw / 2, ty + th / 2)
                        dist = np.sqrt((pc[0] - tc[0]) ** 2 + (pc[1] - tc[1]) ** 2)
                        iou = (pm & tm).sum() / (pm | tm).sum()
                        if iou > iou_thr[k] and not foundI and not usedI[j]:
                            nI, foundI, usedI[j] = nI + 1, True, True
                        if dist_thr[k] > dist and not foundD and not usedD[j]:
                            nD, foundD, usedD[j] = nD + 1, True, True
                out[b, c - 1, 2 + k], out[b, c - 1, 2 + K + k] = nI, nD
    return out


# --------------------------------------------------------------------------------------------------------------------- fast
def _label(mask):
    """Vectorised union-find: component number (0-based, first-block order) per pixel, -1 off the mask; and the count."""
    H, W = mask.shape
    n = H * W
    idx = np.arange(n).reshape(H, W)
    us, vs = [], []
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        y0, y1 = 0, H - dy
        xa0, xa1 = max(0, -dx), W - max(0, dx)
        a = mask[y0:y1, xa0:xa1] & mask[y0 + dy:y1 + dy, xa0 + dx:xa1 + dx]
        us.append(idx[y0:y1, xa0:xa1][a])
        vs.append(idx[y0 + dy:y1 + dy, xa0 + dx:xa1 + dx][a])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(n)

    def compress(p):
        while True:
            q = p[p]
            if np.array_equal(q, p):
                return p
            p = q
    while u.size:
        ru, rv = parent[u], parent[v]
        d = ru != rv
        if not d.any():
            break
        np.minimum.at(parent, np.maximum(ru, rv)[d], np.minimum(ru, rv)[d])
        parent = compress(parent)
    flat = mask.ravel()
    roots = np.unique(parent[flat])
    key = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(key, parent[flat], _block_index(H, W).ravel()[flat])
    order = roots[np.argsort(key[roots], kind="stable")]
    rank = np.full(n, -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    lab = np.where(flat, rank[parent], -1).reshape(H, W)
    return lab, int(order.size)


def _stats(lab, n):
    ys, xs = np.nonzero(lab >= 0)
    ids = lab[ys, xs]
    area = np.bincount(ids, minlength=n)
    x0 = np.full(n, 1 << 30); x1 = np.full(n, -1); y0 = np.full(n, 1 << 30); y1 = np.full(n, -1)
    np.minimum.at(x0, ids, xs); np.maximum.at(x1, ids, xs); np.minimum.at(y0, ids, ys); np.maximum.at(y1, ids, ys)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    return area, x0 + w / 2, y0 + h / 2


def fast(pred, target, C, iou_thr, dist_thr):
    pred, target = np.asarray(pred, dtype=np.int64), np.asarray(target, dtype=np.int64)
    N, H, W = pred.shape
    K = len(iou_thr)
    out = np.zeros((N, C - 1, 2 + 2 * K), dtype=np.int64)
    for b in range(N):
        for c in range(1, C):
            pl, np_ = _label(pred[b] == c)
            tl, nt = _label(target[b] == c)
            out[b, c - 1, 0], out[b, c - 1, 1] = np_, nt
            if np_ == 0 or nt == 0:
                continue
            pa, pcx, pcy = _stats(pl, np_)
            ta, tcx, tcy = _stats(tl, nt)
            both = (pl >= 0) & (tl >= 0)
            keys, inter = np.unique(pl[both] * nt + tl[both], return_counts=True)
            kp, kt = keys // nt, keys % nt
            iou = inter / (pa[kp] + ta[kt] - inter)
            cand = [(kt[kp == i], iou[kp == i]) for i in range(np_)]
            for k in range(K):
                used = np.zeros(nt, dtype=bool)
                n_corr = 0
                for i in range(np_):
                    tj, v = cand[i]
                    ok = tj[(v > iou_thr[k]) & ~used[tj]]
                    if ok.size:
                        used[ok.min()] = True
                        n_corr += 1
                out[b, c - 1, 2 + k] = n_corr
                used = np.zeros(nt, dtype=bool)
                n_corr = 0
                for i in range(np_):
                    dist = np.sqrt((pcx[i] - tcx) ** 2 + (pcy[i] - tcy) ** 2)
                    ok = (dist_thr[k] > dist) & ~used
                    if ok.any():
                        used[int(np.argmax(ok))] = True
                        n_corr += 1
                out[b, c - 1, 2 + K + k] = n_corr
    return out


def scores(batches, C, K):
    """test.py:77-89 per batch, summed over the batches: ([K] IoU sums, [K] distance sums) -- divide by the image count."""
    sums = [[0.0] * K, [0.0] * K]
    for cnt in batches:
        cnt = np.asarray(cnt)
        for crit in (0, 1):
            for k in range(K):
                prec = recall = 0
                for c in range(C - 1):
                    for b in range(cnt.shape[0]):
                        n_pred, n_true, n_corr = int(cnt[b, c, 0]), int(cnt[b, c, 1]), int(cnt[b, c, 2 + crit * K + k])
                        prec += n_corr / n_pred if n_pred != 0 else 1
                        recall += n_corr / n_true if n_true != 0 else 1
                prec /= (C - 1)
                recall /= (C - 1)
                sums[crit][k] += (prec + recall) / 2
    return sums


# ---------------------------------------------------------------------------------------------------------------- test data
def blob_masks(rng, N, H, W, C, n_blobs=12, r_max=None):
    """Class maps of random filled ellipses / rectangles over background 0 (later blobs paint over earlier ones)."""
    r_max = r_max or max(2, min(H, W) // 6)
    out = np.zeros((N, H, W), dtype=np.int64)
    y, x = np.mgrid[0:H, 0:W]
    for b in range(N):
        for _ in range(n_blobs):
            c = int(rng.integers(1, C))
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            ry, rx = rng.integers(1, r_max + 1), rng.integers(1, r_max + 1)
            if rng.random() < 0.5:
                m = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
            else:
                m = (abs(y - cy) <= ry) & (abs(x - cx) <= rx)
            out[b][m] = c
    return out


def jitter(rng, masks, C, p=0.02):
    """A perturbed copy (predictions near the targets): a fraction p of the pixels gets a random class."""
    out = masks.copy()
    flip = rng.random(masks.shape) < p
    out[flip] = rng.integers(0, C, size=int(flip.sum()))
    return out
