"""Float64 numpy restatement of LabelProp's training tail (model.py:563-567 in its out-of-place form) and of the batch assembly
of labelPropTrain.py:162-193, the seeded frame-pair generator the goldens and the tests share, and the plain-torch twin of the
network.  The yardstick of the GPU kernel tests; tests/test_labelprop_train.py pins it to the reference's goldens on the CPU."""
import numpy as np
import torch
import torch.nn as nn

LP_WEIGHTS = (1.0, 6.0, 1.0, 3.0, 2.0)          # labelPropTrain.py:117
LP_SGD = dict(lr=2e-1, momentum=0.5, weight_decay=1e-3)      # labelPropTrain.py:127
# tag -> (frame pairs, H, W, seed of the frames); images of a batch = 2 x pairs
CONFIGS = {
    "lp_2x16x16": (1, 16, 16, 11),
    "lp_2x40x24": (1, 40, 24, 12),
    "lp_4x24x32": (2, 24, 32, 13),
    "lp_16x120x160": (8, 120, 160, 14),
}
SMALL = ("lp_2x16x16", "lp_2x40x24", "lp_4x24x32")
PRUNE_TAG, PRUNE_SEED, PRUNE_RATIO = "lp_4x24x32", 21, 0.3
NEAR_TIE = 1e-4
NEAR_TIE_CAP = 0.002        # share of a configuration's pixels the arg-max comparison may leave out


def synthetic_pairs(P, H, W, seed):
    """Seeded frame pairs (CPU generator, identical on every machine): images float32 [P,2,3,H,W] -- the second frame is the first
    plus a little noise, as consecutive frames are -- and labels int64 [P,2,H,W] in [0, 5)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(P, 1, 3, H, W, generator=g)
    b = a + 0.1 * torch.randn(P, 1, 3, H, W, generator=g)
    labels = torch.randint(0, 5, (P, 2, H, W), generator=g)
    return torch.cat([a, b], 1).contiguous(), labels


def prune_masks(params, seed=PRUNE_SEED, ratio=PRUNE_RATIO):
    """Seeded stand-in for pruneModelNew's index list: one boolean mask per parameter with dim() > 1, in parameters() order."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(p.shape, generator=g) < ratio for p in params if p.dim() > 1]


def sample_index(numel, name, n):
    """n distinct, sorted indices from a generator seeded by `name` (the fixed sample of a large tensor)."""
    import hashlib
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(numel, generator=g)[:n].sort()[0]


# ------------------------------------------------------------------------------------------ batch assembly
def assemble_np(images, labels, num_class=5):
    """labelPropTrain.py:162-193 -> (inputs [2B,8,H,W] float32, targets [2B,H,W] int64).  A label outside [0, num_class) selects no
    class: all class channels -1 (what the HIP kernel writes; torch's scatter_ would raise)."""
    images, labels = np.asarray(images, np.float32), np.asarray(labels, np.int64)
    B, _, _, H, W = images.shape
    x = np.empty((2 * B, 3 + num_class, H, W), np.float32)
    t = np.empty((2 * B, H, W), np.int64)
    cls = np.arange(num_class)[:, None, None]
    for b in range(B):
        ya, yb = images[b, 0, 0], images[b, 1, 0]
        pa = np.where(labels[b, 0][None] == cls, 1.0, -1.0).astype(np.float32)
        pb = np.where(labels[b, 1][None] == cls, 1.0, -1.0).astype(np.float32)
        x[2 * b] = np.concatenate([ya[None], yb[None], (ya - yb)[None], pb])
        x[2 * b + 1] = np.concatenate([yb[None], ya[None], (yb - ya)[None], pa])
        t[2 * b], t[2 * b + 1] = labels[b, 0], labels[b, 1]
    return x, t


# ------------------------------------------------------------------------------------------ the tail
def load_np(r, consts, mode):
    """A stored tensor [..., C] read through its load transform: 0 plain, 1 affine, 5 affine + ReLU (consts rows 0, 1)."""
    r = np.asarray(r, np.float64)
    if mode == 0:
        return r
    v = r * np.asarray(consts[0], np.float64) + np.asarray(consts[1], np.float64)
    return np.maximum(v, 0.0) if mode == 5 else v


def tail_forward_np(t, tc, top, w, b):
    """t [N,H,W,16] = upConv3's conv output, tc rows (scale, shift, mean), top [N,H,W,rch] = the skip VALUE, w [nC,16], b [nC]
    -> (v [N,H,W,16], logits [N,nC,H,W]) in float64."""
    t = np.asarray(t, np.float64)
    v = np.maximum(t * np.asarray(tc[0], np.float64) + np.asarray(tc[1], np.float64), 0.0)
    rch = top.shape[-1]
    v[..., :rch] += np.asarray(top, np.float64)
    logits = np.einsum("nhwk,ck->nchw", v, np.asarray(w, np.float64), optimize=True) + np.asarray(b, np.float64)[None, :, None, None]
    return v, logits


def ce_np(logits, target, weights):
    """Weighted CrossEntropyLoss (mean over the weights) -> (loss, d loss / d logits), float64."""
    lg = np.asarray(logits, np.float64)
    N, C, H, W = lg.shape
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    p = e / e.sum(1, keepdims=True)
    logp = (lg - m) - np.log(e.sum(1, keepdims=True))
    onehot = (np.asarray(target)[:, None] == np.arange(C)[None, :, None, None])
    ok = (np.asarray(target) >= 0) & (np.asarray(target) < C)
    wt = np.where(ok, np.asarray(weights, np.float64)[np.clip(target, 0, C - 1)], 0.0)
    sw = wt.sum()
    loss = -(wt * (logp * onehot).sum(1)).sum() / sw
    dl = (p - onehot) * wt[:, None] / sw
    return loss, dl


def tail_backward_np(t, tc, v, w, dlogits, rch):
    """-> dW [nC,16], db [nC], g [N,H,W,16] (gradient of upConv3's output = of v), gskip = g[..., :rch], and the RCV_STATS_BWD_DEC sums
    [2,16]: sum g*m and sum g*m*(t - mean) with m = (t*scale + shift > 0), the ReLU mask of upConv3 ALONE."""
    t, dl = np.asarray(t, np.float64), np.asarray(dlogits, np.float64)
    w = np.asarray(w, np.float64)
    dW = np.einsum("nchw,nhwk->ck", dl, v, optimize=True)
    db = dl.sum((0, 2, 3))
    g = np.einsum("nchw,ck->nhwk", dl, w, optimize=True)
    m = (t * np.asarray(tc[0], np.float64) + np.asarray(tc[1], np.float64)) > 0
    gm = np.where(m, g, 0.0)
    stats = np.stack([gm.sum((0, 1, 2)), (gm * (t - np.asarray(tc[2], np.float64))).sum((0, 1, 2))])
    return dW, db, g, g[..., :rch].copy(), stats


# ------------------------------------------------------------------------------------------ the twin (plain torch.nn)
class _CBR(nn.Module):
    def __init__(self, cin, cout, stride, dil):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, stride=stride, padding=dil, dilation=dil, bias=False)
        self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        return torch.relu(self.bn(self.conv(x)))


class _Up(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.ConvTranspose2d(cin, cout, 3, padding=1, stride=2, output_padding=1, bias=True)
        self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        return torch.relu(self.bn(self.conv(x)))


class LabelPropTwin(nn.Module):
    """The network in stock torch modules with the out-of-place tail; same sub-module names and state_dict keys as LabelProp."""

    def __init__(self, nC=5, P=32):
        super().__init__()
        self.pre = _CBR(8, P // 4, 1, 1)
        self.down1 = _CBR(P // 4, P // 2, 2, 1)
        self.down2 = _CBR(P // 2, P // 2, 2, 1)
        self.down3 = _CBR(P // 2, P, 2, 1)
        self.conv1 = _CBR(P, 2 * P, 1, 2)
        self.conv2 = _CBR(2 * P, 2 * P, 1, 2)
        self.conv3 = _CBR(2 * P, P, 1, 2)
        self.upConv1 = _Up(P, P // 2)
        self.upConv2 = _Up(P // 2, P // 2)
        self.upConv3 = _Up(P // 2, P // 2)
        self.classifier = nn.Conv2d(P // 2, nC, 1, padding=0)

    def forward(self, x):
        top = self.pre(x)
        middle = self.down1(top)
        bottom = self.down2(middle)
        x = self.conv3(self.conv2(self.conv1(self.down3(bottom))))
        x = bottom + self.upConv1(x)
        x = middle + self.upConv2(x)
        x = self.upConv3(x)
        x = torch.cat([x[:, 0:8] + top, x[:, 8:]], 1)
        return self.classifier(x)


def loop_assembly(images, labels, num_class=5):
    """The script's Python loop (labelPropTrain.py:162-193) in torch ops on whatever device the tensors are on: the twin's batch assembly."""
    B, _, _, H, W = images.shape
    inputs = torch.empty(2 * B, 3 + num_class, H, W, dtype=torch.float32, device=images.device)
    outputs = torch.empty(2 * B, H, W, dtype=torch.int64, device=images.device)
    cnt = 0
    for img, lab in zip(images, labels):
        preds = (torch.ones(2 * H * W, num_class, device=images.device).scatter_(1, lab.reshape(-1, 1), -1.0) * (-1)
                 ).view(2, H, W, num_class).permute(0, 3, 1, 2)
        inputs[cnt] = torch.cat([img[0][0][None], img[1][0][None], (img[0][0] - img[1][0])[None], preds[1]])
        inputs[cnt + 1] = torch.cat([img[1][0][None], img[0][0][None], (img[1][0] - img[0][0])[None], preds[0]])
        outputs[cnt], outputs[cnt + 1] = lab[0], lab[1]
        cnt += 2
    return inputs, outputs


# ------------------------------------------------------------------------------------------ exact cases of the tail kernels
# Operands on the integer grid of small_ops_restatement (every product and partial sum an integer below 2^24: exact in fp32 in any
# order), so that tests/test_gpu_labelprop_train.py compares lp_tail_fwd<0> / lp_tail_bwd<nC,0> with this file bit for bit.
TAIL_SMALL_PLANES = [(2, 9, 11), (1, 1, 1)]


def tail_big_planes(num_cus):
    """Two planes beyond one grid pass of the tail kernels (4 workgroups per CU, 256 pixels a chunk): a multiple of 256 pixels, and an
    odd count (256 CUs: 1x1025x256, 3x299x293)."""
    cap = 4 * num_cus * 256
    hodd = cap // (3 * 293) + 1
    hodd += 1 - hodd % 2
    out = [(1, cap // 256 + 1, 256), (3, hodd, 293)]
    assert all(n * h * w > cap for n, h, w in out) and (out[0][1] * 256) % 256 == 0 and (3 * hodd * 293) % 2 == 1
    return out


TAIL_MODES, TAIL_RCH, TAIL_CLASSES = (0, 1, 5), (4, 8, 12, 16), (1, 5, 8)


def tail_exact_cases(num_cus):
    """(plane, classes, skip width, skip load mode, first pixel of the second grid pass): the full product on the two small planes;
    beyond one grid pass every skip width on both planes, the class count and the load mode rotating (each big case costs about a
    second of float64 host arithmetic)."""
    cap = 4 * num_cus * 256
    out = [(pl, nC, rch, mode, 0) for pl in TAIL_SMALL_PLANES for nC in TAIL_CLASSES for rch in TAIL_RCH for mode in TAIL_MODES]
    for ri, rch in enumerate(TAIL_RCH):
        for pi, pl in enumerate(tail_big_planes(num_cus)):
            out.append((pl, TAIL_CLASSES[(2 * ri + pi) % 3], rch, TAIL_MODES[(ri + 2 * pi) % 3], cap))
    return out


def build_tail(plane, nC, rch, mode, second=0, seed=0, density=1.0):
    """t [N,H,W,16], r [N,H,W,rch], w [nC,16], b [nC], dl [N,nC,H,W] on the grid ({-1..1} on the large planes; `density` thins t, r
    and dl further), tc [5][16] / rc [5][rch] from grid_consts.  The two pixels of drop_masks (the last one; the first of the second
    grid pass, `second`) have dl = 1 for every class, v > 0 in every channel, the ReLU mask on and t != mean; the filter's column sums
    are non-zero: removing either pixel changes every entry of dW, db and both statistics rows."""
    import small_ops_restatement as S
    N, H, W = plane
    npix = N * H * W
    rng = np.random.default_rng(52000 + 7 * seed + npix + 3 * nC + 5 * rch + mode)
    a = 1 if npix > 50000 else 2
    c = dict(plane=plane, nC=nC, rch=rch, mode=mode, npix=npix, second=second)
    c["t"] = S.grid(rng, (N, H, W, 16), a, density)
    c["r"] = S.grid(rng, (N, H, W, rch), a, density)
    c["tc"], c["rc"] = S.grid_consts(rng, 16), S.grid_consts(rng, rch)
    c["w"], c["b"] = S.grid(rng, (nC, 16), 2), S.grid(rng, (nC,), 2)
    dl = S.grid(rng, (npix, nC), a, density)
    col = c["w"].sum(0)
    c["w"][0, col == 0] += np.where(c["w"][0, col == 0] < 2, 1, -1)
    idx, _ = S.drop_masks(npix, second)
    c["t"].reshape(npix, 16)[idx] = 2 * np.sign(c["tc"][0])
    c["r"].reshape(npix, rch)[idx] = 1.0 if mode == 0 else 2 * np.sign(c["rc"][0])
    dl[idx] = 1.0
    c["dl"] = np.ascontiguousarray(dl.reshape(N, H, W, nC).transpose(0, 3, 1, 2))
    return c


def tail_reference(c, keep=None):
    """-> logits, dW, db, g, gskip, statistics rows; keep: a boolean vector over the pixels, a dropped pixel adds nothing to the
    reductions (its logits gradient reads zero)."""
    v, logits = tail_forward_np(c["t"], c["tc"], load_np(c["r"], c["rc"], c["mode"]), c["w"], c["b"])
    dl = c["dl"] if keep is None else c["dl"] * np.asarray(keep, np.float32).reshape(c["plane"])[:, None]
    return (logits,) + tail_backward_np(c["t"], c["tc"], v, c["w"], dl, c["rch"])


def check_tail(c):
    """The preconditions of an exact tail case: sums of |terms| of the logits, dW, db, g and the statistics rows are integers below
    2^24; the ReLU mask meets values at and below zero; each of the two pixels of drop_masks adds a non-zero term to every entry of dW,
    db and both statistics rows (a kernel that loses one of them gets every reduced entry wrong).  -> tail_reference(c)."""
    import small_ops_restatement as S
    A = lambda x: np.abs(np.asarray(x, np.float64))
    npix, nC = c["npix"], c["nC"]
    v, _ = tail_forward_np(c["t"], c["tc"], load_np(c["r"], c["rc"], c["mode"]), c["w"], c["b"])
    full = tail_reference(c)
    g = full[3]
    dlp = np.ascontiguousarray(np.asarray(c["dl"], np.float64).transpose(0, 2, 3, 1)).reshape(npix, nC)
    S.assert_exact(A(c["w"]).sum(1) * A(v).max() + A(c["b"]), 1.0, "tail logits")
    S.assert_exact(A(dlp).T @ A(v).reshape(npix, 16), 1.0, "tail dW")
    S.assert_exact(A(dlp).sum(0), 1.0, "tail db")
    S.assert_exact(S.stats_abs(S.STATS_BWD_DEC, g, c["t"], c["tc"]), 1.0, "tail statistics")
    assert float(A(dlp).sum(1).max() * A(c["w"]).max()) < 2.0 ** 24
    z = np.asarray(c["t"], np.float64).reshape(npix, 16) * c["tc"][0] + c["tc"][1]
    if npix > 1:
        assert (z == 0).any() and (z < 0).any(), "the mask must meet pixels at and below zero"
    for i in S.drop_masks(npix, c["second"])[0]:
        gi = g.reshape(npix, 16)[i]
        assert np.all(dlp[i] != 0) and np.all(v.reshape(npix, 16)[i] != 0) and np.all(z[i] > 0) and np.all(gi != 0), i
        assert np.all(np.asarray(c["t"], np.float64).reshape(npix, 16)[i] != c["tc"][2]), i
    return full
