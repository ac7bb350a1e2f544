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
    logits = np.einsum("nhwk,ck->nchw", v, np.asarray(w, np.float64)) + np.asarray(b, np.float64)[None, :, None, None]
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
    dW = np.einsum("nchw,nhwk->ck", dl, v)
    db = dl.sum((0, 2, 3))
    g = np.einsum("nchw,ck->nhwk", dl, w)
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
