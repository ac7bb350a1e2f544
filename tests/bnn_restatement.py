"""Restatement of the BNN-L / BNN-M-C patch classifiers (reference model.py:569-619) over a ``state_dict``, in two forms:

* ``forward`` -- torch functional ops on the CPU in the dtype of the parameters, with the dropout keep-scales passed in (a Dropout of
  the reference is ``x * noise``, noise = bernoulli(1 - p) / (1 - p), so imposing the noise reproduces it bit for bit).  Differentiable
  through autograd; pinned bit for bit on the goldens (tests/golden/bnn.npz, 8 threads).
* ``stage_fwd64`` / ``stage_bwd64`` / ``head_fwd64`` / ``head_bwd64`` -- float64 forms of ONE stage (conv -> keep-scale -> max-pool ->
  ReLU) and of BNN-L's head with hand-written backward passes: the gradient of a pool window goes to its FIRST maximum in row-major
  window order (aten's rule), a pixel that wins several overlapping windows sums their gradients.

Layouts here are torch's (NCHW activations, [Cout][Cin][K][K] filters); the device tests permute.
"""
import numpy as np
import torch
import torch.nn.functional as F

# name -> (stages, head): a stage is (conv, padding, pool k or 0, relu)
NETS = {
    "BNNL": ([("conv1", 4, 4, True), ("conv2", 3, 4, True), ("conv3", 3, 4, True)], True),
    "BNNMC": ([("conv1", 1, 4, True), ("conv2", 1, 4, True), ("conv3", 1, 2, True), ("classifier", 0, 0, False)], False),
}
SHAPES = {
    "BNNL": [("conv1", (8, 3, 8, 8)), ("conv2", (16, 8, 8, 8)), ("conv3", (16, 16, 8, 8)), ("fc", (512, 16, 1, 1)), ("classifier", (4, 512, 1, 1))],
    "BNNMC": [("conv1", (8, 3, 5, 5)), ("conv2", (16, 8, 3, 3)), ("conv3", (16, 16, 3, 3)), ("classifier", (4, 16, 3, 3))],
}
DROP_P = 0.25
# the stage cases of the device tests: N, H, W, Cin, Cout, K, padding, pool k, dropout (ReLU wherever there is a pool)
STAGE_CASES = [
    (2, 9, 12, 3, 8, 8, 4, 4, True),        # NCHW first stage; conv 10x13 -> 4x5; column 12 lies in no window
    (3, 15, 15, 8, 16, 8, 3, 4, True),      # BNN-L stage 2 as it runs
    (2, 6, 6, 16, 16, 8, 3, 4, False),      # filter larger than the plane, -> 1x1, row and column 4 unused
    (2, 12, 10, 3, 8, 5, 1, 4, True),
    (2, 7, 9, 16, 16, 3, 1, 2, True),       # remainder row and column
    (2, 5, 4, 16, 4, 3, 0, 0, False),       # no ReLU: BNN-M-C's classifier
    (1, 40, 36, 3, 8, 8, 4, 4, True),       # more than one tile per plane
]
NORMAL_CASES = {1: 11, 6: 12}               # index into STAGE_CASES -> seed of the random-normal run
CE_WEIGHTS = (1.0, 2.0, 0.5, 3.0)


def state_keys(net):
    """(key, shape) in the reference's parameter order."""
    out = []
    for name, shape in SHAPES[net]:
        out += [(name + ".weight", shape), (name + ".bias", (shape[0],))]
    return out


def forward(net, sd, x, masks=None, taps=None):
    """Logits [B,4,h,w].  ``masks``: None (eval mode) or the keep-scales in forward order: do1..3 as [N,C] (0 or 1/(1-p)), BNN-L's dof as
    [N,512,h,w] (0 or 2).  ``taps``: a dict that receives the pool inputs, pool outputs and the head's ReLU input."""
    stages, head = NETS[net]
    mi = 0
    for si, (name, pad, k, relu) in enumerate(stages):
        x = F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)
        if k:
            if masks is not None:
                x = x * masks[mi].reshape(x.shape[0], x.shape[1], 1, 1).to(x.dtype)
                mi += 1
            if taps is not None:
                taps["pool_in%d" % si] = x
            x = F.max_pool2d(x, k, 2)
            if taps is not None:
                taps["pool_out%d" % si] = x
        if relu:
            x = F.relu(x)
    if head:
        x = F.conv2d(x, sd["fc.weight"], sd["fc.bias"])
        if masks is not None:
            x = x * masks[mi].to(x.dtype)
        if taps is not None:
            taps["head_relu_in"] = x
        x = F.conv2d(F.relu(x), sd["classifier.weight"], sd["classifier.bias"])
    return x


def out_plane(net, H, W):
    for name, pad, k, relu in NETS[net][0]:
        K = dict(SHAPES[net])[name][2]
        H, W = H + 2 * pad - K + 1, W + 2 * pad - K + 1
        if k:
            H, W = (H - k) // 2 + 1, (W - k) // 2 + 1
    return H, W


def train_steps(net, sd, x, t, masks_per_step, lr=1e-2, momentum=0.9, weight_decay=5e-4):
    """objDetEval.py:113-119 on the CPU: per step squeeze, weighted CrossEntropyLoss, backward, SGD.  Returns (losses, final params)."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.SGD([{"params": list(params.values())}], lr=lr, momentum=momentum, weight_decay=weight_decay)
    crit = torch.nn.CrossEntropyLoss(torch.tensor(CE_WEIGHTS))
    losses = []
    for masks in masks_per_step:
        opt.zero_grad()
        loss = crit(torch.squeeze(forward(net, params, x, masks)), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in params.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# float64, explicit backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _windows(cv, k):
    """[N,C,Hc,Wc] -> [N,C,Ho,Wo,k*k], stride 2, floor."""
    w = cv.unfold(2, k, 2).unfold(3, k, 2)
    return w.reshape(*w.shape[:4], k * k)


def stage_fwd64(x, w, b, keep, pad, k, relu):
    """x [N,Cin,H,W], w [Cout,Cin,K,K], keep [N,Cout] or None, all float64.  Returns (out [N,Cout,Ho,Wo], arg uint8 or None): arg =
    the window offset of the first maximum in row-major window order."""
    cv = F.conv2d(x, w, b, padding=pad)
    if keep is not None:
        cv = cv * keep.reshape(keep.shape[0], keep.shape[1], 1, 1)
    arg = None
    if k:
        win = _windows(cv, k)
        arg = torch.from_numpy(win.numpy().argmax(axis=-1).astype(np.uint8))      # numpy: the first occurrence
        cv = torch.gather(win, 4, arg.long().unsqueeze(-1)).squeeze(-1)
    out = torch.clamp(cv, min=0) if relu else cv
    return out, arg


def stage_bwd64(x, w, keep, pad, k, relu, out, arg, dout):
    """Returns (dx, dW, db, dconv) in float64; dconv = d loss / d (conv + bias)."""
    N, Cin, H, W = x.shape
    Cout, _, K, _ = w.shape
    Hc, Wc = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    g = torch.where(out > 0, dout, torch.zeros_like(dout)) if relu else dout
    if k:
        Ho, Wo = out.shape[2], out.shape[3]
        dconv = torch.zeros(N, Cout, Hc, Wc, dtype=torch.float64)
        for j in range(k * k):
            dy, dx_ = j // k, j % k
            dconv[:, :, dy:dy + 2 * Ho:2, dx_:dx_ + 2 * Wo:2][:, :, :Ho, :Wo] += torch.where(arg == j, g, torch.zeros_like(g))
    else:
        dconv = g.clone()
    if keep is not None:
        dconv = dconv * keep.reshape(N, Cout, 1, 1)
    xp = F.pad(x, (pad, pad, pad, pad))
    dW = torch.zeros_like(w)
    for ky in range(K):
        for kx in range(K):
            dW[:, :, ky, kx] = torch.einsum("noyx,ncyx->oc", dconv, xp[:, :, ky:ky + Hc, kx:kx + Wc])
    db = dconv.sum(dim=(0, 2, 3))
    dxp = torch.zeros_like(xp)
    for ky in range(K):
        for kx in range(K):
            dxp[:, :, ky:ky + Hc, kx:kx + Wc] += torch.einsum("noyx,oc->ncyx", dconv, w[:, :, ky, kx])
    dx = dxp[:, :, pad:pad + H, pad:pad + W].clone()
    return dx, dW, db, dconv


def head_fwd64(x, wfc, bfc, keep, wc, bc):
    """x [M,16], wfc [512,16], keep [M,512] or None, wc [nC,512]; returns (logits [M,nC], z [M,512] = the ReLU's input)."""
    z = x @ wfc.t() + bfc
    if keep is not None:
        z = z * keep
    return torch.clamp(z, min=0) @ wc.t() + bc, z


def head_bwd64(x, wfc, keep, wc, z, dl):
    """Returns (dx, dWfc, dbfc, dWc, dbc)."""
    h = torch.clamp(z, min=0)
    dWc = dl.t() @ h
    dbc = dl.sum(0)
    dz = torch.where(z > 0, dl @ wc, torch.zeros_like(z))
    if keep is not None:
        dz = dz * keep
    return dz @ wfc, dz.t() @ x, dz.sum(0), dWc, dbc


def exact_case(seed, N, H, W, Cin, Cout, K, pad, k, dropout):
    """Operands whose every sum is exact in fp32 whatever its order: small integer inputs and output gradients, filters and biases
    that are multiples of 1/8, keep-scales in {0, 2}.  Full of exact ties and of pixels that win several overlapping windows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, Cin, H, W), generator=g).double()
    w = torch.randint(-8, 9, (Cout, Cin, K, K), generator=g).double() / 8
    b = torch.randint(-8, 9, (Cout,), generator=g).double() / 8
    keep = (torch.randint(0, 2, (N, Cout), generator=g).double() * 2) if dropout else None
    Hc, Wc = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    Ho, Wo = ((Hc - k) // 2 + 1, (Wc - k) // 2 + 1) if k else (Hc, Wc)
    dout = torch.randint(-4, 5, (N, Cout, Ho, Wo), generator=g).double()
    return x, w, b, keep, dout


def normal_case(seed, N, H, W, Cin, Cout, K, pad, k, dropout):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g)
    b = torch.randn(Cout, generator=g)
    keep = ((torch.rand(N, Cout, generator=g) < 0.75).float() / torch.tensor(0.75)) if dropout else None
    Hc, Wc = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    Ho, Wo = ((Hc - k) // 2 + 1, (Wc - k) // 2 + 1) if k else (Hc, Wc)
    dout = torch.randn(N, Cout, Ho, Wo, generator=g)
    return x, w, b, keep, dout


def near_tie_windows(x, w, b, keep, pad, k, gap=1e-5):
    """Boolean [N,Cout,Ho,Wo]: windows of the float64 conv whose two largest values differ by less than ``gap`` (kept channels only:
    a dropped channel is all zeros and carries no gradient)."""
    cv = F.conv2d(x, w, b, padding=pad)
    if keep is not None:
        cv = cv * keep.reshape(keep.shape[0], keep.shape[1], 1, 1)
    top = torch.topk(_windows(cv, k), 2, dim=-1)[0]
    near = (top[..., 0] - top[..., 1]) < gap
    if keep is not None:
        near = near & (keep.reshape(keep.shape[0], keep.shape[1], 1, 1) != 0)
    return near
