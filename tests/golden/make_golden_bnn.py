"""Golden vectors of the BNN-L / BNN-M-C patch classifiers (reference model.py:569-619, the step of objDetEval.py:89-119).  Runs ONLY
where the reference exists: it imports the reference's ``model.py`` (pure PyTorch) and runs it on the CPU with 8 threads on seeded
inputs, in the style of ``make_golden_classify.py``.  Nothing from the reference's source text is stored: tensors and numbers only.

    python tests/golden/make_golden_bnn.py          # writes bnn.npz / bnn.json next to this script

Per configuration: the init state_dict hash (torch.manual_seed(12345678)), the input seed and hash, the dropout keep masks the
reference drew (forward hooks: a channel / element is kept iff its output is non-zero), the train-mode logits, the weighted
CrossEntropyLoss (weights 1, 2, .5, 3) of the squeezed logits, the targets, every parameter gradient (in full up to 4096 elements,
otherwise its norm and a fixed seeded sample of 1024 elements), the parameter sums after one SGD(lr 1e-2, momentum .9, weight decay
5e-4) step and the eval-mode logits after it.

Near ties.  A pool arg-max or a ReLU sign that sits within fp32 rounding moves a whole element's share of a gradient, so an input
is accepted only if it has none: a float64 twin (tests/bnn_restatement.py over the same parameters and masks) gives, per pool,
d = max |fp32 - fp64| over the pool's input; on kept channels every window's top-2 gap and every pooled value (the ReLU's input)
must be >= 8 d, and every kept input of the head's ReLU >= 8 x that tensor's own d.  The first input seed from 3 upward (at most 64
tried) that passes is taken; the seed and the worst ratios go to bnn.json.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.environ.get("GOLDEN_OUT") or os.path.dirname(os.path.abspath(__file__))      # where the fixtures are written
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))         # tests/: the restatement lives beside the tests
import bnn_restatement as R  # noqa: E402

THREADS = 8
FULL_MAX = 4096
SAMPLE = 1024
MARGIN = 8.0

# tag -> (net, B, H, W)
CONFIGS = {
    "bnnl_3x32x32": ("BNNL", 3, 32, 32),
    "bnnl_2x40x36": ("BNNL", 2, 40, 36),          # a 2x2 logit plane
    "bnnmc_3x32x32": ("BNNMC", 3, 32, 32),
    "bnnmc_2x40x36": ("BNNMC", 2, 40, 36),        # 2x1
}


def sd_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def npy(t):
    return t.detach().cpu().numpy().copy()


def sample_index(numel, name):
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(numel, generator=g)[:SAMPLE].sort()[0]


def make_input(B, H, W, seed):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


def one_try(ref, net, B, H, W, seed):
    torch.manual_seed(12345678)
    model = getattr(ref, net)()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x = make_input(B, H, W, seed)
    masks, taps = [], {}
    for name in ("do1", "do2", "do3"):
        do = getattr(model, name)
        do.register_forward_hook(lambda m, i, o: masks.append(
            (o != 0).flatten(2).any(2).to(torch.float32) / torch.tensor(1.0 - m.p)))
    for si, name in enumerate(("pool1", "pool2", "pool3")):
        getattr(model, name).register_forward_hook(lambda m, i, o, si=si: taps.update({"pool_in%d" % si: i[0].detach(), "pool_out%d" % si: o.detach()}))
    if net == "BNNL":
        model.dof.register_forward_hook(lambda m, i, o: (masks.append(((o != 0) | (i[0] == 0)).to(torch.float32) / torch.tensor(1.0 - m.p)),
                                                         taps.update({"head_relu_in": o.detach()})) and None)
    crit = torch.nn.CrossEntropyLoss(torch.tensor(R.CE_WEIGHTS))
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-2, momentum=0.9, weight_decay=5e-4)
    model.train()
    opt.zero_grad()
    logits = model(x)
    pred = torch.squeeze(logits)
    tshape = tuple(list(pred.shape[:1]) + list(pred.shape[2:]))
    t = torch.randint(0, 4, tshape, generator=torch.Generator().manual_seed(4))
    loss = crit(pred, t)
    loss.backward()
    masks = masks[:4 if net == "BNNL" else 3]
    # float64 twin with the same masks
    taps64 = {}
    sd64 = {k: v.double() for k, v in sd0.items()}
    l64 = R.forward(net, sd64, x.double(), [m.double() for m in masks], taps64)
    ratios = {}
    ok = True
    for si in range(3):
        a, b64 = taps["pool_in%d" % si], taps64["pool_in%d" % si]
        d = float((a.double() - b64).abs().max())
        kept = (masks[si] != 0).reshape(B, -1, 1, 1)
        k = 2 if (net == "BNNMC" and si == 2) else 4
        top = torch.topk(R._windows(b64, k), 2, dim=-1)[0]
        gap = (top[..., 0] - top[..., 1])[kept.expand_as(top[..., 0])]
        mag = taps64["pool_out%d" % si].abs()[kept.expand_as(taps64["pool_out%d" % si])]
        ratios["pool%d_gap" % (si + 1)] = float(gap.min()) / d
        ratios["pool%d_relu" % (si + 1)] = float(mag.min()) / d
    if net == "BNNL":
        a, b64 = taps["head_relu_in"], taps64["head_relu_in"]
        d = float((a.double() - b64).abs().max())
        ratios["head_relu"] = float(b64.abs()[masks[3] != 0].min()) / d
    ok = all(v >= MARGIN for v in ratios.values())
    return ok, ratios, dict(model=model, sd0=sd0, x=x, masks=masks, logits=logits, t=t, loss=loss, opt=opt, l64=l64)


def run(ref, tag, out, meta):
    net, B, H, W = CONFIGS[tag]
    for seed in range(3, 3 + 64):
        ok, ratios, s = one_try(ref, net, B, H, W, seed)
        print(tag, "seed", seed, "ok" if ok else "near tie", {k: round(v, 1) for k, v in ratios.items()})
        if ok:
            break
    else:
        raise SystemExit("%s: no input seed in 3..66 is free of near ties" % tag)
    model, opt, x, logits, loss = s["model"], s["opt"], s["x"], s["logits"], s["loss"]
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    sd1 = {k: v.clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        eval_logits = model(x)
    e = {"net": net, "B": B, "H": H, "W": W, "weights": list(R.CE_WEIGHTS), "threads": torch.get_num_threads(), "torch": torch.__version__,
         "sd_hash_init": sd_hash(s["sd0"]), "input_seed": seed, "x_sha": hashlib.sha256(npy(x).tobytes()).hexdigest()[:16],
         "loss": float(loss.detach()), "near_tie_ratios": ratios, "margin": MARGIN,
         "grad_norm": {k: float(g.double().norm()) for k, g in grads.items()},
         "param_after_step_sum": {k: float(v.double().sum()) for k, v in sd1.items()},
         "logits_shape": list(logits.shape), "sgd": {"lr": 1e-2, "momentum": 0.9, "weight_decay": 5e-4}}
    for mi, m in enumerate(s["masks"]):
        out["%s/keep%d" % (tag, mi)] = npy(m != 0).astype(np.uint8)
    out[tag + "/t"] = npy(s["t"]).astype(np.int64)
    out[tag + "/logits"] = npy(logits)
    out[tag + "/eval_logits"] = npy(eval_logits)
    for k, g in grads.items():
        if g.numel() <= FULL_MAX:
            out["%s/grad/%s" % (tag, k)] = npy(g)
        else:
            out["%s/grad_sample/%s" % (tag, k)] = npy(g.reshape(-1)[sample_index(g.numel(), k)])
    meta[tag] = e


def main():
    torch.set_num_threads(THREADS)
    sys.path.insert(0, REF)
    import model as ref          # the reference, imported (never copied)
    out, meta = {}, {}
    for tag in CONFIGS:
        run(ref, tag, out, meta)
    meta["_sample"] = {"full_max": FULL_MAX, "sample": SAMPLE}
    np.savez_compressed(os.path.join(HERE, "bnn.npz"), **out)
    with open(os.path.join(HERE, "bnn.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
