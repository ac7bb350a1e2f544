"""Golden vectors for the networks whose last convolution is 5x5 (PB_FCN(kernelSize=5), ROBO_UNet(classSize=5)).  Runs ONLY where the
reference checkout exists (REF below); like make_golden.py it imports the reference's ``model.py``, runs it on seeded inputs and stores
tensors and numbers -- nothing of the reference's source text.

Each case is one seeded training step of the reference in fp32 plus the same step evaluated in float64 (the pattern of make_golden.py's
run_step / pbfcn_step): loss, logits, arg-max with its near-tie list (top-2 margin < 1e-4), parameter gradients (whole tensors up to
FULL elements, the first 64 values and the norm otherwise; fp32 and float64), eval-mode logits of image 0 after the step, the cross entropy of a second
training forward.  The inputs
are oracle.cpu_reference.synthetic_batch(B, H, W) and are not stored.

    python tests/golden/make_golden_cls5.py        -> tests/golden/cls5.npz, cls5.json
"""
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 4
FULL = 1024
PB_W = [1, 6, 1.5, 3, 3]           # trainer.py:133-138
CE_W = [1, 10, 30, 10, 2]          # train.py:309-313

sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.cpu_reference import synthetic_batch      # noqa: E402


def sd_hash(sd):      # tests/conftest.py
    import hashlib
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def npy(t):
    return t.detach().cpu().contiguous().numpy()


def one_step(make, dtype, x, t, weights, adam):
    torch.manual_seed(12345678)
    model = make().to(dtype)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    crit = ref.CrossEntropyLoss2d(torch.tensor(weights, dtype=dtype))
    if adam:       # train.py:43-74: Adam, L1 term on the loss
        opt = torch.optim.Adam([{"params": model.parameters()}], lr=1e-3)
    else:          # trainer.py:205-221
        opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-1, momentum=0.5, weight_decay=1e-3)
    model.train()
    opt.zero_grad()
    pred = model(x.to(dtype))
    ce = crit(pred, t)
    loss = ce
    if adam:
        reg = 0
        for p in model.parameters():
            reg = reg + torch.sum(torch.abs(p))
        loss = ce + 1e-6 * reg
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    none_grads = [k for k, p in model.named_parameters() if p.grad is None]
    opt.step()
    model.eval()
    with torch.no_grad():
        pred_eval = model(x[:1].to(dtype))
    model.train()           # the cross entropy of a second iteration on the same batch (optimizer state, updated statistics)
    with torch.no_grad():
        ce2 = float(crit(model(x.to(dtype)), t))
    return {"ce_step2": ce2, "sd0": sd0, "pred": pred.detach(), "ce": float(ce), "loss": float(loss), "grads": grads, "none_grads": none_grads,
            "pred_eval": pred_eval}


def case(out, meta, tag, make, B, H, W, weights, adam):
    x, t = synthetic_batch(B, H, W)
    r32 = one_step(make, torch.float32, x, t, weights, adam)
    r64 = one_step(make, torch.float64, x, t, weights, adam)
    pred = r32["pred"]
    _, pc = torch.max(pred, 1)
    top2 = torch.topk(pred, 2, dim=1)[0]
    near = np.nonzero(npy(top2[:, 0] - top2[:, 1]).reshape(-1) < 1e-4)[0].astype(np.int32)
    # the reference alone must stay inside the budget the tests grant: at most 1 % near-tie pixels, and its own fp32 mask equal to
    # its float64 mask outside them
    assert near.size <= 0.01 * pc.numel(), (tag, near.size)
    pc64 = torch.max(r64["pred"], 1)[1]
    assert np.setdiff1d(np.nonzero(npy(pc != pc64).reshape(-1))[0], near).size == 0, tag
    meta[tag] = {
        "B": B, "H": H, "W": W, "adam": adam, "weights": weights, "threads": torch.get_num_threads(), "torch": torch.__version__,
        "sd_hash_init": sd_hash(r32["sd0"]), "ce": r32["ce"], "loss": r32["loss"], "ce64": r64["ce"], "ce_step2": r32["ce_step2"], "none_grads": r32["none_grads"],
        "near_ties": int(near.size),
        "grad_norm": {k: float(g.double().norm()) for k, g in r32["grads"].items()},
        "grad_norm64": {k: float(g.norm()) for k, g in r64["grads"].items()},
    }
    out[tag + "/logits"] = npy(pred)
    out[tag + "/argmax"] = npy(pc).astype(np.uint8)
    out[tag + "/near_tie_idx"] = near
    out[tag + "/eval_logits0"] = npy(r32["pred_eval"])
    for k, g in r32["grads"].items():
        g64 = r64["grads"][k].float()
        if g.numel() <= FULL:
            out["%s/grad/%s" % (tag, k)] = npy(g)
            out["%s/grad64/%s" % (tag, k)] = npy(g64)
        else:
            out["%s/grad_head/%s" % (tag, k)] = npy(g.reshape(-1)[:64])
            out["%s/grad64_head/%s" % (tag, k)] = npy(g64.reshape(-1)[:64])
    print(tag, "ce=%.8f (fp64 %.8f) near ties %d of %d" % (r32["ce"], r64["ce"], near.size, pc.numel()))


if __name__ == "__main__":
    torch.set_num_threads(THREADS)
    sys.path.insert(0, REF)
    import model as ref          # the reference, imported (never copied)
    out, meta = {}, {}
    case(out, meta, "pbfcn5_s_2x48x64", lambda: ref.PB_FCN(32, 5, 5, False, 0), 2, 48, 64, PB_W, False)      # labelPropTrain.py:90-92
    case(out, meta, "pbfcn5_l_1x64x96", lambda: ref.PB_FCN(32, 5, 5, True, 0), 1, 64, 96, PB_W, False)
    case(out, meta, "robo5_s_2x48x64", lambda: ref.ROBO_UNet(classSize=5), 2, 48, 64, CE_W, True)
    case(out, meta, "v25_s_2x48x64", lambda: ref.ROBO_UNet(v2=True, classSize=5, levels=1, bellySize=2), 2, 48, 64, CE_W, True)     # detect.py:96-100
    np.savez_compressed(os.path.join(HERE, "cls5.npz"), **out)
    with open(os.path.join(HERE, "cls5.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("cls5.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "cls5.npz")))
