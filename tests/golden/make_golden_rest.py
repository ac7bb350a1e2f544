"""Golden vectors for the rest of the reference's ``model.py``: FCN (model.py:311-330) with the trained weights the reference ships
for it, its ConvPoolDouble block (model.py:144-164) and the separable blocks ConvSep / trConvSep (model.py:333-377).  Runs only
where the reference checkout exists.

It imports the reference's ``model.py`` on the CPU at 8 threads and stores TENSORS only -- inputs, parameters, outputs, gradients,
key / shape lists -- never program text.  The checkpoints themselves are not copied: their parameter arrays are stored as float32
(weights are data).

    python tests/golden/make_golden_rest.py

Writes rest.json and rest_kats_<i>.npz (block vectors in the key scheme of layer_kats.npz, the FCN step in the scheme of pbfcn.npz,
the eval vectors of both checkpoints) and rest_seg1_<i>.npz / rest_seg1_pruned_<i>.npz (the parameter arrays).  Every array set is cut
into numbered parts of at most PART_BYTES of raw data, so that no file passes 1 MiB; a reader takes the union of the parts.
"""
import json
import os
import sys

import numpy as np
import torch

HERE_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE_DIR)
import make_golden as G      # noqa: E402  (sd_hash, npy, block_kat: the shared recipe)

REF = G.REF
HERE = G.HERE
CKPTS = {"seg1": "bestModelSeg1.pth", "seg1_finetuned": "bestModelSeg1Finetuned.pth", "seg1_pruned": "bestModelSeg1FinetunedPruned.pth"}
STORED = ("seg1", "seg1_pruned")
EVAL_SHAPES = [(2, 3, 48, 64), (1, 3, 120, 160)]
PB_W = (1, 6, 1.5, 3, 3)
PART_BYTES = 900 * 1024


def save_parts(prefix, arrays):
    """arrays -> prefix_0.npz, prefix_1.npz, ...: keys in order, a new part whenever the raw bytes would pass PART_BYTES."""
    for old in os.listdir(HERE):
        if old.startswith(prefix + "_") and old.endswith(".npz") and old[len(prefix) + 1:-4].isdigit():
            os.remove(os.path.join(HERE, old))
    part, size, n = {}, 0, 0
    for k, v in arrays.items():
        if part and size + v.nbytes > PART_BYTES:
            np.savez_compressed(os.path.join(HERE, "%s_%d.npz" % (prefix, n)), **part)
            part, size, n = {}, 0, n + 1
        part[k] = v
        size += v.nbytes
    np.savez_compressed(os.path.join(HERE, "%s_%d.npz" % (prefix, n)), **part)


def fcn_step(ref, out, meta, tag, B, H, W):
    """trainer.py:205-221 on FCN, two iterations: the recipe of make_golden.pbfcn_step with the model swapped."""
    torch.manual_seed(12345678)
    model = ref.FCN()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    gg = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, H, W, generator=gg)
    t = torch.randint(0, 5, (B, H, W), generator=gg)
    crit = ref.CrossEntropyLoss2d(torch.tensor(list(PB_W), dtype=torch.float32))
    opt = torch.optim.SGD([{'params': model.parameters()}], lr=1e-1, momentum=0.5, weight_decay=1e-3)
    model.train()
    losses = []
    for it in range(2):
        opt.zero_grad()
        pred = model(x)
        loss = crit(pred, t)
        loss.backward()
        if it == 0:
            pred0 = pred.detach().clone()
            grads0 = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            none_grads = [k for k, p in model.named_parameters() if p.grad is None]
            gsum = {k: [float(g.double().sum()), float(g.double().abs().sum()), float(g.double().norm())] for k, g in grads0.items()}
            gnorm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads0.values())))
        opt.step()
        losses.append(float(loss))
        if it == 0:
            sd1 = {k: v.clone() for k, v in model.state_dict().items()}
    sd2 = model.state_dict()
    _, pc = torch.max(pred0, 1)
    top2 = torch.topk(pred0, 2, dim=1)[0]
    margin = top2[:, 0] - top2[:, 1]
    model.eval()
    with torch.no_grad():
        pred_eval = model(x)
    meta[tag] = {
        "B": B, "H": H, "W": W, "threads": torch.get_num_threads(), "torch": torch.__version__,
        "sd_hash_init": G.sd_hash(sd0), "sd_hash_after_step": G.sd_hash(sd1), "sd_hash_after_2_steps": G.sd_hash(sd2),
        "loss": losses[0], "loss_step2": losses[1], "grad_norm": gnorm, "grad_summary": gsum, "none_grads": none_grads,
        "argmax_hist": [int((pc == c).sum()) for c in range(5)], "correct": int((pc == t).sum()),
        "near_ties": int((margin < 1e-4).sum()),
        "param_after_step_sum": {k: float(v.double().sum()) for k, v in sd1.items() if v.dtype.is_floating_point},
        "param_after_2_steps_sum": {k: float(v.double().sum()) for k, v in sd2.items() if v.dtype.is_floating_point},
    }
    out[tag + "/argmax"] = G.npy(pc).astype(np.uint8)
    out[tag + "/near_tie_idx"] = np.nonzero(G.npy(margin).reshape(-1) < 1e-4)[0].astype(np.int32)
    out[tag + "/x"] = G.npy(x)
    out[tag + "/t"] = G.npy(t).astype(np.int64)
    out[tag + "/logits"] = G.npy(pred0)
    out[tag + "/eval_logits"] = G.npy(pred_eval)
    for k, gr in grads0.items():
        if gr.numel() <= 4096:
            out["%s/grad/%s" % (tag, k)] = G.npy(gr)
        else:
            out["%s/grad_head/%s" % (tag, k)] = G.npy(gr.reshape(-1)[:64])
    for k, v in sd1.items():
        if "running" in k:
            out["%s/after/%s" % (tag, k)] = G.npy(v)
    print(tag, "loss=%.8f / %.8f gnorm=%.8f near ties %d" % (losses[0], losses[1], gnorm, meta[tag]["near_ties"]))


def checkpoints(ref, out, meta):
    """Key / shape lists of the three FCN checkpoints, the parameter arrays of two of them, and eval vectors of those two."""
    crit = ref.CrossEntropyLoss2d(torch.tensor(list(PB_W), dtype=torch.float32))
    meta["checkpoints"] = {}
    for name, fname in CKPTS.items():
        sd = torch.load(os.path.join(REF, "pth", fname), map_location="cpu")
        model = ref.FCN()
        model.load_state_dict(sd, strict=True)
        info = {"keys": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()],
                "elements": int(sum(v.numel() for v in sd.values())), "sd_hash": G.sd_hash(model.state_dict()),
                "count_zero_weights": ref.count_zero_weights(model),
                "conv_weights_zero": float(sum(int((p == 0).sum()) for p in model.parameters() if p.dim() > 1))
                / float(sum(p.numel() for p in model.parameters() if p.dim() > 1))}
        meta["checkpoints"][name] = info
        print(name, len(sd), "keys", info["elements"], "elements, count_zero_weights %.6f, zero conv weights %.4f"
              % (info["count_zero_weights"], info["conv_weights_zero"]))
        if name not in STORED:
            continue
        save_parts("rest_%s" % name, {k: G.npy(v) for k, v in model.state_dict().items()})
        model.eval()
        info["eval"] = {}
        for shape in EVAL_SHAPES:
            tag = "%s_%s" % (name, "x".join(map(str, shape)))
            gg = torch.Generator().manual_seed(1)
            x = torch.randn(*shape, generator=gg)
            t = torch.randint(0, 5, (shape[0],) + shape[2:], generator=gg)
            with torch.no_grad():
                pred = model(x)
                loss = float(crit(pred, t))
            _, pc = torch.max(pred, 1)
            top2 = torch.topk(pred, 2, dim=1)[0]
            margin = (top2[:, 0] - top2[:, 1]).reshape(-1)
            out[tag + "/logits"] = G.npy(pred)
            out[tag + "/t"] = G.npy(t).astype(np.int64)
            out[tag + "/argmax"] = G.npy(pc).astype(np.uint8)
            out[tag + "/near_tie_idx"] = np.nonzero(G.npy(margin) < 1e-4)[0].astype(np.int32)
            info["eval"][tag] = {"shape": list(shape), "loss": loss, "near_ties": int((margin < 1e-4).sum()),
                                 "argmax_hist": [int((pc == c).sum()) for c in range(5)], "correct": int((pc == t).sum())}
            print(" ", tag, "loss %.8f near ties %d hist %s" % (loss, info["eval"][tag]["near_ties"], info["eval"][tag]["argmax_hist"]))


def main():
    torch.set_num_threads(G.THREADS)
    sys.path.insert(0, REF)
    import model as ref
    out, meta = {}, {}
    g = torch.Generator().manual_seed(5059)
    torch.manual_seed(11)
    G.block_kat(ref, out, "cpd_16_32", ref.ConvPoolDouble(16, 32), torch.randn(2, 16, 12, 16, generator=g), 500)
    G.block_kat(ref, out, "cpd_32_64", ref.ConvPoolDouble(32, 64), torch.randn(2, 32, 10, 14, generator=g), 501)
    # the separable blocks (model.py:333-377) at the shapes of tests/test_gpu_rest.py: odd planes, more pixels than a tile is
    # never reached at these sizes -- the pointwise records themselves are checked against float64 at larger ones
    G.block_kat(ref, out, "convsep_16_32_s1", ref.ConvSep(16, 32, 3, 1), torch.randn(2, 16, 9, 13, generator=g), 502)
    G.block_kat(ref, out, "convsep_16_32_s2", ref.ConvSep(16, 32, 3, 2), torch.randn(2, 16, 10, 14, generator=g), 503)
    G.block_kat(ref, out, "trconvsep_32_16", ref.trConvSep(32, 16), torch.randn(2, 32, 5, 7, generator=g), 504)
    G.block_kat(ref, out, "convsep_64_128_s1", ref.ConvSep(64, 128, 3, 1), torch.randn(1, 64, 6, 10, generator=g), 505)
    G.block_kat(ref, out, "trconvsep_128_64", ref.trConvSep(128, 64), torch.randn(1, 128, 3, 5, generator=g), 506)
    meta["sd_hash"] = {}
    for what, make in (("FCN()", lambda: ref.FCN()), ("ConvSep(16,32,3,1)", lambda: ref.ConvSep(16, 32, 3, 1)),
                       ("ConvSep(16,32,3,2)", lambda: ref.ConvSep(16, 32, 3, 2)), ("trConvSep(32,16)", lambda: ref.trConvSep(32, 16)),
                       ("ConvPoolDouble(16,32)", lambda: ref.ConvPoolDouble(16, 32)), ("DownSamplerThick(32)", lambda: ref.DownSamplerThick(32))):
        torch.manual_seed(12345678)
        meta["sd_hash"][what] = G.sd_hash(make().state_dict())
    fcn_step(ref, out, meta, "fcn_2x48x64", 2, 48, 64)
    checkpoints(ref, out, meta)
    save_parts("rest_kats", out)
    with open(os.path.join(HERE, "rest.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
