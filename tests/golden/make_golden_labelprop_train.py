"""Golden vectors of LabelProp's training step (labelPropTrain.py:162-215).  Runs ONLY in the build container, where the reference
exists: it imports the reference's ``model.py`` and ``transform.py`` (pure PyTorch) and runs them on the CPU with 8 threads on seeded
inputs, in the style of ``make_golden_classify.py``.  Nothing of the reference's source text is stored: tensors and numbers only.

    python tests/golden/make_golden_labelprop_train.py      # writes labelprop_train_<config>.npz / labelprop_train.json next to this script

The reference's own ``LabelProp.forward`` writes ``x[:,0:8] += top`` into the output of upConv3's ReLU, which autograd of current
torch versions refuses to differentiate.  The step is therefore taken through the reference's own sub-modules with that line out of
place (``tail`` below); before anything is recorded the generator ASSERTS that this form equals ``net(x)`` bit for bit in eval mode.
The class needs the constructor wrapper of ``make_golden.py:labelprop`` (8 arguments into a 7-argument ConvPoolSimple.__init__; the
extra one is a dropout rate the block never uses).

Per configuration (tests/labelprop_restatement.py CONFIGS; frames and labels from its seeded generator, assembled by the script's
loop through the reference's ``labelToPred``): init state_dict hash, train-mode logits, weighted cross entropy, every parameter
gradient, running statistics after the step, parameter sums after SGD steps 1 and 2, the step-2 loss, eval-mode logits after step 1,
the arg-max plane and its near-tie mask (top-2 margin < 1e-4; asserted to stay below 0.2 % of the pixels), the relative distance of
every fp32 gradient from the same step evaluated in float64, for lp_4x24x32 one step with a seeded prune mask, and for lp_2x16x16 the
tail's operands.  Small configurations store tensors in full; the large one stores sums, norms and seeded samples.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.environ.get("GOLDEN_OUT") or os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import labelprop_restatement as R      # noqa: E402  (tests/: the seeded frame generator and the constants the tests share)

THREADS = 8
LOGIT_SAMPLE = 4096
GRAD_SAMPLE = 1024


def sd_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def npy(t):
    return t.detach().cpu().numpy().copy()


def make_net(ref):
    orig = ref.ConvPoolSimple.__init__

    def patched(self, inplanes, planes, size, stride, padding, dilation, bias, *_ignored):
        orig(self, inplanes, planes, size, stride, padding, dilation, bias)
    ref.ConvPoolSimple.__init__ = patched
    try:
        torch.manual_seed(12345678)
        return ref.LabelProp(5, 32, 0.0)
    finally:
        ref.ConvPoolSimple.__init__ = orig


def tail(net, x):
    """net.forward with its in-place line written out of place, through the reference's own sub-modules."""
    top = net.pre(x)
    middle = net.down1(top)
    bottom = net.down2(middle)
    y = net.down3(bottom)
    y = net.conv3(net.conv2(net.conv1(y)))
    y = bottom + net.upConv1(y)
    y = middle + net.upConv2(y)
    y = net.upConv3(y)
    y = torch.cat([y[:, 0:8] + top, y[:, 8:]], 1)
    return net.classifier(y)


def script_batch(tr, images, labels):
    """labelPropTrain.py:162-193 with the reference's labelToPred."""
    B, H, W = images.shape[0], images.shape[3], images.shape[4]
    inputs = torch.empty(2 * B, 8, H, W)
    outputs = torch.empty(2 * B, H, W, dtype=torch.int64)
    cnt = 0
    for img, lab in zip(images, labels):
        preds = tr.labelToPred(lab, 5)
        inputs[cnt] = torch.cat([img[0][0][None], img[1][0][None], (img[0][0] - img[1][0])[None], preds[1]])
        inputs[cnt + 1] = torch.cat([img[1][0][None], img[0][0][None], (img[1][0] - img[0][0])[None], preds[0]])
        outputs[cnt], outputs[cnt + 1] = lab[0], lab[1]
        cnt += 2
    return inputs, outputs


def one_step(net, opt, crit, x, t, masks=None):
    net.train()
    opt.zero_grad()
    logits = tail(net, x)
    loss = crit(logits, t)
    loss.backward()
    if masks is not None:                      # labelPropTrain.py:201-206
        k = 0
        for p in net.parameters():
            if p.dim() > 1:
                p.grad[masks[k]] = 0
                k += 1
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    return logits.detach(), float(loss.detach()), grads


def run(ref, tr, tag, out, meta):
    P, H, W, seed = R.CONFIGS[tag]
    small = tag in R.SMALL
    images, labels = R.synthetic_pairs(P, H, W, seed)
    x, t = script_batch(tr, images, labels)
    net = make_net(ref)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        assert torch.equal(tail(net, x), net(x.clone())), "the out-of-place tail must equal the reference's forward bit for bit"
    crit = torch.nn.CrossEntropyLoss(torch.tensor(R.LP_WEIGHTS))
    opt = torch.optim.SGD(net.parameters(), **R.LP_SGD)
    ops = {}
    if tag == "lp_2x16x16":
        def keep(name):          # (a forward hook that returns a value would replace the module's output: return None)
            def hook(m, i, o):
                ops.setdefault(name, o.detach().clone())
            return hook
        hooks = [net.upConv3.conv.register_forward_hook(keep("t")), net.pre.register_forward_hook(keep("top"))]
    logits, loss, grads = one_step(net, opt, crit, x, t)
    if tag == "lp_2x16x16":
        for h in hooks:
            h.remove()
        tt = ops["t"]
        out[tag + "/tail/t"] = npy(tt.permute(0, 2, 3, 1))
        out[tag + "/tail/top"] = npy(ops["top"].permute(0, 2, 3, 1))
        out[tag + "/tail/mean"] = npy(tt.double().mean((0, 2, 3)))
        out[tag + "/tail/var"] = npy(tt.double().var((0, 2, 3), unbiased=False))
        out[tag + "/tail/bn_weight"] = npy(sd0["upConv3.bn.weight"])
        out[tag + "/tail/bn_bias"] = npy(sd0["upConv3.bn.bias"])
        out[tag + "/tail/cls_weight"] = npy(sd0["classifier.weight"])
        out[tag + "/tail/cls_bias"] = npy(sd0["classifier.bias"])
    sd1 = {k: v.clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        eval_logits = tail(net, x)
    _, loss2, _ = one_step(net, opt, crit, x, t)
    sd2 = {k: v.clone() for k, v in net.state_dict().items()}

    # the same first step in float64: how far the reference's own fp32 gradients are from exact arithmetic
    net64 = make_net(ref).double()
    l64 = tail(net64.train(), x.double())
    torch.nn.CrossEntropyLoss(torch.tensor(R.LP_WEIGHTS, dtype=torch.float64))(l64, t).backward()
    g64 = {k: p.grad for k, p in net64.named_parameters()}
    # (a conv bias ahead of a BatchNorm has a gradient of exactly zero: both evaluations give rounding noise there, left out)
    rel64 = {k: float((grads[k].double() - g64[k]).norm() / float(g64[k].norm())) for k in grads
             if not (k.startswith("upConv") and k.endswith("conv.bias"))}

    top2 = torch.topk(logits, 2, dim=1)[0]
    near = (top2[:, 0] - top2[:, 1]) < R.NEAR_TIE
    npx = near.numel()
    assert int(near.sum()) <= max(1, int(R.NEAR_TIE_CAP * npx)), (tag, int(near.sum()), npx)
    am = torch.max(logits, 1)[1]
    e = {"P": P, "H": H, "W": W, "seed": seed, "threads": torch.get_num_threads(), "torch": torch.__version__,
         "sd_hash_init": sd_hash(sd0), "loss": loss, "loss_step2": loss2, "correct": int((am == t).sum()), "near_ties": int(near.sum()),
         "images_sum": float(images.double().sum()), "labels_sum": int(labels.sum()), "x_sum": float(x.double().sum()),
         "grad_norm": {k: float(g.double().norm()) for k, g in grads.items()},
         "grad_sum": {k: float(g.double().sum()) for k, g in grads.items()},
         "grad_fp32_vs_fp64_rel": rel64,
         "logits_sum": float(logits.double().sum()), "logits_abs_sum": float(logits.double().abs().sum()),
         "eval_logits_sum": float(eval_logits.double().sum()), "eval_logits_abs_sum": float(eval_logits.double().abs().sum()),
         "param_after_step_sum": {k: float(v.double().sum()) for k, v in sd1.items() if v.dtype.is_floating_point},
         "param_after_2_steps_sum": {k: float(v.double().sum()) for k, v in sd2.items() if v.dtype.is_floating_point},
         "num_batches_tracked": int(sd2["pre.bn.num_batches_tracked"])}
    out[tag + "/argmax"] = npy(am).astype(np.uint8)
    out[tag + "/near_tie"] = np.packbits(npy(near).astype(np.uint8).reshape(-1))
    for k, v in sd1.items():
        if "running" in k:
            out["%s/after/%s" % (tag, k)] = npy(v)
    if small:
        out[tag + "/images"], out[tag + "/labels"] = npy(images), npy(labels).astype(np.int64)
        out[tag + "/x"], out[tag + "/t"] = npy(x), npy(t).astype(np.int64)
        out[tag + "/logits"], out[tag + "/eval_logits"] = npy(logits), npy(eval_logits)
        for k, g in grads.items():
            out["%s/grad/%s" % (tag, k)] = npy(g)
    else:
        idx = R.sample_index(logits.numel(), tag + "/logits", LOGIT_SAMPLE)
        out[tag + "/logits_sample"] = npy(logits.reshape(-1)[idx])
        out[tag + "/eval_logits_sample"] = npy(eval_logits.reshape(-1)[idx])
        for k, g in grads.items():
            if g.numel() <= GRAD_SAMPLE:
                out["%s/grad/%s" % (tag, k)] = npy(g)
            else:
                out["%s/grad_sample/%s" % (tag, k)] = npy(g.reshape(-1)[R.sample_index(g.numel(), k, GRAD_SAMPLE)])
    if tag == R.PRUNE_TAG:
        netp = make_net(ref)
        masks = R.prune_masks(list(netp.parameters()))
        optp = torch.optim.SGD(netp.parameters(), **R.LP_SGD)
        _, lossp, gp = one_step(netp, optp, crit, x, t, masks)
        e["prune"] = {"loss": lossp, "masked": int(sum(int(m.sum()) for m in masks)),
                      "grad_norm": {k: float(g.double().norm()) for k, g in gp.items()},
                      "param_after_step_sum": {k: float(v.double().sum()) for k, v in netp.state_dict().items()
                                               if v.dtype.is_floating_point}}
    meta[tag] = e
    print(tag, "loss %.8f step2 %.8f near ties %d of %d, worst fp32-vs-fp64 gradient distance %.2e"
          % (loss, loss2, int(near.sum()), npx, max(rel64.values())))


def main():
    torch.set_num_threads(THREADS)
    sys.path.insert(0, REF)
    for name in ("cv2", "skimage", "skimage.color"):      # transform.py imports them at the top; labelToPred uses neither
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["skimage.color"], "rgb2yuv"):
        sys.modules["skimage.color"].rgb2yuv = None
    import model as ref          # the reference, imported (never copied)
    import transform as tr
    meta = {}
    for tag in R.CONFIGS:          # one archive per configuration (the three that hold every gradient in full are ~0.4 MB each)
        out = {}
        run(ref, tr, tag, out, meta)
        np.savez_compressed(os.path.join(HERE, "labelprop_train_%s.npz" % tag[3:]), **out)
    meta["_sample"] = {"logits": LOGIT_SAMPLE, "grad": GRAD_SAMPLE}
    with open(os.path.join(HERE, "labelprop_train.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
