#!/usr/bin/env python3
"""Time of the patch-classifier step of objDetEval.py:113-119 (GPU box): B = 64 patches of 32x32, ``torch.squeeze``, stock
``torch.nn.CrossEntropyLoss`` and stock ``torch.optim.SGD(lr 1e-2, momentum .9, weight decay 5e-4)`` around ``BNNL`` / ``BNNMC`` of this
package, against the same networks in stock PyTorch-ROCm (eager, fp32) on the same card.  The two alternate in ONE process: a window of
the device path, a window of the eager twin, and again, so both see the same clocks.  Also the eval forward (``predict`` against
``model(x)`` + ``torch.max``).

    python scripts/bench_bnn.py [--only BNNL|BNNMC] [--min-seconds 0.5] [--repeats 5] [--batch 64]

One JSON line per net: ms per step (median of the windows) and the spread for both sides, patches per second, the library launches of
the device step (counted from the plan: forward records, backward records x 2 -- kernel + row reduction; the two torch launches that
draw the keep-scales are reported apart as an assumption) and ``hip_over_torch`` (below 1 = the device path is faster).  The bar is 1, without a margin."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M        # noqa: E402

WEIGHTS = (1.0, 2.0, 0.5, 3.0)
SGD = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)


class Twin(nn.Module):
    """The same network out of stock torch layers, parameters copied from the device module."""

    def __init__(self, m):
        super().__init__()
        self.head = hasattr(m, "fc")
        convs = [m.conv1, m.conv2, m.conv3] + ([m.fc] if self.head else []) + [m.classifier]
        self.convs = nn.ModuleList([nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, padding=c.padding) for c in convs])
        self.pools = nn.ModuleList([nn.MaxPool2d(p.kernel_size, p.stride) for p in (m.pool1, m.pool2, m.pool3)])
        self.dos = nn.ModuleList([nn.Dropout2d(0.25) for _ in range(3)])
        self.dof = nn.Dropout(0.5)
        self.relu = nn.ReLU()
        with torch.no_grad():
            for a, b in zip(self.convs, convs):
                a.weight.copy_(b.weight)
                a.bias.copy_(b.bias)

    def forward(self, x):
        for k in range(3):
            x = self.relu(self.pools[k](self.dos[k](self.convs[k](x))))
        if self.head:
            x = self.relu(self.dof(self.convs[3](x)))
        return self.convs[-1](x)


def window(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(steps, min_seconds, repeats, warmup):
    """steps: name -> callable.  Returns name -> {ms, spread_ms, all_ms}; the windows of the callables alternate."""
    counts = {}
    for name, step in steps.items():
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        counts[name] = max(5, int(min_seconds * 1e3 / max(window(step, 5), 1e-3)) + 1)
    out = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            out[name].append(window(step, counts[name]))
    res = {}
    for name, v in out.items():
        v = sorted(v)
        res[name] = {"ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4), "steps_per_window": counts[name], "all_ms": [round(t, 4) for t in v]}
    return res


def run(net, B, min_seconds, repeats, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    t = torch.randint(0, 4, (B,), generator=g).to(dev)
    torch.manual_seed(12345678)
    model = getattr(M, net)().to(dev)
    twin = Twin(model).to(dev)
    crit = torch.nn.CrossEntropyLoss(torch.tensor(WEIGHTS, device=dev))

    def make_step(m):
        opt = torch.optim.SGD([{"params": m.parameters()}], **SGD)

        def step():
            opt.zero_grad()
            pred = torch.squeeze(m(x))
            loss = crit(pred, t)
            loss.backward()
            opt.step()
            return loss
        return step
    model.train()
    twin.train()
    row = {"net": net, "batch": B, "H": 32, "W": 32}
    tr = alternate({"hip": make_step(model), "torch_eager": make_step(twin)}, min_seconds, repeats, warmup)
    plan = model._last_plan
    f, b = plan.launches()
    row["train"] = tr
    # forward / backward: counted from the plan's records (a backward record = kernel + row reduction).  The keep-scale draw is two
    # torch calls (bernoulli(out=), mul_), ASSUMED to be one launch each: nothing here counts torch's launches
    draw = 2 if (plan.keep_views is not None and model.__dict__.get("_imposed") is None) else 0
    row["train"]["launches"] = {"forward": f, "backward": b, "library_total": f + b, "dropout_draw_assumed": draw}
    row["train"]["patches_per_s"] = round(B / (tr["hip"]["ms"] * 1e-3))
    row["train"]["hip_over_torch"] = round(tr["hip"]["ms"] / tr["torch_eager"]["ms"], 4)
    model.eval()
    twin.eval()

    def hip_eval():
        return model.predict(x)

    def torch_eval():
        with torch.no_grad():
            return torch.max(torch.squeeze(twin(x)), 1)[1]
    ev = alternate({"hip": hip_eval, "torch_eager": torch_eval}, min_seconds, repeats, warmup)
    row["eval"] = ev
    row["eval"]["launches"] = plan.launches()[0]
    row["eval"]["patches_per_s"] = round(B / (ev["hip"]["ms"] * 1e-3))
    row["eval"]["hip_over_torch"] = round(ev["hip"]["ms"] / ev["torch_eager"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["BNNL", "BNNMC"])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    for net in ([a.only] if a.only else ["BNNL", "BNNMC"]):
        print(json.dumps(run(net, a.batch, a.min_seconds, a.repeats, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
