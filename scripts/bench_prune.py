#!/usr/bin/env python3
"""Times of the prune stage (GPU box), in the style of scripts/bench_bnn.py: HIP events, warm-up, the median of alternating windows.

(a) One call of each mask builder (model.pruneModelNew / pruneModel / pruneModel2: ONE RCV_OP_PRUNE launch and one copy back) over the
    parameters of PB_FCN(32), PB_FCN_2, LabelProp and ROBO-UNet, against the same rule composed of eager torch ops on the same card
    (max / sum / std / topk and the ``float(...)`` host syncs that come with them).  The weights are restored from a copy before every
    call (outside the timed region); the time is wall clock between two device synchronisations, since host syncs are what differs.
(b) The prune-phase step of pruner.py:158-209 (PB_FCN, 160x120, batch 8, SGD, masks from pruneModel2): the masked RCV_OP_SGD launch
    against the step as it was before optim.SGD had ``set_prune_mask`` -- Trainer's literal ``p.grad[mask] = 0`` loop, one boolean
    index-put per weight tensor, then the unmasked launch.  Both run in this process, windows alternating.

    python scripts/bench_prune.py [--only a|b] [--min-seconds 0.5] [--repeats 7]

One JSON line per row."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M        # noqa: E402
from robocupvision_amd.optim import SGD    # noqa: E402
from robocupvision_amd.train import Trainer  # noqa: E402
from scripts.bench_bnn import alternate    # noqa: E402

DEV = torch.device("cuda:0")
NETS = {"PB_FCN": lambda: M.PB_FCN(32, 5, 1, False, 0), "PB_FCN_2": lambda: M.PB_FCN_2(False, nClass=5),
        "LabelProp": lambda: M.LabelProp(5, 32, 0.0), "ROBO_UNet": lambda: M.ROBO_UNet()}


# ---- the rules composed of eager torch ops (what a caller of the reference runs on the card) ----
def eager_max_ratio(params, ratio=0.01):
    out = []
    for p in params:
        if p.dim() > 1:
            p = p.data
            thresh = torch.max(torch.abs(p)) * ratio
            _ = float(torch.sum(torch.abs(p) < thresh)) / float(torch.sum(p != 0)) * 100
            p[torch.abs(p) < thresh] = 0
            out.append(torch.abs(p) < thresh)
    return out


def eager_std_search(params, lower=73, upper=77):
    out = []
    for p in params:
        if p.dim() > 1:
            p = p.data
            thresh = p.std()
            for _ in range(4096):
                num = float(torch.sum(torch.abs(p) < thresh)) / float(torch.sum(p != 0)) * 100
                if num < lower:
                    thresh *= 1.025
                elif num > upper:
                    thresh *= 0.975
                else:
                    break
            p[torch.abs(p) < thresh] = 0
            out.append(torch.abs(p) < thresh)
    return out


def eager_smallest_k(params, ratio, lT, hT):
    out = []
    for p in params:
        if p.dim() > 1:
            n = p.numel()
            r = 0 if n < 100 else (ratio * 0.8 if n < lT else ratio)
            if n > hT:
                r = ratio * 1.05
            flat = p.data.reshape(-1)
            amount = int(n * r)
            if amount > 0:
                _, idx = torch.topk(torch.abs(flat), amount, dim=0, largest=False)
                flat[idx] = 0.0
            out.append(p.data == 0.0)
    return out


def timed_calls(fn, params, saved, repeats, warmup):
    ms = []
    for k in range(warmup + repeats):
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.data.copy_(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn(params)
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 4), "spread_ms": round(ms[-1] - ms[0], 4)}


def bench_builders(repeats, warmup):
    rules = {"pruneModelNew": (lambda ps: M.pruneModelNew(ps, 0.01), lambda ps: eager_max_ratio(ps, 0.01)),
             "pruneModel": (lambda ps: M.pruneModel(ps, 73, 77), lambda ps: eager_std_search(ps, 73, 77)),
             "pruneModel2": (lambda ps: M.pruneModel2(ps, 0.3, 1000, 50000), lambda ps: eager_smallest_k(ps, 0.3, 1000, 50000))}
    for net, make in NETS.items():
        torch.manual_seed(12345678)
        params = list(make().to(DEV).parameters())
        saved = [p.detach().clone() for p in params]
        big = [p.numel() for p in params if p.dim() > 1]
        for rule, (hip, eager) in rules.items():
            row = {"bench": "builder", "net": net, "rule": rule, "tensors": len(big), "largest": max(big), "weights": sum(big)}
            # interleaved: a few calls of one side, then of the other, twice
            try:
                a1, b1 = timed_calls(hip, params, saved, repeats, warmup), timed_calls(eager, params, saved, repeats, warmup)
                a2, b2 = timed_calls(hip, params, saved, repeats, 1), timed_calls(eager, params, saved, repeats, 1)
            except M.L.RcvError as e:                       # pruneModel's search need not end on every tensor: reported, not timed
                row["refused"] = str(e)
                print(json.dumps(row), flush=True)
                continue
            row["hip"] = {"ms": min(a1["ms"], a2["ms"]), "windows": [a1, a2]}
            row["torch_eager"] = {"ms": min(b1["ms"], b2["ms"]), "windows": [b1, b2]}
            row["hip_over_torch"] = round(row["hip"]["ms"] / row["torch_eager"]["ms"], 4)
            print(json.dumps(row), flush=True)


class LoopSGD(SGD):
    """optim.SGD as it was before it took a mask: Trainer finds no ``set_prune_mask`` and runs its literal gradient-masking loop."""

    @property
    def set_prune_mask(self):
        raise AttributeError("set_prune_mask")


def bench_step(B, H, W, min_seconds, repeats, warmup):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 3, H, W, generator=g).to(DEV)
    t = torch.randint(0, 5, (B, H, W), generator=g).to(DEV)
    steps = {}
    for name, cls in (("masked_launch", SGD), ("literal_loop", LoopSGD)):
        torch.manual_seed(12345678)
        model = M.PB_FCN(32, 5, 1, False, 0).to(DEV)
        tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=cls(model, lr=1e-2, momentum=0.1, weight_decay=1e-3))
        tr.step(x, t)                                        # the engine lays the parameters out
        with contextlib.redirect_stdout(io.StringIO()):
            tr.prune("pruneModel2", ratio=0.3, lT=1000, hT=50000)
        assert hasattr(tr.optimizer, "set_prune_mask") == (cls is SGD)
        steps[name] = (lambda tr=tr: tr.step(x, t))
    res = alternate(steps, min_seconds, repeats, warmup)
    row = {"bench": "prune_phase_step", "net": "PB_FCN", "batch": B, "H": H, "W": W, **res}
    row["masked_over_loop"] = round(res["masked_launch"]["ms"] / res["literal_loop"]["ms"], 4)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["a", "b"])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.only in (None, "a"):
        bench_builders(a.repeats, 2)
    if a.only in (None, "b"):
        bench_step(8, 120, 160, a.min_seconds, a.repeats, a.warmup)


if __name__ == "__main__":
    main()
