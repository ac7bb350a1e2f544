#!/usr/bin/env python3
"""Time of one validation pass (valid(), train.py:97-178) per batch on the GPU box.

    python scripts/bench_validate.py [--only NAME] [--batches 8] [--min-seconds 1.0] [--repeats 5] [--no-launches] [--append FILE]

One JSON line per shape, all four paths on the same build, in one process, on one card, their windows alternating:
  network   (a) ``model(x)`` in eval mode alone: what any validation path has to pay
  evaluate  (b) ``Trainer.evaluate`` + ``SegmentationMetrics.update`` per batch, ``compute()`` at the end of the pass: the path a
                caller had before ``Trainer.validate`` (RCV_OP_CLS_FWD, RCV_OP_CE_FWD, torch.zeros, RCV_OP_CONFUSION, float64 torch ops)
  literal   (c) the same with the reference's ``losstotal += loss.item()``: one synchronisation per batch
  validate_batches  (d) the batch loop of ``Trainer.validate``: ``model.validate`` per batch (RCV_OP_CLS_VALID + RCV_OP_VALID_FOLD at
                the end of the eval plan) and ``state.compute()``, the one read-back per pass; what (b) and (c) compare with
  validate  ``Trainer.validate`` whole: (d) plus what valid() does once per pass and (b) / (c) leave out, ``decay * l1reg(model)``
                and ``count_zero_weights(model)`` (per parameter six torch launches and a read-back); ``epilogue_ms_per_pass`` is
                the difference, per pass
A pass is --batches batches of one shape (the tensors stay on the device, as an ``EpochLoader`` hands them over) and ends with the
read-back of its report, so every window ends in a synchronisation.  Each entry: median ms PER BATCH over --repeats windows of at least
--min-seconds (device events, after warm-up), spread = max - min.  ``validate_over_evaluate`` (of validate_batches) < 1 means the new path is faster;
``beyond_spread`` says whether the gap exceeds both spreads.  ``launches_per_batch``: device kernels per batch of (b) and (d), counted
by torch.profiler over one pass after the timing (null with the reason if the profiler is not usable)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd.metrics import SegmentationMetrics, ValidationState      # noqa: E402
from robocupvision_amd.train import Trainer          # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {"robo_64x120x160": (64, 120, 160), "robo_32x480x640": (32, 480, 640)}
WEIGHTS = (1, 10, 30, 10, 2)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def timed_alternating(fns, batches, min_seconds, repeats, warmup=3):
    """fns: name -> pass function.  Windows of the paths alternate, so drift of the box meets all of them alike."""
    n = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        n[name] = max(2, int(min_seconds * 1e3 / max(window(fn, 1), 1e-3)) + 1)
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            out[name].append(window(fn, n[name]) / batches)
    res = {}
    for name, v in out.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 5), "spread_ms": round(v[-1] - v[0], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5),
                     "passes_per_window": n[name], "repeats": repeats}
    return res


def compare(a, b):
    return {"ratio": round(b["ms"] / a["ms"], 4), "beyond_spread": bool(abs(a["ms"] - b["ms"]) > a["spread_ms"] + b["spread_ms"])}


def count_launches(fn, batches):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        if not kernels:
            return {"per_batch": None, "reason": "the profiler recorded no device kernels"}
        return {"per_batch": round(len(kernels) / batches, 2), "kernels_in_pass": len(kernels)}
    except Exception as exc:          # the count is a by-product: the timings above stand without it
        return {"per_batch": None, "reason": "%s: %s" % (type(exc).__name__, exc)}


def run_config(name, a):
    B, H, W = CONFIGS[name]
    torch.manual_seed(12345678)
    model = M.ROBO_UNet().to(DEV).eval()
    tr = Trainer(model, class_weights=WEIGHTS)
    batches = [(torch.randn(B, 3, H, W, device=DEV), torch.randint(0, 5, (B, H, W), device=DEV)) for _ in range(a.batches)]
    state = ValidationState(5, DEV)

    def network():
        with torch.no_grad():
            for x, _ in batches:
                model(x)
        torch.cuda.synchronize()

    def evaluate(sync_per_batch=False):
        met = SegmentationMetrics(5, DEV)
        total = torch.zeros((), dtype=torch.float64, device=DEV)
        host_total = 0.0
        for x, t in batches:
            _, loss, am = tr.evaluate(x, t)
            met.update(am, t)
            if sync_per_batch:
                host_total += loss.item()          # train.py:131
            else:
                total += loss
        out = met.compute()
        out["loss"] = (host_total if sync_per_batch else float(total)) / len(batches)
        return out

    def validate():
        state.reset()
        return tr.validate(batches, state)

    def validate_batches():
        state.reset()
        for x, t in batches:
            model.validate(x, t, state, weight=tr.criterion.weight)
        return state.compute()

    ref, got = evaluate(), validate()
    row = {"config": name, "B": B, "size": [H, W], "batches_per_pass": a.batches,
           "mean_iou_gap": abs(ref["mean_iou"] - got["mean_iou"]), "mean_class_acc_equal": bool(ref["mean_class_acc"] == got["mean_class_acc"]),
           "loss_gap": abs(ref["loss"] + got["reg"] - got["loss"])}
    fns = {"network": network, "evaluate": evaluate, "literal": lambda: evaluate(True), "validate_batches": validate_batches, "validate": validate}
    row.update(timed_alternating(fns, a.batches, a.min_seconds, a.repeats))
    row["validate_over_evaluate"] = compare(row["evaluate"], row["validate_batches"])
    row["validate_over_literal"] = compare(row["literal"], row["validate_batches"])
    row["tail_ms_evaluate"] = round(row["evaluate"]["ms"] - row["network"]["ms"], 5)
    row["tail_ms_validate"] = round(row["validate_batches"]["ms"] - row["network"]["ms"], 5)
    row["epilogue_ms_per_pass"] = round((row["validate"]["ms"] - row["validate_batches"]["ms"]) * a.batches, 4)
    if not a.no_launches:
        row["launches_per_batch"] = {"evaluate": count_launches(evaluate, a.batches), "validate_batches": count_launches(validate_batches, a.batches)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--append", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    for name in ([a.only] if a.only else list(CONFIGS)):
        line = json.dumps(run_config(name, a))
        print(line, flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
