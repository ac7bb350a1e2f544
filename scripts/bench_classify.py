#!/usr/bin/env python3
"""Throughput of the patch-classification step of classTrainer.py:118-135 (GPU box): forward, torch.squeeze, stock
torch.nn.CrossEntropyLoss on the squeezed logits, backward, torch.optim.SGD(lr 1e-2, momentum .9, weight decay 1e-5).

    python scripts/bench_classify.py [--steps 50] [--warmup 10] [--only NAME] [--rocprof]

One JSON line per configuration: patches/s of the whole step, and the pooled head's two records (RCV_OP_POOL_CLS_FWD / _BWD) timed
alone with HIP events (Engine.profile_last) with their algorithmic bytes and GB/s.  --rocprof additionally runs every configuration in
a child process under ``rocprofv3 --kernel-trace --stats`` and reports the head kernels' share of the step's kernel time."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M        # noqa: E402

CONFIGS = {
    "pbfcn_c5_bs32_32x32": (lambda: M.PB_FCN(32, 5, 1, False, 1), 32, 32, 32),
    "pbfcn2_c5_bs64_32x32": (lambda: M.PB_FCN_2(True), 64, 32, 32),
    "pbfcn2_c5_bs32_120x160": (lambda: M.PB_FCN_2(True), 32, 120, 160),
}
HEAD_KERNELS = ("pool_cls_fwd_kernel", "pool_cls_bwd_head_kernel", "pool_cls_scatter_kernel")


def run_config(name, steps, warmup, profile=True):
    make, bs, H, W = CONFIGS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(12345678)
    model = make().to(dev).train()
    crit = torch.nn.CrossEntropyLoss(torch.ones(5, device=dev))
    opt = torch.optim.SGD([{"params": model.parameters()}], lr=1e-2, momentum=0.9, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 5, (bs,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        pred = torch.squeeze(model(x))
        loss = crit(pred, t)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    e1.synchronize()
    wall = (time.perf_counter() - t0) / steps
    ms = e0.elapsed_time(e1) / steps
    row = {"config": name, "bs": bs, "H": H, "W": W, "steps": steps, "ms_per_step": round(ms, 4), "wall_ms_per_step": round(wall * 1e3, 4),
           "patches_per_s": round(bs / (ms / 1e3), 1), "loss": float(loss)}
    if not profile:
        return row
    eng = model._get_engine()
    step()
    for r in eng.profile_last(reps=5, with_loss=False):
        if r["label"].startswith("pool_cls"):
            key = "head_bwd" if r["bwd"] else "head_fwd"
            row[key] = {"label": r["label"], "ms": round(r["ms"], 5), "MB": round(r["bytes"] / 1e6, 3),
                        "GBps": round(r["bytes"] / (r["ms"] * 1e-3) / 1e9, 1) if r["ms"] > 0 else None}
    return row


def rocprof_share(name, steps, warmup):
    """Kernel-time share of the head kernels in a rocprofv3 --kernel-trace --stats run of this configuration (child process)."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--only", name, "--steps", str(steps), "--warmup", str(warmup), "--no-profile-last"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=ROOT, timeout=300)      # (a hung child is killed, not waited for)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv from rocprofv3"}
        total, head, per = 0.0, 0.0, {}
        with open(files[0]) as f:
            for rec in csv.DictReader(f):
                ns = float(rec["TotalDurationNs"])
                total += ns
                if any(k in rec["Name"] for k in HEAD_KERNELS):
                    head += ns
                    kname = next(k for k in HEAD_KERNELS if k in rec["Name"])
                    per[kname] = {"calls": int(rec["Calls"]), "avg_us": round(float(rec["AverageNs"]) / 1e3, 3)}
        return {"head_share_of_kernel_time": round(head / total, 4) if total else None, "kernels": per,
                "kernel_ms_total": round(total / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-profile-last", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [a.only] if a.only else list(CONFIGS)
    for name in names:
        row = run_config(name, a.steps, a.warmup, profile=not a.no_profile_last)      # (the rocprofv3 child: the timed steps only)
        if a.rocprof:
            row["rocprof"] = rocprof_share(name, a.steps, a.warmup)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
