#!/usr/bin/env python3
"""Time of the assembled LabelProp training step of labelPropTrain.py:162-215 (GPU box): ``labelprop_batch`` + ``Trainer.step``
(CrossEntropyLoss2d weights (1,6,1,3,2), fused SGD lr 0.2, momentum 0.5, weight decay 1e-3) against the same step in stock
PyTorch-ROCm on the same card in the same run -- the plain-torch twin of tests/labelprop_restatement.py (eager, fp32,
torch.optim.SGD, the script's Python-loop batch assembly).  The parent of this feature cannot run the step, so the twin is the
yardstick.

    python scripts/bench_labelprop_train.py [--only NAME] [--min-seconds 1.0] [--repeats 3] [--no-twin] [--rocprof]

One JSON line per configuration: ms per step (median of the repeats, each a window of at least --min-seconds timed with device
events after warm-up) and the spread (max - min) for both, the launch counts of the training plan (forward / backward records that
launch something, a counted number), and the bytes the two tail kernels and the assembly kernel must move (from the shapes) with the
time that takes at the 8 TB/s HBM peak.  --rocprof additionally runs the HIP step in a child process under
``rocprofv3 --kernel-trace --stats`` and reports those kernels' measured average times and their share of that peak."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robocupvision_amd.model as M        # noqa: E402
from robocupvision_amd import _lib as L    # noqa: E402
from robocupvision_amd.optim import SGD    # noqa: E402
from robocupvision_amd.train import Trainer    # noqa: E402
import labelprop_restatement as R          # noqa: E402

# name -> (frame pairs, H, W): images per step = 2 x pairs
CONFIGS = {"lp_16x8x120x160": (8, 120, 160), "lp_64x8x120x160": (32, 120, 160)}
HBM_PEAK = 8e12
KERNELS = ("lp_tail_fwd_kernel", "lp_tail_bwd_kernel", "lp_batch_kernel")


def kernel_bytes(P, H, W, nC=5):
    """Bytes each new kernel must move once (fp32; int64 labels 8 B, arg-max 1 B per pixel; constants and filters excluded)."""
    px = 2 * P * H * W
    return {"lp_tail_fwd_kernel": px * (4 * (16 + 8 + nC) + 8 + 1),            # t, top in; logits, arg-max out; target in
            "lp_tail_bwd_kernel": px * (4 * (16 + 8) + 8 + 4 * (16 + 8)),          # t, top, target in; g and g[0:8] out
            "lp_batch_kernel": P * H * W * (2 * 4 + 2 * 8 + 2 * 8 * 4 + 2 * 8)}    # 2 frames' channel 0, 2 label planes in; 2 samples, 2 targets out


def timed(step, min_seconds, repeats, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    n = max(5, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    out.sort()
    return {"ms": round(out[len(out) // 2], 4), "spread_ms": round(out[-1] - out[0], 4), "steps_per_window": n, "all_ms": [round(v, 4) for v in out]}


def run_config(name, min_seconds, repeats, warmup, twin=True, hip=True):
    P, H, W = CONFIGS[name]
    dev = torch.device("cuda:0")
    images, labels = R.synthetic_pairs(P, H, W, 14)
    images, labels = images.to(dev), labels.to(dev)
    row = {"config": name, "pairs": P, "images": 2 * P, "H": H, "W": W}
    if hip:
        torch.manual_seed(12345678)
        model = M.LabelProp(5, 32, 0.0).to(dev)
        tr = Trainer(model, class_weights=R.LP_WEIGHTS, optimizer=SGD(model, **R.LP_SGD))

        def step():
            x, t = M.labelprop_batch(images, labels)
            tr.step(x, t)
        row["hip"] = timed(step, min_seconds, repeats, warmup)
        row["hip"]["loss"] = tr.pop_metrics()["loss"]
        plan = model._get_engine()._last[0]
        count = lambda ops: sum(ops.arr[k].kind != L.OP_NOP for k in range(ops.n))      # noqa: E731
        row["launch_records"] = {"forward": count(plan.ce["fwd"]), "backward": count(plan.ce["bwd"]), "assembly": 1, "optimizer": 1}
        kb = kernel_bytes(P, H, W)
        row["bytes"] = {k: {"MB": round(v / 1e6, 3), "us_at_8TBps_hbm_peak": round(v / HBM_PEAK * 1e6, 3)} for k, v in kb.items()}
    if twin:
        try:
            torch.manual_seed(12345678)
            net = R.LabelPropTwin().to(dev).train()
            crit = torch.nn.CrossEntropyLoss(torch.tensor(R.LP_WEIGHTS, device=dev))
            opt = torch.optim.SGD(net.parameters(), **R.LP_SGD)

            def tstep():
                x, t = R.loop_assembly(images, labels)
                opt.zero_grad()
                loss = crit(net(x), t)
                loss.backward()
                opt.step()
                return loss
            row["torch_eager"] = timed(tstep, min_seconds, repeats, warmup)
            row["torch_eager"]["loss"] = float(tstep().detach())
            if hip:
                row["hip_over_torch"] = round(row["hip"]["ms"] / row["torch_eager"]["ms"], 4)
        except Exception as exc:          # e.g. a MIOpen problem of the installed torch: report the HIP time alone and say why
            row["torch_eager"] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
    return row


def rocprof_kernels(name, warmup):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--only", name, "--min-seconds", "0.2", "--repeats", "1", "--warmup", str(warmup), "--no-twin"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=ROOT, timeout=300)      # (a hung child is killed, not waited for)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv from rocprofv3"}
        kb = kernel_bytes(*CONFIGS[name])
        total, per = 0.0, {}
        with open(files[0]) as f:
            for rec in csv.DictReader(f):
                total += float(rec["TotalDurationNs"])
                for k in KERNELS:
                    if k in rec["Name"]:
                        avg = float(rec["AverageNs"])
                        per[k] = {"calls": int(rec["Calls"]), "avg_us": round(avg / 1e3, 3), "share_of_kernel_time": float(rec["TotalDurationNs"]),
                                  "TBps": round(kb[k] / (avg * 1e-9) / 1e12, 3), "share_of_8TBps_hbm_peak": round(kb[k] / (avg * 1e-9) / HBM_PEAK, 4)}
        for v in per.values():
            v["share_of_kernel_time"] = round(v["share_of_kernel_time"] / total, 4) if total else None
        return {"kernels": per, "kernel_ms_total": round(total / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    for name in ([a.only] if a.only else list(CONFIGS)):
        row = run_config(name, a.min_seconds, a.repeats, a.warmup, twin=not a.no_twin)
        if a.rocprof:
            row["rocprof"] = rocprof_kernels(name, a.warmup)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
