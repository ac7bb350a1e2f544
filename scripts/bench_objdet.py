#!/usr/bin/env python
"""Device time of one DetectionMetrics.update (RCV_OP_OBJECT_MATCH, csrc/objdet.hip) per case, HIP events, warmed up, median of
--iters; next to it the time of the numpy restatement of the same contract (tests/objdet_restatement.py) on the same data.
One JSON line per case.  --rocprof: the same run in a child process under `rocprofv3 --kernel-trace --stats` (kernel table in
--rocprof-dir).

    python scripts/bench_objdet.py [--iters 50] [--warmup 10] [--cases unet64,unet16,blob64,grid64] [--no-cpu] [--rocprof]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objdet_restatement as R  # noqa: E402
from robocupvision_amd import metrics as M  # noqa: E402

C = 5
IT, DT = M.DEFAULT_IOU_THRESHOLDS, M.DEFAULT_DIST_THRESHOLDS


def unet_argmax(B, H, W, seed):
    import robocupvision_amd.model as Mo
    torch.manual_seed(seed)
    model = Mo.ROBO_UNet().to("cuda:0").eval()
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 3, H, W)).astype(np.float32)).to("cuda:0")
    with torch.no_grad():
        return torch.max(model(x), 1)[1]


def grid(B, H, W, off):
    a = np.zeros((B, H, W), dtype=np.int64)
    a[:, off::2, off::2] = 1
    return a


def make_case(name):
    rng = np.random.default_rng(7)
    if name == "unet64":
        return unet_argmax(64, 120, 160, 1), R.blob_masks(rng, 64, 120, 160, C, 15)
    if name == "unet16":
        return unet_argmax(16, 240, 320, 2), R.blob_masks(rng, 16, 240, 320, C, 15)
    if name == "blob64":
        t = R.blob_masks(rng, 64, 120, 160, C, 15)
        return torch.from_numpy(R.jitter(rng, t, C, 0.01)).to(torch.uint8).to("cuda:0"), t
    if name == "grid64":
        return torch.from_numpy(grid(64, 120, 160, 0)).to(torch.uint8).to("cuda:0"), grid(64, 120, 160, 1)
    raise SystemExit("unknown case " + name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="unet64,unet16,blob64,grid64")
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement timing")
    ap.add_argument("--cpu-images", type=int, default=64, help="time the restatement on at most this many images of the batch")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-dir", default=os.path.join(ROOT, "out", "rocprof_objdet"))
    a = ap.parse_args()
    if a.rocprof:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof_dir, "-o", "objdet", "--", sys.executable,
               os.path.abspath(__file__), "--iters", str(a.iters), "--warmup", str(a.warmup), "--cases", a.cases, "--no-cpu"]
        sys.exit(subprocess.run(cmd).returncode)
    for name in a.cases.split(","):
        pred, target_np = make_case(name)
        target = torch.from_numpy(target_np).to("cuda:0")
        B, H, W = pred.shape
        m = M.DetectionMetrics(C, device="cuda:0")
        for _ in range(a.warmup):
            m.update(pred, target)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.update(pred, target)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        res = {"case": name, "B": B, "H": H, "W": W, "C": C, "K": len(IT), "device_ms_median": round(statistics.median(times), 4),
               "device_ms_min": round(min(times), 4), "iters": a.iters}
        t0 = time.perf_counter()
        m.compute()
        res["compute_ms_per_update"] = round((time.perf_counter() - t0) * 1e3 / (a.warmup + a.iters), 4)
        if not a.no_cpu:
            nb = min(B, a.cpu_images)
            p_np = pred.cpu().numpy()
            t0 = time.perf_counter()
            ref = R.fast(p_np[:nb], target_np[:nb], C, IT, DT)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            res["cpu_restatement_images"] = nb
            res["cpu_restatement_ms_per_update"] = round(cpu_ms * B / nb, 1)
            dev = M.object_match_counts(pred[:nb].contiguous(), target[:nb].contiguous(), C).cpu().numpy()
            res["counts_equal"] = bool(np.array_equal(dev, ref))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
