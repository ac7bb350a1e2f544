#!/usr/bin/env python
"""Device time of one find_objects call (RCV_OP_OBJECTS, csrc/objects.hip) per case: HIP events, warmed up, median of --iters.  Every
sample of a case times, one after the other in the same loop, the library's route, the general form, the single-launch LDS form
(where the plane fits) and -- the one bar -- DetectionMetrics.update(map, map) on the same maps (RCV_OP_OBJECT_MATCH: twice the planes,
the pair hash and the matcher).  Next to it the host alternative a user had before: .cpu() + the numpy restatement, timed on at most
--cpu-images images and scaled to the batch.  One JSON line per case, appended to --out.

    python scripts/bench_objects.py [--iters 30] [--warmup 5] [--cases blob64,blob8,blob1,blob16_240,blob1_480,speckle64]  (blob<B>[_240|_480], speckle<B>) [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objdet_restatement as R  # noqa: E402
import objects_restatement as OR  # noqa: E402
from robocupvision_amd import _lib as L  # noqa: E402
from robocupvision_amd import infer as I  # noqa: E402
from robocupvision_amd import metrics as M  # noqa: E402

C = 5
DEV = "cuda:0"
DEFAULT_CASES = "blob64,blob8,blob1,blob16_240,blob1_480,speckle64"
SIZES = {"": (120, 160), "240": (240, 320), "480": (480, 640)}
RULES = {k: v for k, v in I.DBCONVERT.items() if k != "num_class"}


def make_case(name):
    kind, _, size = name.partition("_")          # blob<B>[_240|_480], speckle<B>[...]
    B = int(kind.lstrip("abcdefghijklmnopqrstuvwxyz"))
    H, W = SIZES[size]
    if name.startswith("speckle"):          # arg-max of a seeded, untrained ROBO_UNet: thousands of small components
        import robocupvision_amd.model as Mo
        torch.manual_seed(1)
        model = Mo.ROBO_UNet().to(DEV).eval()
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
        with torch.no_grad():
            return torch.max(model(x), 1)[1].to(torch.uint8)
    return torch.from_numpy(R.blob_masks(np.random.default_rng(7), B, H, W, C, 15)).to(torch.uint8).to(DEV)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host alternative")
    ap.add_argument("--cpu-images", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objects.py needs the GPU: there is nothing to time without one")
    h = L.handle(0)
    for name in a.cases.split(","):
        maps = make_case(name)
        B, H, W = maps.shape
        fits = ((H + 1) // 2) * ((W + 1) // 2) <= 7680
        m = M.DetectionMetrics(C, device=DEV)
        calls = {"route": lambda: I.find_objects(maps, C, **RULES), "general": lambda: I.find_objects(maps, C, _form=1, **RULES),
                 "object_match": lambda: m.update(maps, maps)}
        if fits:
            calls["lds"] = lambda: I.find_objects(maps, C, _form=2, **RULES)
        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(a.iters):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        m.reset()
        res = {"case": name, "B": B, "H": H, "W": W, "C": C, "rules": "DBCONVERT", "iters": a.iters,
               "label": L.OpList([I.ObjectsRecord(B, H, W, C, **RULES).op]).labels(h)[0]}
        for k, v in times.items():
            res[k + "_ms_median"] = round(statistics.median(v), 4)
            res[k + "_ms_min"] = round(min(v), 4)
        o = I.find_objects(maps, C, **RULES)
        res["components"] = int(o.counts[..., 0].sum())
        res["emitted"] = int(o.counts[..., 3].sum())
        if fits:
            g, s = I.find_objects(maps, C, _form=1, **RULES), I.find_objects(maps, C, _form=2, **RULES)
            res["forms_equal"] = bool(torch.equal(g.rows, s.rows) and torch.equal(g.counts, s.counts))
        if not a.no_cpu:
            nb = min(B, a.cpu_images)
            t0 = time.perf_counter()
            ref = OR.find_objects(maps[:nb].cpu().numpy(), C, RULES["min_area"], RULES["min_ratio"], RULES["max_objects"])
            res["host_images"] = nb
            res["host_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 * B / nb, 1)
            res["rows_equal"] = bool(np.array_equal(o.rows[:nb].cpu().numpy(), ref[0]) and np.array_equal(o.counts[:nb].cpu().numpy(), ref[1]))
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
