#!/usr/bin/env python
"""Device time of the class-map cleaning functions (RCV_OP_MAP_FILTER, csrc/map_filter.hip): ``majority_filter`` (the reference's window
4, 15, 7), ``erode_map``, ``open_map``, ``close_map`` (window 3) on uint8 maps and ``trim_pseudo_labels`` (window 3) on int64 maps, C = 5,
at [64,120,160] and [32,480,640].  Against (a) the eager-torch composition on the same card -- one_hot, zero padding, avg_pool2d as the
box sum, the rule in tensor arithmetic -- and (b) the host route a user had before: .cpu(), scipy.ndimage (the numpy restatement for
the vote, which scipy has no call for), upload; (b) is timed on at most --cpu-images images and scaled to the batch.  The two device
sides alternate inside one call: --windows windows, in each --iters calls per side between two HIP events; the figure is the median
of the windows' per-call times.  bytes/s counts what the op must move: one read and one write per pixel (2 bytes for uint8, 16 for
int64).  One JSON line per (shape, function), appended to --out.

    python scripts/bench_clean.py [--iters 20] [--windows 5] [--warmup 3] [--no-cpu] [--cpu-images 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_filter_restatement as R  # noqa: E402
import objdet_restatement as OD  # noqa: E402
from robocupvision_amd import infer as I  # noqa: E402

C = 5
DEV = "cuda:0"
SHAPES = [(64, 120, 160), (32, 480, 640)]


# ---- (a) the eager composition --------------------------------------------------------------------------------------------------
def _box(x, k):
    """Sum over every pixel's window (zero outside the image): exact in fp32, the sums are small integers."""
    r0 = k // 2
    return torch.round(F.avg_pool2d(F.pad(x, (r0, k - 1 - r0, r0, k - 1 - r0)), k, stride=1) * (k * k))


def _parts(m, k):
    wide = m.long()
    isc = (wide >= 0) & (wide < C)
    v = torch.where(isc, wide, torch.zeros_like(wide))
    hot = F.one_hot(torch.where(isc, wide, torch.full_like(wide, C)), C + 1)[..., :C].permute(0, 3, 1, 2).float()
    return isc, v, hot, _box(hot, k)


def eager_majority(m, k=4, min_major=15, min_own=7):
    isc, v, _, h = _parts(m, k)
    mx, first = h.max(1)
    own = h.gather(1, v[:, None])[:, 0]
    return torch.where(isc & ((mx >= min_major) | (own < min_own)), first.to(m.dtype), m)


def eager_erode(m, n, k=3, fill=0):
    isc, v, _, h = _parts(m, k)
    return torch.where(isc & (h.gather(1, v[:, None])[:, 0] < n), torch.full_like(m, fill), m)


def eager_open(m, n, k=3, fill=0):
    isc, v, hot, h = _parts(m, k)
    kept = _box(hot * (h == n[:, None]), k) > 0
    return torch.where(isc & ~kept.gather(1, v[:, None])[:, 0], torch.full_like(m, fill), m)


def eager_close(m, n, k=3):
    isc, v, _, h = _parts(m, k)
    closed = _box((h > 0).float(), k) == n[:, None]
    out = m.clone()
    may = ~isc | (v == 0)
    for c in range(C - 1, 0, -1):          # the lowest class is written last: it wins
        out = torch.where(closed[:, c] & (may | (v == c)), torch.full_like(m, c), out)
    return out


# ---- (b) the host route ---------------------------------------------------------------------------------------------------------
def host_call(name, m):
    import scipy.ndimage as ndi
    a = m.cpu().numpy()
    st = np.ones((1, 3, 3), bool)
    if name == "majority":
        out = R.majority_filter(a)
    elif name in ("erode", "trim"):
        out = a.copy()
        for c in range(C):
            b = a == c
            out[b & ~ndi.binary_erosion(b, st, border_value=1)] = 0 if name == "erode" else -100
    elif name == "open":
        out = a.copy()
        for c in range(C):
            b = a == c
            out[b & ~ndi.binary_dilation(ndi.binary_erosion(b, st, border_value=1), st)] = 0
    else:
        out = a.copy()
        may = (a == 0) | (a >= C)
        for c in range(C - 1, 0, -1):
            out[ndi.binary_erosion(ndi.binary_dilation(a == c, st), st, border_value=1) & may] = c
    return torch.from_numpy(out).to(m.device)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host route")
    ap.add_argument("--cpu-images", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clean.py needs the GPU: there is nothing to time without one")
    for N, H, W in SHAPES:
        rng = np.random.default_rng(11)
        maps = OD.jitter(rng, OD.blob_masks(rng, N, H, W, C, 15), C, p=0.02)
        maps[rng.random(maps.shape) < 0.01] = 255
        u8 = torch.from_numpy(maps).to(torch.uint8).to(DEV)
        i64 = torch.where(u8 == 255, torch.full((), -100, dtype=torch.int64, device=DEV), u8.long())
        n3 = _box(torch.ones(1, 1, H, W, device=DEV), 3)[:, 0]
        cases = {"majority": (u8, lambda: I.majority_filter(u8), lambda: eager_majority(u8)),
                 "erode": (u8, lambda: I.erode_map(u8, C), lambda: eager_erode(u8, n3)),
                 "open": (u8, lambda: I.open_map(u8, C), lambda: eager_open(u8, n3)),
                 "close": (u8, lambda: I.close_map(u8, C), lambda: eager_close(u8, n3)),
                 "trim": (i64, lambda: I.trim_pseudo_labels(i64, C), lambda: eager_erode(i64, n3, fill=-100))}
        for name, (src, hip, eager) in cases.items():
            for _ in range(a.warmup):
                hip()
                eager()
            torch.cuda.synchronize()
            t = {"hip": [], "eager": []}
            for _ in range(a.windows):
                t["hip"].append(window_ms(hip, a.iters))
                t["eager"].append(window_ms(eager, a.iters))
            hip_ms, eager_ms = statistics.median(t["hip"]), statistics.median(t["eager"])
            moved = N * H * W * 2 * src.element_size()
            res = {"function": name, "N": N, "H": H, "W": W, "C": C, "dtype": str(src.dtype).replace("torch.", ""),
                   "window": 4 if name == "majority" else 3, "iters": a.iters, "windows": a.windows,
                   "hip_ms": round(hip_ms, 4), "hip_ms_windows": [round(x, 4) for x in t["hip"]],
                   "eager_ms": round(eager_ms, 4), "eager_ms_windows": [round(x, 4) for x in t["eager"]],
                   "eager_over_hip": round(eager_ms / hip_ms, 2), "bytes_moved": moved, "hip_GBps": round(moved / hip_ms / 1e6, 1),
                   "eager_equal": bool(torch.equal(hip(), eager()))}
            if not a.no_cpu:
                nb = min(N, a.cpu_images)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = host_call(name, src[:nb])
                torch.cuda.synchronize()
                res["host_images"] = nb
                res["host_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 * N / nb, 1)
                res["host_equal"] = bool(torch.equal(hip()[:nb], ref))
            line = json.dumps(res)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
