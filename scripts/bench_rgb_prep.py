#!/usr/bin/env python3
"""Time of ``prepare_rgb_batch`` (RCV_OP_RGB_PREP: the RGB loader of trainer.py:75-123 for a whole batch -- Scale, flips, PIL
ColorJitter, rgb2yuv, Normalize, maskLabel) on the GPU box, against what it replaces.

    python scripts/bench_rgb_prep.py [--only NAME] [--min-seconds 0.5] [--repeats 5] [--no-host] [--no-step]
    python scripts/bench_rgb_prep.py --loop 200 [--only NAME]            # nothing timed: calls for a kernel trace of the profiler
    python scripts/bench_rgb_prep.py --kernel-stats kernel_stats.csv     # one JSON line from the profiler's per-kernel statistics

One JSON line per configuration:
  hip               median ms of one ``prepare_rgb_batch`` call in training mode, parameter rows on the device (both launches, no host
                    work but the call itself), over the repeats (each a window of at least --min-seconds timed with device events
                    after warm-up), the spread (max - min), and the share of the 8 TB/s HBM peak the bytes below reach
  hip_host_rows     the same with the rows on the host, as ``draw_color_jitter`` returns them: the rows are checked and uploaded
  hip_no_contrast   training mode with the contrast taken out of every row: the statistics launch is skipped (one launch)
  hip_validation    validation mode (one launch, no operations)
  bytes             what the main launch must move, from the shapes: every frame byte in, the gathered label elements in, the fp32
                    NCHW batch and the int64 targets out; and the time that takes at 8 TB/s
  host              the chain the reference runs per image on the host, as Pillow's own calls (tests/rgb_prep_restatement.py
                    ``pillow_image``; the float64 YUV step in NumPy), on --host-threads threads (default 16), stacked and uploaded:
                    ms per batch, end to end with a device synchronise
  step              for context, ms of one SGD step of PB_FCN (trainer.py) on the prepared batch, same run
The time of the statistics launch alone comes from a kernel trace (--loop under the profiler, then --kernel-stats).  The parent of
this feature cannot run the path at all."""
import argparse
import csv
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd import data as D              # noqa: E402
from robocupvision_amd.optim import SGD              # noqa: E402
from robocupvision_amd.train import Trainer          # noqa: E402
import rgb_prep_restatement as R                     # noqa: E402

# name -> (B, (Hs, Ws), scale, labels)
CONFIGS = {"b32_480x640_to_120x160": (32, (480, 640), 4, True), "b64_patches_32x32": (64, (32, 32), 1, False),
           "b8_480x640_no_scale": (8, (480, 640), 1, True)}
HBM_PEAK = 8e12


def timed(fn, min_seconds, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    n = max(5, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    out.sort()
    return {"ms": round(out[len(out) // 2], 5), "spread_ms": round(out[-1] - out[0], 5), "min_ms": round(out[0], 5), "max_ms": round(out[-1], 5),
            "calls_per_window": n, "repeats": repeats}


def make_inputs(name):
    B, src, scale, with_labels = CONFIGS[name]
    frames_h, labels_h = R.synthetic_frames(min(B, 4), src[0], src[1], 31)
    reps = (B + len(frames_h) - 1) // len(frames_h)
    frames_h, labels_h = np.concatenate([frames_h] * reps)[:B], np.concatenate([labels_h] * reps)[:B]
    random.seed(32)
    np.random.seed(32)
    rows = D.draw_color_jitter(B)
    return B, src, scale, frames_h, (labels_h if with_labels else None), rows


def run_config(name, a):
    B, src, scale, frames_h, labels_h, rows = make_inputs(name)
    size = R.scaled_size(src[0], src[1], scale)
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(frames_h).to(dev)
    labels = None if labels_h is None else torch.from_numpy(labels_h).to(dev)
    rows_d = rows.to(dev)
    no_c = rows.clone()                                   # the contrast taken out of every row
    for b in range(B):
        ops = [v for v in no_c[b, 3:7].tolist() if v != D.OP_CONTRAST]
        no_c[b, 2], no_c[b, 3:7] = 3, torch.tensor(ops + [-1.0])
    flags = (False, False, True, False)
    kw = dict(scale=scale, no_ball=flags[0], no_robot=flags[1], no_goal=flags[2], no_line=flags[3])
    if a.loop:
        for _ in range(a.loop):
            D.prepare_rgb_batch(frames, labels, params=rows_d, **kw)
        torch.cuda.synchronize()
        return {"config": name, "looped": a.loop}
    row = {"config": name, "B": B, "src": list(src), "size": list(size), "labels": labels is not None}
    nbytes = B * (src[0] * src[1] * 3 + size[0] * size[1] * ((labels.element_size() + 8 if labels is not None else 0) + 3 * 4))
    row["bytes"] = {"MB": round(nbytes / 1e6, 3), "us_at_8TBps_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 3)}
    t = lambda fn: timed(fn, a.min_seconds, a.repeats, a.warmup)          # noqa: E731
    row["hip"] = t(lambda: D.prepare_rgb_batch(frames, labels, params=rows_d, **kw))
    row["hip"]["share_of_8TBps_hbm_peak"] = round(nbytes / (row["hip"]["ms"] * 1e-3) / HBM_PEAK, 4)
    row["hip_host_rows"] = t(lambda: D.prepare_rgb_batch(frames, labels, params=rows, **kw))
    row["hip_no_contrast"] = t(lambda: D.prepare_rgb_batch(frames, labels, params=no_c, **kw))
    row["hip_validation"] = t(lambda: D.prepare_rgb_batch(frames, labels, train=False, **kw))
    if not a.no_host:
        rows_h = rows.numpy()

        def one(i):
            return R.pillow_image(frames_h[i], None if labels_h is None else labels_h[i], size, rows_h[i], flags)[:2]

        def batch():
            outs = list(ex.map(one, range(B)))
            x = torch.from_numpy(np.stack([o[0] for o in outs])).to(dev)
            y = None if labels_h is None else torch.from_numpy(np.stack([o[1] for o in outs])).to(dev)
            torch.cuda.synchronize()
            return x, y
        with ThreadPoolExecutor(a.host_threads) as ex:
            batch()                                        # warm-up
            times = []
            for _ in range(a.host_batches):
                t0 = time.perf_counter()
                x, y = batch()
                times.append((time.perf_counter() - t0) * 1e3)
        hi, ht = D.prepare_rgb_batch(frames, labels, params=rows, **kw)
        times.sort()
        row["host"] = {"threads": a.host_threads, "batches_timed": a.host_batches, "ms_per_batch": round(times[len(times) // 2], 2),
                       "min_ms": round(times[0], 2), "max_ms": round(times[-1], 2), "what": "Pillow calls per image + float64 YUV, stacked, uploaded",
                       "imgs_bits_equal": bool(torch.equal(x.view(torch.int32), hi.view(torch.int32))),
                       "targets_equal": None if y is None else bool(torch.equal(y, ht))}
        row["host_over_hip"] = round(row["host"]["ms_per_batch"] / row["hip_host_rows"]["ms"], 1)
    if not a.no_step and labels is not None:
        torch.manual_seed(12345678)
        model = M.PB_FCN(32, 5, 1, scale == 1, 0).to(dev)
        tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))
        x, y = D.prepare_rgb_batch(frames, labels, params=rows, scale=scale)
        row["step"] = timed(lambda: tr.step(x, y), a.min_seconds, min(a.repeats, 3), a.warmup)
        row["step"]["loss"] = tr.pop_metrics()["loss"]
    return row


def kernel_stats(path):
    """The rgb_prep kernels of a profiler's per-kernel statistics (CSV with Name, Calls, TotalDurationNs, AverageNs ... columns)."""
    out = {"kernel_trace": os.path.basename(path), "kernels": []}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "rgb_prep" in r.get("Name", ""):
                out["kernels"].append({"name": r["Name"], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                                       "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-batches", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)), flush=True)
        return
    for name in ([a.only] if a.only else list(CONFIGS)):
        print(json.dumps(run_config(name, a)), flush=True)


if __name__ == "__main__":
    main()
