#!/usr/bin/env python3
"""Time of ``prepare_batch`` (RCV_OP_BATCH_PREP: the loader's resize / normalise / flip / jitter / maskLabel of dataset.py:107-133 for a
whole batch in one launch) on the GPU box, against what it replaces.

    python scripts/bench_batch_prep.py [--only NAME] [--min-seconds 0.5] [--repeats 5] [--no-host] [--no-step]

One JSON line per configuration:
  hip          median ms of ``prepare_batch`` in training mode over the repeats (each a window of at least --min-seconds timed with
               device events after warm-up), the spread (max - min), and the share of the 8 TB/s HBM peak the bytes below reach
  bytes        what the launch must move, from the shapes: every frame byte in, the gathered label elements in, the fp32 NCHW batch and
               the int64 targets out; and the time that takes at 8 TB/s
  torch_eager  (the configuration without a resize only) the same arithmetic in stock eager PyTorch on the same card in the same run:
               uint8 -> float, div(255), normalise, flip by torch.where, (y + b) * c, the 2x2 einsum, maskLabel's sequential rule.
               Eager torch cannot resize as Pillow does, so the twin has no resize and is the yardstick of that configuration alone:
               ``beats_twin`` = the launch is faster than the twin by more than the twin's own spread
  host         the pipeline the reference runs per image on the host (the NumPy restatement of tests/batch_prep_restatement.py, which
               is what Pillow + torch compute there), on --host-threads threads (default 16) over --host-images images: ms per batch
  step         for context, ms of ``Trainer.step`` of a ROBO_UNet on the prepared batch, same run
The parent of this feature cannot run the path at all."""
import argparse
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
from robocupvision_amd.train import Trainer          # noqa: E402
import batch_prep_restatement as R                   # noqa: E402

# name -> (B, (Hs, Ws), (H, W))
CONFIGS = {"b64_480x640_to_120x160": (64, (480, 640), (120, 160)), "b32_480x640_to_240x320": (32, (480, 640), (240, 320)),
           "b32_480x640_identity": (32, (480, 640), (480, 640))}
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


def eager_twin(frames, labels, rows, finetune, flags):
    """The arithmetic of the kernel without the resize, in eager torch ops on the device."""
    dev = frames.device
    mean = torch.tensor(D.MEAN[finetune], device=dev).view(1, 3, 1, 1)
    std = torch.tensor(D.STD[finetune], device=dev).view(1, 3, 1, 1)
    flip = (rows[:, 0] != 0).view(-1, 1, 1, 1)
    b, c = rows[:, 1].view(-1, 1, 1), rows[:, 2].view(-1, 1, 1)
    mtx = rows[:, 3:7].reshape(-1, 2, 2)

    def fn():
        x = frames.permute(0, 3, 1, 2).to(torch.float32).div(255)
        x = (x - mean) / std
        x = torch.where(flip, x.flip(3), x)
        y = (x[:, 0] + b) * c
        uv = torch.einsum("bnm,bmhw->bnhw", mtx, x[:, 1:])
        imgs = torch.cat([y[:, None], uv], 1)
        t = labels.long()
        t = torch.where(flip[:, 0], t.flip(2), t)
        rN, gN, lN = 2, 3, 4          # transform.py:26-49
        if flags[0]:
            t[t == 1] = 0
            t[t > 1] -= 1
            rN, gN, lN = 1, 2, 3
        if flags[1]:
            t[t == rN] = 0
            t[t > rN] -= 1
            gN, lN = 1, 2
        if flags[2]:
            t[t == gN] = 0
            t[t > gN] -= 1
            lN = 1
        if flags[3]:
            t[t == lN] = 0
        return imgs, t
    return fn


def run_config(name, a):
    B, src, size = CONFIGS[name]
    dev = torch.device("cuda:0")
    frames_h, labels_h = R.synthetic_frames(min(B, 4), src[0], src[1], 31)
    reps = (B + len(frames_h) - 1) // len(frames_h)
    frames_h, labels_h = np.concatenate([frames_h] * reps)[:B], np.concatenate([labels_h] * reps)[:B]
    frames, labels = torch.from_numpy(frames_h).to(dev), torch.from_numpy(labels_h).to(dev)
    random.seed(32)
    torch.manual_seed(32)
    rows = D.draw_jitter(B).to(dev)
    flags = (False, False, True, False)
    kw = dict(no_ball=flags[0], no_robot=flags[1], no_goal=flags[2], no_line=flags[3])
    row = {"config": name, "B": B, "src": list(src), "size": list(size)}
    nbytes = B * (src[0] * src[1] * 3 + size[0] * size[1] * (labels.element_size() + 3 * 4 + 8))
    row["bytes"] = {"MB": round(nbytes / 1e6, 3), "us_at_8TBps_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 3)}
    row["hip"] = timed(lambda: D.prepare_batch(frames, labels, size, params=rows, **kw), a.min_seconds, a.repeats, a.warmup)
    row["hip"]["TBps"] = round(nbytes / (row["hip"]["ms"] * 1e-3) / 1e12, 3)
    row["hip"]["share_of_8TBps_hbm_peak"] = round(nbytes / (row["hip"]["ms"] * 1e-3) / HBM_PEAK, 4)
    if src == size:
        twin = eager_twin(frames, labels, rows, False, flags)
        ti, tt = twin()
        hi, ht = D.prepare_batch(frames, labels, size, params=rows, **kw)
        row["torch_eager"] = timed(twin, a.min_seconds, a.repeats, a.warmup)
        row["torch_eager"]["targets_equal"] = bool(torch.equal(tt, ht))
        row["torch_eager"]["max_abs_diff"] = float((ti - hi).abs().max())
        row["hip_over_twin"] = round(row["hip"]["ms"] / row["torch_eager"]["ms"], 4)
        row["beats_twin"] = bool(row["torch_eager"]["ms"] - row["hip"]["ms"] > row["torch_eager"]["spread_ms"])
    if not a.no_host:
        n = min(B, a.host_images)
        rows_h = rows.cpu().numpy()

        def one(i):
            return R.prepare_image(frames_h[i], labels_h[i], size, False, True, rows_h[i], flags)
        with ThreadPoolExecutor(a.host_threads) as ex:
            list(ex.map(one, range(min(n, a.host_threads))))          # warm-up
            t0 = time.perf_counter()
            list(ex.map(one, range(n)))
            dt = time.perf_counter() - t0
        row["host"] = {"threads": a.host_threads, "images_timed": n, "ms_per_batch": round(dt / n * B * 1e3, 2), "what": "NumPy restatement per image"}
    if not a.no_step:
        torch.manual_seed(12345678)
        tr = Trainer(M.ROBO_UNet().to(dev))
        x, t = D.prepare_batch(frames, labels, size, params=rows)
        row["step"] = timed(lambda: tr.step(x, t), a.min_seconds, min(a.repeats, 3), a.warmup)
        row["step"]["loss"] = tr.pop_metrics()["loss"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-images", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    for name in ([a.only] if a.only else list(CONFIGS)):
        print(json.dumps(run_config(name, a)), flush=True)


if __name__ == "__main__":
    main()
