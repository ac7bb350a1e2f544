#!/usr/bin/env python
"""Device time of object_patches (RCV_OP_OBJECT_PATCHES, csrc/patches.hip) on N = 32 frames of 480 x 640 with the DBCONVERT boxes of
120 x 160 class maps: HIP events (the helper of scripts/bench_objects.py), warmed up, median of --iters.  Per case one JSON line,
appended to --out:

  blob       the boxes find_objects(**DBCONVERT) gives for seeded blob maps (balls, robots, goal posts of ordinary size)
  fullframe  the same, with the first robot of every image replaced by a box that fills the frame: the most expensive slot there is
             next to the cheapest ones (the load imbalance of DESIGN §4.12)

Timed, one after the other in the same loop: the launch alone (float images only, and with the bytes); the chain find_objects +
object_patches; Segmenter(objects=DBCONVERT) with and without patches={} (a seeded ROBO_UNet, its own maps).  Next to them the host
alternative a user had before: Objects.to_list() (a host copy and a synchronisation), Pillow resize(box=) of every box, the numpy
YUV step, one upload -- host clock around a device synchronise, --host-iters times.  Bytes: the source pixels under the valid boxes
(3 bytes each, every one read at least once) plus the outputs written, over the launch's median time.

    python scripts/bench_patches.py [--iters 30] [--warmup 5] [--cases blob,fullframe] [--no-host]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import objdet_restatement as R  # noqa: E402
import patches_restatement as PR  # noqa: E402
from bench_objects import timed  # noqa: E402
from robocupvision_amd import _lib as L  # noqa: E402
from robocupvision_amd import infer as I  # noqa: E402
from robocupvision_amd import patches as P  # noqa: E402

DEV = "cuda:0"
N, HS, WS, H, W = 32, 480, 640, 120, 160
SIZE = (32, 32)


def host_alternative(frames_host, objs):
    """What a user did without the op: boxes to the host, Pillow crop + resize, numpy YUV, upload.  Returns the uploaded batch."""
    from PIL import Image
    out = []
    for n, found in enumerate(objs.to_list()):
        im = Image.fromarray(frames_host[n])
        for (_, x, y, w, h, _) in found:
            box = (x * WS / W, y * HS / H, (x + w) * WS / W, (y + h) * HS / H)
            out.append(PR.to_yuv(np.asarray(im.resize((SIZE[1], SIZE[0]), Image.BILINEAR, box=box))))
    batch = torch.from_numpy(np.stack(out)).to(DEV) if out else torch.empty(0, 3, *SIZE, device=DEV)
    torch.cuda.synchronize()
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--cases", default="blob,fullframe")
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patches.py needs the GPU: there is nothing to time without one")
    import robocupvision_amd.model as Mo
    h = L.handle(0)
    frames_host = PR.seeded_frames(1, N, HS, WS)
    frames = torch.from_numpy(frames_host).to(DEV)
    maps = torch.from_numpy(R.blob_masks(np.random.default_rng(7), N, H, W, 5, 15)).to(torch.uint8).to(DEV)
    torch.manual_seed(1)
    net = Mo.ROBO_UNet().to(DEV)
    seg_plain = I.Segmenter(net, img_size=(H, W), objects=I.DBCONVERT)
    seg_patch = I.Segmenter(net, img_size=(H, W), objects=I.DBCONVERT, patches={})
    for name in a.cases.split(","):
        objs = I.find_objects(maps, **I.DBCONVERT)
        if name == "fullframe":
            rows = objs.rows.clone()
            rows[:, 1, 0, 0:4] = torch.tensor([0, 0, W, H], dtype=torch.int32, device=DEV)
            counts = objs.counts.clone()
            counts[:, 1, 3] = counts[:, 1, 3].clamp(min=1)
            objs = I.Objects(rows, counts)
        elif name != "blob":
            raise SystemExit("unknown case %r (blob, fullframe)" % name)
        calls = {"launch": lambda: P.object_patches(frames, objs, map_size=(H, W)),
                 "launch_bytes": lambda: P.object_patches(frames, objs, map_size=(H, W), return_bytes=True),
                 "find_and_cut": lambda: P.object_patches(frames, I.find_objects(maps, **I.DBCONVERT), map_size=(H, W)),
                 "segmenter": lambda: seg_plain(frames), "segmenter_patches": lambda: seg_patch(frames)}
        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(a.iters):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        rec = P.PatchesRecord(N, HS, WS, 4, objs.rows.shape[2], (H, W), SIZE, 0)
        res = {"case": name, "N": N, "Hs": HS, "Ws": WS, "H": H, "W": W, "size": list(SIZE), "rules": "DBCONVERT", "iters": a.iters,
               "label": L.OpList([rec.op]).labels(h)[0], "slots": int(objs.rows.shape[0] * objs.rows.shape[1] * objs.rows.shape[2])}
        for k, v in times.items():
            res[k + "_ms_median"] = round(statistics.median(v), 4)
            res[k + "_ms_min"] = round(min(v), 4)
        p = P.object_patches(frames, objs, map_size=(H, W), return_bytes=True)
        valid = p.valid.cpu().numpy()
        rows_h = objs.rows.cpu().numpy()
        res["valid"] = int(valid.sum())
        src = [int(r[2]) * (WS // W) * int(r[3]) * (HS // H) * 3 for r in rows_h[valid]]
        res["source_bytes"] = int(sum(src))
        res["largest_slot_source_bytes"], res["smallest_slot_source_bytes"] = (int(max(src)), int(min(src))) if src else (0, 0)
        res["written_bytes"] = int(p.images.numel() * 4)
        res["launch_GBps"] = round((res["source_bytes"] + res["written_bytes"]) / (res["launch_ms_median"] * 1e-3) / 1e9, 2)
        res["segmenter_valid"] = int(seg_patch(frames)[3].valid.sum())
        if not a.no_host:
            ts = []
            for _ in range(a.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch = host_alternative(frames_host, objs)
                ts.append((time.perf_counter() - t0) * 1e3)
            res["host_ms_median"] = round(statistics.median(ts), 2)
            flat = valid.reshape(-1)
            res["host_equal"] = bool(torch.equal(batch.cpu(), p.images.cpu()[torch.from_numpy(flat)]))
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
