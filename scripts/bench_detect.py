#!/usr/bin/env python3
"""Time of the detect.py path (detect.py:125-138: frames -> network -> class map -> colour mask) on the GPU box.

    python scripts/bench_detect.py [--only NAME] [--min-seconds 1.0] [--repeats 3] [--no-tail]
    python scripts/bench_detect.py --profile-child          # only the tail kernels, a fixed number of launches (for a kernel trace)

One JSON line per configuration, all paths on the same build, in the same process, on one card:
  composition  (a) what a caller could do before ``predict`` existed: ``model(x)``, ``torch.max(pred, 1)``, ``palette[idx]``
  predict      (b) ``model.predict(x, colour=True)``: the eval-labels plan, RCV_OP_CLS_LABEL at its end, no logits
  segmenter    (b) from decoded uint8 frames: ``Segmenter(model)(frames)`` = RCV_OP_FRAME_PREP + the above (ROBO-UNet configurations)
  frames_composition  (a) from frames: ``prepare_batch(train=False)`` with a zero label tensor, then the composition
Each entry: median ms over --repeats windows of at least --min-seconds (device events, after warm-up), spread = max - min.
``predict_over_composition`` < 1 means the new path is faster; ``beyond_spread`` says whether the gap exceeds both spreads.

Tail lines ("tail": ...): the RCV_OP_CLS_LABEL record alone on random operands, both store shapes (1 = bytes per pixel and lane,
4 = dwords of four pixels), with the bytes it must move and the share of the 8 TB/s HBM peak it reaches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robocupvision_amd                              # noqa: E402
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd import _lib as L              # noqa: E402
from robocupvision_amd import data as D              # noqa: E402
from robocupvision_amd import palette as P           # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8e12
# name -> (network, batch, (H, W), source frame size or None)
CONFIGS = {"robo_1x120x160": ("robo", 1, (120, 160), (480, 640)), "robo_64x120x160": ("robo", 64, (120, 160), (480, 640)),
           "robo_32x480x640": ("robo", 32, (480, 640), (480, 640)), "labelprop_16x120x160": ("labelprop", 16, (120, 160), None)}
# name -> (pixels N, H, W; CIN; fused skip channels (0 = plain); source form)
TAILS = {"c8_fused_32x480x640": (32, 480, 640, 8, 8, 0), "c8_fused_64x120x160": (64, 120, 160, 8, 8, 0), "c16_fused8_16x120x160": (16, 120, 160, 16, 8, 0),
         "c16_fused8_32x480x640": (32, 480, 640, 16, 8, 0), "logits8_32x480x640": (32, 480, 640, 8, 0, 1), "classmap_u8_32x480x640": (32, 480, 640, 1, 0, 2)}


def timed(fn, min_seconds, repeats, warmup=10):
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


def compare(a, b):
    return {"ratio": round(b["ms"] / a["ms"], 4), "beyond_spread": bool(abs(a["ms"] - b["ms"]) > a["spread_ms"] + b["spread_ms"])}


def run_config(name, a):
    net, B, size, src = CONFIGS[name]
    torch.manual_seed(12345678)
    if net == "robo":
        model = M.ROBO_UNet().to(DEV).eval()
        x = torch.randn(B, 3, size[0], size[1], device=DEV)
    else:
        model = M.LabelProp(5, 32).to(DEV).eval()
        x = torch.randn(B, size[0], size[1], 8, device=DEV).permute(0, 3, 1, 2)          # NHWC memory, as labelprop_batch hands it over
    pal = P.device_palette(None, DEV)

    def composition(inp):
        idx = torch.max(model(inp), 1)[1]
        return idx, pal[idx]

    with torch.no_grad():
        idx, col = composition(x)
        lab, col2 = model.predict(x, colour=True)
        row = {"config": name, "network": net, "B": B, "size": list(size), "labels_equal": bool(torch.equal(lab, idx.to(torch.uint8))),
               "colour_equal": bool(torch.equal(col, col2))}
        row["composition"] = timed(lambda: composition(x), a.min_seconds, a.repeats)
        row["predict"] = timed(lambda: model.predict(x, colour=True), a.min_seconds, a.repeats)
        row["predict_over_composition"] = compare(row["composition"], row["predict"])
        if src is not None:
            frames = torch.randint(0, 256, (B, src[0], src[1], 3), dtype=torch.uint8, device=DEV)
            zero = torch.zeros(B, src[0], src[1], dtype=torch.uint8, device=DEV)
            seg = robocupvision_amd.Segmenter(model, img_size=size)
            row["src"] = list(src)
            row["frames_composition"] = timed(lambda: composition(D.prepare_batch(frames, zero, size, train=False)[0]), a.min_seconds, a.repeats)
            row["segmenter"] = timed(lambda: seg(frames), a.min_seconds, a.repeats)
            row["segmenter_over_frames_composition"] = compare(row["frames_composition"], row["segmenter"])
    return row


def tail_record(name, store):
    N, H, W, cin, rch, form = TAILS[name]
    n = N * H * W
    g = torch.Generator(device=DEV).manual_seed(7)
    keep = {"lab": torch.empty(n, dtype=torch.uint8, device=DEV), "col": torch.empty(n, 3, dtype=torch.uint8, device=DEV),
            "pal": P.device_palette(None, DEV)}
    kw = dict(n=N, h=H, w=W, cin=cin, cout=5 if form != 2 else 8, inmode=form, count=store, p_x0=keep["col"].data_ptr(), p_x1=keep["pal"].data_ptr())
    flags = 0
    if form == 2:
        keep["x"] = torch.randint(0, 5, (n,), dtype=torch.uint8, device=DEV, generator=g)
        kw.update(inmode2=1, p_in=keep["x"].data_ptr())
        nbytes = n * (1 + 3)
    else:
        keep["x"] = torch.randn(n, cin, device=DEV, generator=g)
        keep["b"] = torch.randn(5, device=DEV, generator=g)
        kw.update(p_in=keep["x"].data_ptr(), p_bias=keep["b"].data_ptr(), p_out=keep["lab"].data_ptr())
        nbytes = n * (4 * cin + 4)
        if form == 0:
            keep["w"] = torch.randn(5, cin, device=DEV, generator=g)
            kw["p_w"] = keep["w"].data_ptr()
        if rch:
            flags = L.F_FUSED_UP
            keep["tc"], keep["rc"] = torch.rand(5, cin, device=DEV, generator=g) + 0.5, torch.rand(5, rch, device=DEV, generator=g) + 0.5
            keep["r"] = torch.randn(n, rch, device=DEV, generator=g)
            kw.update(aux0=L.LOAD_AFFINE, aux1=rch, p_in_c=keep["tc"].data_ptr(), p_x3=keep["r"].data_ptr(), p_x4=keep["rc"].data_ptr())
            nbytes += n * 4 * rch
    return L.OpList([L.make_op(L.OP_CLS_LABEL, flags, **kw)]), keep, nbytes


def run_tail(name, a):
    h, stream = L.handle(0), torch.cuda.current_stream(DEV).cuda_stream
    row = {"tail": name}
    for store in (1, 4):
        ops, keep, nbytes = tail_record(name, store)
        t = timed(lambda: ops.run(h, stream), a.min_seconds, a.repeats)
        t["TBps"] = round(nbytes / (t["ms"] * 1e-3) / 1e12, 3)
        t["share_of_8TBps_hbm_peak"] = round(nbytes / (t["ms"] * 1e-3) / HBM_PEAK, 4)
        row["store_%d" % store] = t
        row["bytes_per_pixel"] = nbytes // (TAILS[name][0] * TAILS[name][1] * TAILS[name][2])
    row["store4_over_store1"] = compare(row["store_1"], row["store_4"])
    return row


def profile_child():
    """The tail kernels alone, 50 launches each (run this under a kernel trace; nothing is timed here)."""
    h, stream = L.handle(0), torch.cuda.current_stream(DEV).cuda_stream
    for name in TAILS:
        for store in (1, 4):
            ops, keep, nbytes = tail_record(name, store)
            for _ in range(50):
                ops.run(h, stream)
            torch.cuda.synchronize()
            print(json.dumps({"tail": name, "store": store, "bytes": nbytes, "launches": 50}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-tail", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    for name in ([a.only] if a.only else list(CONFIGS)):
        print(json.dumps(run_config(name, a)), flush=True)
    if not a.no_tail and not a.only:
        for name in TAILS:
            print(json.dumps(run_tail(name, a)), flush=True)


if __name__ == "__main__":
    main()
