#!/usr/bin/env python3
"""Time of class probabilities per batch on the GPU box: the softmax tail (RCV_OP_CLS_PROBA) against the composition it replaces.

    python scripts/bench_proba.py [--only NAME] [--min-seconds 1.0] [--repeats 5] [--append FILE]

One JSON line per shape, the three paths on the same build, in one process, on one card, their windows alternating:
  proba        ``model.proba(x, labels=True, confidence=True)``: the eval-proba plan, RCV_OP_CLS_PROBA at its end, no logits
  composition  ``z = model(x); p = torch.softmax(z, 1); conf, cls = p.max(1)``: the eval plan, then two torch passes over the logits
  predict      ``model.predict(x)`` alone: the eval-labels plan, what any tail has to pay for the network
Each entry: median ms per call over --repeats windows of at least --min-seconds (device events, after warm-up), spread = max - min.
``proba_over_composition`` < 1 means the tail is faster; ``beyond_box_spread`` says whether the gap exceeds the +-1.5 % box spread of
DESIGN.md section 9.  ``tail``: the RCV_OP_CLS_PROBA record alone on random operands of the network's tail shape (the fused decoder
form), its algorithmic bytes -- the features and the skip tensor read once, probabilities, class bytes and confidences written once --
and the bytes per second they give."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd import _lib as L              # noqa: E402

DEV = torch.device("cuda:0")
# name -> (constructor, input shape, (classifier input channels, skip channels))
CONFIGS = {"robo_64x120x160": (lambda: M.ROBO_UNet(), (64, 3, 120, 160), (8, 8)),
           "robo_32x480x640": (lambda: M.ROBO_UNet(), (32, 3, 480, 640), (8, 8)),
           "labelprop_64x120x160": (lambda: M.LabelProp(5, 32, 0.0), (64, 8, 120, 160), (16, 8))}
BOX_SPREAD = 0.015


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def timed_alternating(fns, min_seconds, repeats, warmup=3):
    """fns: name -> call.  Windows of the paths alternate, so drift of the box meets all of them alike."""
    n = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        n[name] = max(2, int(min_seconds * 1e3 / max(window(fn, 1), 1e-3)) + 1)
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            out[name].append(window(fn, n[name]))
    res = {}
    for name, v in out.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 5), "spread_ms": round(v[-1] - v[0], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5),
                     "calls_per_window": n[name], "repeats": repeats}
    return res


def tail_record(N, H, W, cin, rch):
    """The record alone, fused decoder form, on random operands; -> (call, algorithmic bytes)."""
    P = N * H * W
    g = torch.Generator(device=DEV).manual_seed(1)
    t, r = torch.randn(P, cin, device=DEV, generator=g), torch.randn(P, rch, device=DEV, generator=g)
    tc, rc = torch.rand(5, cin, device=DEV, generator=g) + 0.5, torch.rand(5, rch, device=DEV, generator=g) + 0.5
    w, b = 0.5 * torch.randn(5, cin, device=DEV, generator=g), torch.zeros(5, device=DEV)
    prob = torch.empty(N, 5, H, W, device=DEV)
    lab = torch.empty(N, H, W, dtype=torch.uint8, device=DEV)
    conf = torch.empty(N, H, W, device=DEV)
    ops = L.OpList([L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, n=N, h=H, w=W, cin=cin, cout=5, inmode=L.CLS_LABEL_FEATURES,
                              aux0=L.LOAD_AFFINE_RELU, aux1=rch, p_in=t.data_ptr(), p_in_c=tc.data_ptr(), p_x3=r.data_ptr(), p_x4=rc.data_ptr(),
                              p_w=w.data_ptr(), p_bias=b.data_ptr(), p_x0=prob.data_ptr(), p_out=lab.data_ptr(), p_x1=conf.data_ptr())])
    h = L.handle(0)
    keep = (t, r, tc, rc, w, b, prob, lab, conf)

    def call():
        ops.run(h, torch.cuda.current_stream(DEV).cuda_stream)
    call.keep = keep
    return call, P * (4 * cin + 4 * rch + 4 * 5 + 1 + 4)


def run_config(name, a):
    make, shape, (cin, rch) = CONFIGS[name]
    torch.manual_seed(12345678)
    model = make().to(DEV).eval()
    x = torch.randn(*shape, device=DEV)

    def proba():
        return model.proba(x, labels=True, confidence=True)

    def composition():
        with torch.no_grad():
            z = model(x)
            p = torch.softmax(z, 1)
            conf, cls = p.max(1)
        return p, cls, conf

    def predict():
        return model.predict(x)

    p, lab, conf = proba()
    p2, cls2, conf2 = composition()
    row = {"config": name, "shape": list(shape),
           "max_abs_gap_to_torch_softmax": float((p - p2).abs().max()), "classes_equal": bool(torch.equal(lab.long(), cls2))}
    tail, nbytes = tail_record(shape[0], shape[2], shape[3], cin, rch)
    row.update(timed_alternating({"proba": proba, "composition": composition, "predict": predict, "tail": tail}, a.min_seconds, a.repeats))
    ratio = row["proba"]["ms"] / row["composition"]["ms"]
    row["proba_over_composition"] = {"ratio": round(ratio, 4), "beyond_box_spread": bool(abs(ratio - 1.0) > BOX_SPREAD),
                                     "not_slower": bool(ratio <= 1.0 + BOX_SPREAD)}
    row["tail_ms_proba"] = round(row["proba"]["ms"] - row["predict"]["ms"], 5)
    row["tail_ms_composition"] = round(row["composition"]["ms"] - row["predict"]["ms"], 5)
    row["tail"]["algorithmic_bytes"] = nbytes
    row["tail"]["gb_per_s"] = round(nbytes / (row["tail"]["ms"] * 1e-3) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
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
