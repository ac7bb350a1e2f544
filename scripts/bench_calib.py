#!/usr/bin/env python3
"""Time of one calibration pass per batch on the GPU box: the calibration tail (RCV_OP_CLS_CALIB) against the composition it replaces
and against the validation tail.

    python scripts/bench_calib.py [--only NAME] [--min-seconds 1.0] [--repeats 5] [--append FILE] [--tag TEXT]

One JSON line per shape, the paths on the same build, in one process, on one card, their windows alternating (ROBO_UNet, 5 classes,
K = 16 edges):
  calibrate    ``model.calibrate(x, state, targets)``: the eval-calib plan, RCV_OP_CLS_CALIB at its end, nothing per pixel stored
  composition  ``model.proba(x, labels=True, confidence=True)``, ``torch.bucketize`` of the confidence over the edges and ONE
               ``torch.bincount`` over (bin, class, label column): the counts only -- the confidence sums would be a second, weighted
               bincount, which the composition is not charged
  validate     ``model.validate(x, targets, state, weight)``: the yardstick -- the same tensors through a similar tail
  predict      ``model.predict(x)`` alone: what any tail has to pay for the network
Each entry: median ms per call over --repeats windows of at least --min-seconds (device events, after warm-up), spread = max - min.
``tail_ms_*`` = path - predict.  ``calibrate_tail_vs_validate_tail``: their difference against validate's own min-to-max spread.
Records alone, on random operands of the network's tail shape (fused decoder form): ``rec_calib`` (confidences spread over the bins),
``rec_calib_hot`` (a bias puts every pixel into class 0 above 0.99: all counts of a wave meet one LDS entry), ``rec_valid`` and
``rec_valid_hot`` (RCV_OP_CLS_VALID on the same operands), ``rec_maps`` / ``rec_maps_hot`` (the class-map form).  ``--tag`` names the
build in the row (A/B of two libraries: RCV_LIBRARY)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M                                       # noqa: E402
from robocupvision_amd import _lib as L                                   # noqa: E402
from robocupvision_amd.metrics import CalibrationState, ValidationState   # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {"robo_64x120x160": (64, 3, 120, 160), "robo_32x480x640": (32, 3, 480, 640)}
EDGES = tuple(round(0.5 + 0.03 * i, 4) for i in range(15)) + (0.99,)          # K = 16
WEIGHTS = (1.0, 10.0, 30.0, 10.0, 2.0)
C = 5


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


def records(N, H, W, targets, edges):
    """The tail records alone, fused decoder form (8 + 8 channels), on random operands; -> name -> call."""
    P = N * H * W
    g = torch.Generator(device=DEV).manual_seed(1)
    t, r = torch.randn(P, 8, device=DEV, generator=g), torch.randn(P, 8, device=DEV, generator=g)
    tc, rc = torch.rand(5, 8, device=DEV, generator=g) + 0.5, torch.rand(5, 8, device=DEV, generator=g) + 0.5
    w = 0.5 * torch.randn(C, 8, device=DEV, generator=g)
    bias = {"": torch.zeros(C, device=DEV), "_hot": torch.tensor([40.0, 0, 0, 0, 0], device=DEV)}
    cw = torch.tensor(WEIGHTS, device=DEV)
    h = L.handle(0)
    keep = [t, r, tc, rc, w, bias, cw]
    src = dict(n=N, h=H, w=W, cin=8, cout=C, inmode=L.CLS_LABEL_FEATURES, aux0=L.LOAD_AFFINE_RELU, aux1=8, p_in=t.data_ptr(), p_in_c=tc.data_ptr(),
               p_x3=r.data_ptr(), p_x4=rc.data_ptr(), p_w=w.data_ptr(), p_in2=targets.data_ptr())
    out = {}

    def runner(ops):
        def call():
            ops.run(h, torch.cuda.current_stream(DEV).cuda_stream)
        return call

    for tag, b in bias.items():
        state = torch.zeros(len(EDGES) + 1, C, C + 3, dtype=torch.int64, device=DEV)
        out["rec_calib" + tag] = runner(L.OpList([L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP, count=len(EDGES), p_bias=b.data_ptr(), p_x0=edges.data_ptr(),
                                                            p_x2=state.data_ptr(), **src)]))
        counts = torch.zeros(N, C, C, dtype=torch.int32, device=DEV)
        vop = L.make_op(L.OP_CLS_VALID, L.F_FUSED_UP, p_bias=b.data_ptr(), p_x0=cw.data_ptr(), p_x2=counts.data_ptr(), **src)
        rows = torch.zeros(max(L.op_workspace(h, vop), 4) // 4, device=DEV)
        vop.p[L.RCV_P_PART] = rows.data_ptr()
        out["rec_valid" + tag] = runner(L.OpList([vop]))
        lab = torch.empty(N, H, W, dtype=torch.uint8, device=DEV)
        conf = torch.empty(N, H, W, device=DEV)
        L.OpList([L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, p_bias=b.data_ptr(), p_out=lab.data_ptr(), p_x1=conf.data_ptr(),
                            **{k: v for k, v in src.items() if k != "p_in2"})]).run(h, torch.cuda.current_stream(DEV).cuda_stream)
        mstate = torch.zeros_like(state)
        out["rec_maps" + tag] = runner(L.OpList([L.make_op(L.OP_CLS_CALIB, 0, n=N, h=H, w=W, cin=1, cout=C, inmode=L.CLS_LABEL_CLASSMAP,
                                                           count=len(EDGES), p_in=lab.data_ptr(), p_x1=conf.data_ptr(), p_in2=targets.data_ptr(),
                                                           p_x0=edges.data_ptr(), p_x2=mstate.data_ptr())]))
        keep += [state, counts, rows, lab, conf, mstate]
    torch.cuda.synchronize()
    out["rec_calib"].keep = keep
    return out


def run_config(name, a):
    shape = CONFIGS[name]
    N, _, H, W = shape
    torch.manual_seed(12345678)
    model = M.ROBO_UNet().to(DEV).eval()
    x = torch.randn(*shape, device=DEV)
    targets = torch.randint(0, C, (N, H, W), device=DEV)
    targets.view(-1)[::41] = -100
    cstate, vstate = CalibrationState(C, EDGES, DEV), ValidationState(C, DEV)
    edges = cstate.edges_dev
    w = torch.tensor(WEIGHTS, device=DEV)
    cols = C + 1

    def calibrate():
        model.calibrate(x, cstate, targets)

    def composition():
        _, lab, conf = model.proba(x, labels=True, confidence=True)
        b = torch.bucketize(conf, edges, right=True)                      # the number of edges <= confidence
        col = torch.where((targets >= 0) & (targets < C), targets, torch.full_like(targets, C))
        return torch.bincount(((b * C + lab.long()) * cols + col).view(-1), minlength=(len(EDGES) + 1) * C * cols)

    def validate():
        model.validate(x, targets, vstate, weight=w)

    def predict():
        return model.predict(x)

    cstate.reset()
    calibrate()
    counts = composition().view(len(EDGES) + 1, C, cols)
    row = {"config": name, "shape": list(shape), "edges": len(EDGES), "tag": a.tag, "library": os.path.basename(L.LIB_PATH),
           "counts_equal_composition": bool(torch.equal(cstate.buf[:, :, :cols], counts)),
           "bins_filled": int((cstate.buf[:, :, :cols].sum((1, 2)) > 0).sum())}
    fns = {"calibrate": calibrate, "composition": composition, "validate": validate, "predict": predict}
    fns.update(records(N, H, W, targets, edges))
    row.update(timed_alternating(fns, a.min_seconds, a.repeats))
    ratio = row["calibrate"]["ms"] / row["composition"]["ms"]
    row["calibrate_over_composition"] = {"ratio": round(ratio, 4), "faster": bool(ratio < 1.0)}
    for k in ("calibrate", "composition", "validate"):
        row["tail_ms_" + k] = round(row[k]["ms"] - row["predict"]["ms"], 5)
    gap = row["tail_ms_calibrate"] - row["tail_ms_validate"]
    row["calibrate_tail_vs_validate_tail"] = {"gap_ms": round(gap, 5), "validate_spread_ms": row["validate"]["spread_ms"],
                                              "slower_beyond_spread": bool(gap > row["validate"]["spread_ms"])}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--append", default=None, help="also append the lines to this file")
    ap.add_argument("--tag", default="plain", help="names the build in the row")
    a = ap.parse_args()
    for name in ([a.only] if a.only else list(CONFIGS)):
        line = json.dumps(run_config(name, a))
        print(line, flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
