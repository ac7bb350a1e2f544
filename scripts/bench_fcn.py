#!/usr/bin/env python3
"""FCN, the pointwise (1x1) convolution family and the separable blocks on the GPU box.  Measures; asserts nothing.

    python scripts/bench_fcn.py [--reps 50] [--rounds 5] [--steps 20] [--warmup 5] [--out profiles/fcn_bench.jsonl]

1. Each pointwise record (csrc/conv_pw.hip) against the same product run as a centre-tap 3x3 record -- the path that exists without
   the family: a [Cout][Cin][3][3] filter whose centre tap holds the 1x1 filter, packed in the layout rcv_op_filter_layout asks for,
   run by whatever family the planner picks.  At N x H x W = 64 x 60 x 80 for the channel pairs of tests/test_gpu_pw.py, three kinds:
   the training forward (RCV_LOAD_AFFINE_RELU, RCV_STATS_FWD), the data gradient (RCV_LOAD_GRAD_DEC, RCV_STATS_BWD_DEC) and the filter
   gradient with its reduction.  Both sides are timed interleaved inside one call: device-event time over `reps` back-to-back
   launches, the median of `rounds` windows taken alternately.
2. The FCN training step (Trainer, fused optim.SGD) and `predict` at 64 x 3 x 120 x 160 against stock PyTorch on the same card: the
   same network written with torch.nn.functional calls over the module's own parameters, torch.optim.SGD, F.cross_entropy.
3. The share of a ConvSep / trConvSep training step (forward + backward of the block) spent in the cross-filter 3x3 records, from
   per-record event times (Engine.profile_last), and what a dedicated 1-D family could save at most: those records do 3x (ConvSep)
   and 1.8x (trConvSep) the necessary multiplications.
One JSON line per figure, printed and appended to --out."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M        # noqa: E402
from robocupvision_amd import _lib as L    # noqa: E402
from robocupvision_amd.optim import SGD    # noqa: E402
from robocupvision_amd.train import Trainer    # noqa: E402

DEV = torch.device("cuda:0")
PAIRS = [(8, 8), (16, 8), (16, 16), (32, 16), (128, 64), (128, 128)]
PW_N, PW_H, PW_W = 64, 60, 80
PB_W = [1, 6, 1.5, 3, 3]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(cands, reps, rounds):
    """name -> list of window times; the candidates alternate inside every round (drift of the shared box hits all alike)."""
    for fn in cands.values():
        window(fn, 5)
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(window(fn, reps))
    return times


def _round_up(a, b):
    return (a + b - 1) // b * b


def pack3(h, stream, w, D0, D1, rows_from_d1, flip, layout, keep):
    """engine._Lowering.add_pack for one filter: the packed tensor in the layout the library asked for.  The padding rules are that
    method's, restated because it needs a plan to allocate into; a note there points back here."""
    rows, cols = (D1, D0) if rows_from_d1 else (D0, D1)
    split = layout in (3, 4, 5)
    rp = _round_up(rows, (16 if layout == 5 else (32 if rows > 32 else 8)) if split else 4)
    cp = _round_up(cols, 16)
    taps = 16 if layout == 2 else 9
    ksteps = (rp // 16) * 5 if layout == 5 else (taps * rp + 31) // 32
    dst = torch.zeros(3 * ksteps * cp * 16 if split else taps * rp * cp, device=DEV)
    job = L.RcvPackJob()
    job.src, job.dst, job.D0, job.D1 = w.data_ptr(), dst.data_ptr(), D0, D1
    job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = int(rows_from_d1), int(flip), rp, cp, layout
    table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
    L.OpList([L.make_op(L.OP_PACK, 0, count=1, aux0=16 * rp * cp, p_in=table.data_ptr())]).run(h, stream)
    torch.cuda.synchronize()
    keep += [dst, table]
    return dst


def pointwise_candidates(cin, cout, wgrad_cap=0):
    """name -> callable; labels; for the three record kinds in their pointwise and their centre-tap 3x3 form."""
    h = L.handle(0)
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(100 * cin + cout)
    N, H, W = PW_N, PW_H, PW_W
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    x, c_in, y, dy = rnd(N, H, W, cin), rnd(5, cin) * 0.5, rnd(N, H, W, cout), rnd(N, H, W, cout)
    c_out, e_in, ec_in = rnd(5, cout) * 0.5, rnd(N, H, W, cin), rnd(3, cin) * 0.5
    w1 = (rnd(cout, cin, 1, 1) * 0.1).contiguous()
    w3 = torch.zeros(cout, cin, 3, 3, device=DEV)
    w3[:, :, 1, 1] = w1[:, :, 0, 0]
    out_f, out_d = torch.empty(N, H, W, cout, device=DEV), torch.empty(N, H, W, cin, device=DEV)
    dw1, dw3 = torch.empty_like(w1), torch.empty_like(w3)
    keep = [x, c_in, y, dy, c_out, e_in, ec_in, w1, w3, out_f, out_d, dw1, dw3]
    cands, labels = {}, {}

    def ws(op):
        nbytes = L.op_workspace(h, op)
        if nbytes:
            t = torch.empty(nbytes // 4, device=DEV)
            keep.append(t)
            op.p[L.RCV_P_PART] = t.data_ptr()
        return op

    def add(name, ops):
        lst = L.OpList(ops)
        labels[name] = lst.labels(h)
        cands[name] = lambda: lst.run(h, stream)

    dims = dict(n=N, h=H, w=W, ho=H, wo=W, stride=1, dil=1)
    # ---- training forward: relu(bn(.)) of the producer on load, BatchNorm sums of the output
    fwd = dict(cin=cin, cout=cout, inmode=L.LOAD_AFFINE_RELU, stats=L.STATS_FWD, p_in=x.data_ptr(), p_in_c=c_in.data_ptr(), p_out=out_f.data_ptr())
    add("fwd/pw", [ws(L.make_op(L.OP_PW, 0, p_w=w1.data_ptr(), **fwd, **dims))])
    op3 = L.make_op(L.OP_CONV, 0, **fwd, **dims)
    lay = L.op_filter_layout(h, op3, False)
    if lay:
        op3.i[L.RCV_I_AUX0] = lay
    op3.p[L.RCV_P_W] = pack3(h, stream, w3, cout, cin, True, False, lay, keep).data_ptr()
    add("fwd/conv3x3", [ws(op3)])
    # ---- data gradient: ReLU and BatchNorm backward of this layer on load, the producer's BatchNorm-backward sums
    dg = dict(cin=cout, cout=cin, inmode=L.LOAD_GRAD_DEC, stats=L.STATS_BWD_DEC, p_in=dy.data_ptr(), p_in_aux=y.data_ptr(), p_in_c=c_out.data_ptr(),
              p_epi_aux=e_in.data_ptr(), p_epi_c=ec_in.data_ptr(), p_out=out_d.data_ptr())
    add("dgrad/pw", [ws(L.make_op(L.OP_PW, L.F_TRANSPOSED_SRC, p_w=w1.data_ptr(), **dg, **dims))])
    od3 = L.make_op(L.OP_CONV, 0, **dg, **dims)
    lay = L.op_filter_layout(h, od3, False)
    if lay:
        od3.i[L.RCV_I_AUX0] = lay
    od3.p[L.RCV_P_W] = pack3(h, stream, w3, cout, cin, False, True, lay, keep).data_ptr()
    add("dgrad/conv3x3", [ws(od3)])
    # ---- filter gradient and its reduction
    wg = dict(cin=cin, cout=cout, inmode=L.LOAD_AFFINE_RELU, inmode2=L.LOAD_GRAD_DEC, p_in=x.data_ptr(), p_in_c=c_in.data_ptr(), p_in2=dy.data_ptr(),
              p_in2_aux=y.data_ptr(), p_in2_c=c_out.data_ptr())
    wp = ws(L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, aux0=wgrad_cap, **wg))
    add("wgrad/pw", [wp, L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=wp.i[L.RCV_I_NSPLIT], p_part=wp.p[L.RCV_P_PART],
                                   p_out=dw1.data_ptr())])
    w3op = ws(L.make_op(L.OP_WGRAD, 0, **wg, **dims))
    add("wgrad/conv3x3", [w3op, L.make_op(L.OP_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=w3op.i[L.RCV_I_NSPLIT], p_part=w3op.p[L.RCV_P_PART],
                                          p_out=dw3.data_ptr())])
    return cands, labels, keep


def bench_pointwise(reps, rounds, emit, wgrad_cap=0):
    px = PW_N * PW_H * PW_W
    for cin, cout in PAIRS:
        cands, labels, _keep = pointwise_candidates(cin, cout, wgrad_cap)
        times = interleaved(cands, reps, rounds)
        for kind in ("fwd", "dgrad", "wgrad"):
            a, b = times[kind + "/pw"], times[kind + "/conv3x3"]
            ma, mb = statistics.median(a), statistics.median(b)
            emit({"what": "pointwise_vs_centre_tap", "kind": kind, "cin": cin, "cout": cout, "N": PW_N, "H": PW_H, "W": PW_W,
                  "pw_ms": round(ma, 5), "pw_ms_min_max": [round(min(a), 5), round(max(a), 5)], "pw_labels": labels[kind + "/pw"],
                  "conv3x3_ms": round(mb, 5), "conv3x3_ms_min_max": [round(min(b), 5), round(max(b), 5)], "conv3x3_labels": labels[kind + "/conv3x3"],
                  "pw_over_conv3x3": round(ma / mb, 4), "reps": reps, "rounds": rounds, "wgrad_cap": wgrad_cap,
                  "pw_useful_gflops": round(2.0 * cin * cout * px / ma / 1e6, 1),
                  "pw_gbytes_per_s": round(4.0 * px * ((cin + cout) * (2 if kind == "dgrad" else 1) + (cout if kind == "wgrad" else 0)) / ma / 1e6, 1)})


def torch_fcn(p, x, training, buffers):
    """FCN's forward in stock torch calls over the parameter dict ``p`` (state_dict names)."""
    def bn(t, pre):
        return F.batch_norm(t, buffers[pre + ".running_mean"], buffers[pre + ".running_var"], p[pre + ".weight"], p[pre + ".bias"], training, 0.1, 1e-5)

    def cps(t, pre, s, d):
        return F.relu(bn(F.conv2d(t, p[pre + ".conv.weight"], stride=s, padding=d, dilation=d), pre + ".bn"))

    def cpd(t, pre):
        t = F.relu(F.conv2d(t, p[pre + ".conv1.weight"], padding=2, dilation=2))
        t = F.relu(F.conv2d(t, p[pre + ".conv2.weight"], padding=2, dilation=2))
        return F.relu(bn(F.conv2d(t, p[pre + ".pool.weight"], stride=2, padding=1), pre + ".bn"))

    def up(t, pre):
        return F.relu(bn(F.conv_transpose2d(t, p[pre + ".conv.weight"], p[pre + ".conv.bias"], stride=2, padding=1, output_padding=1), pre + ".bn"))

    f0 = cps(cps(x, "FCN.conv0", 1, 2), "FCN.conv0_1", 1, 2)
    f1 = cps(f0, "FCN.conv1", 2, 1)
    f2 = cpd(f1, "FCN.conv2")
    f3 = cps(cps(cpd(f2, "FCN.conv3"), "FCN.conv4", 1, 2), "FCN.conv5", 1, 2)
    t = up(f3, "up1") + f2
    t = up(t, "up2") + f1
    t = up(t, "up3") + f0
    return F.conv2d(t, p["classifier.classifier.weight"], p["classifier.classifier.bias"])


def bench_fcn(steps, warmup, emit):
    N, H, W = 64, 120, 160
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=gen).to(DEV)
    t = torch.randint(0, 5, (N, H, W), generator=gen).to(DEV)
    torch.manual_seed(12345678)
    model = M.FCN().to(DEV)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = Trainer(model, class_weights=PB_W, optimizer=SGD(model, lr=1e-3, momentum=0.5, weight_decay=1e-3))
    p = {k: v.clone().requires_grad_() for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    buffers = {k: v.clone() for k, v in sd.items() if "running" in k}
    opt = torch.optim.SGD(list(p.values()), lr=1e-3, momentum=0.5, weight_decay=1e-3)
    cw = torch.tensor(PB_W, device=DEV)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(torch_fcn(p, x, True, buffers), t, cw).backward()
        opt.step()

    cands = {"step/hip": lambda: tr.step(x, t), "step/torch": torch_step}
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    times = interleaved(cands, steps, 3)
    ms = {k: statistics.median(v) for k, v in times.items()}
    emit({"what": "fcn_step", "N": N, "H": H, "W": W, "hip_ms_per_step": round(ms["step/hip"], 4), "torch_ms_per_step": round(ms["step/torch"], 4),
          "hip_ms_min_max": [round(min(times["step/hip"]), 4), round(max(times["step/hip"]), 4)],
          "torch_ms_min_max": [round(min(times["step/torch"]), 4), round(max(times["step/torch"]), 4)],
          "torch_over_hip": round(ms["step/torch"] / ms["step/hip"], 3), "hip_img_per_s": round(N / ms["step/hip"] * 1e3, 1), "steps": steps,
          "hip_loss": tr.pop_metrics()["loss"]})
    model.eval()
    pe = {k: v.detach() for k, v in p.items()}

    def torch_predict():
        with torch.no_grad():
            torch.max(torch_fcn(pe, x, False, buffers), 1)[1]

    cands = {"predict/hip": lambda: model.predict(x), "predict/torch": torch_predict}
    times = interleaved(cands, steps, 3)
    ms = {k: statistics.median(v) for k, v in times.items()}
    emit({"what": "fcn_predict", "N": N, "H": H, "W": W, "hip_ms": round(ms["predict/hip"], 4), "torch_ms": round(ms["predict/torch"], 4),
          "hip_ms_min_max": [round(min(times["predict/hip"]), 4), round(max(times["predict/hip"]), 4)],
          "torch_ms_min_max": [round(min(times["predict/torch"]), 4), round(max(times["predict/torch"]), 4)],
          "torch_over_hip": round(ms["predict/torch"] / ms["predict/hip"], 3), "calls": steps})


def bench_sep_blocks(emit):
    cases = [("ConvSep(16,32,3,2)", lambda: M.ConvSep(16, 32, 3, 2), (64, 16, 120, 160), 3.0),
             ("ConvSep(32,64,3,1)", lambda: M.ConvSep(32, 64, 3, 1), (64, 32, 30, 40), 3.0),
             ("ConvSep(128,128,3,1)", lambda: M.ConvSep(128, 128, 3, 1), (64, 128, 15, 20), 3.0),
             ("trConvSep(64,32)", lambda: M.trConvSep(64, 32), (64, 64, 15, 20), 1.8),
             ("trConvSep(32,16)", lambda: M.trConvSep(32, 16), (64, 32, 30, 40), 1.8),
             ("trConvSep(16,8)", lambda: M.trConvSep(16, 8), (64, 16, 60, 80), 1.8)]
    for name, make, shape, excess in cases:
        torch.manual_seed(3)
        mod = make().to(DEV).train()
        x = torch.randn(*shape, device=DEV, requires_grad=True)
        for _ in range(3):
            y = mod(x)
            y.backward(torch.ones_like(y))
        rows = mod._engine.profile_last(reps=5, with_loss=False)
        total = sum(r["ms"] for r in rows)
        is_cross = lambda r: r["kind"] in (L.OP_CONV, L.OP_TCONV, L.OP_WGRAD, L.OP_WGRAD_REDUCE, L.OP_CROSS_PACK, L.OP_CROSS_GRAD, L.OP_PACK)
        cross = sum(r["ms"] for r in rows if is_cross(r))
        pw = sum(r["ms"] for r in rows if r["kind"] in (L.OP_PW, L.OP_PW_WGRAD, L.OP_PW_WGRAD_REDUCE))
        emit({"what": "separable_block_step", "block": name, "input": list(shape), "records_ms": round(total, 4), "cross_records_ms": round(cross, 4),
              "pointwise_records_ms": round(pw, 4), "cross_share": round(cross / total, 3), "pointwise_share": round(pw / total, 3),
              "excess_multiplications": excess, "dedicated_1d_family_saves_at_most": round(cross / total * (1 - 1 / excess), 3),
              "rows": [[r["label"], round(r["ms"], 4)] for r in rows]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcn_bench.jsonl"))
    ap.add_argument("--only", default="pointwise,fcn,blocks")
    ap.add_argument("--wgrad-cap", type=int, default=0, help="i[AUX0] of the RCV_OP_PW_WGRAD records: filter blocks per wave (0 = the library's choice, 4, 8)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fcn.py measures on the GPU; no HIP device is visible")
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))

    only = a.only.split(",")
    if "pointwise" in only:
        bench_pointwise(a.reps, a.rounds, emit, a.wgrad_cap)
    if "fcn" in only:
        bench_fcn(a.steps, a.warmup, emit)
    if "blocks" in only:
        bench_sep_blocks(emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
