#!/usr/bin/env python3
"""The 5x5 classifier convolution family (csrc/conv5.hip) on the GPU box: its three records and the whole PB_FCN(32, 5, 5) step.

    python scripts/bench_cls5.py [--reps 200] [--rounds 5] [--steps 50] [--warmup 10] [--out profiles/cls5_bench.jsonl]

Records, at N x H x W = 32 x 120 x 160 with 8 and 16 input channels (the segmenters of PB_FCN(32, ..) / ROBO_UNet and of the v2 net):
RCV_OP_CONV5 forward (Cin -> 8 padded class channels), RCV_OP_CONV5 data gradient (8 -> Cin, RCV_F_RESID off, no statistics),
RCV_OP_WGRAD5 + RCV_OP_WGRAD5_REDUCE; next to them this package's 3x3 classifier records at the same shape (RCV_OP_CONV both ways,
RCV_OP_WGRAD + RCV_OP_WGRAD_REDUCE) and torch.nn.functional.conv2d (5x5, Cin -> 5, NCHW) with its autograd on the same card.  Each
figure is device-event time over `reps` back-to-back launches, the median of `rounds` such windows taken alternately over all
candidates; FLOPs are 2 * 25 (9) * Cin * classes(5) * pixels, the useful ones; issued_gflops counts what the 5x5 kernels hand the matrix pipe
(16 output rows per MFMA: 2 * 25 * K * 16 * pixels).
Whole step: Trainer.step of PB_FCN(32, 5, k, False, 0), k = 5, 3, 1, fused optim.SGD, batch 32 at 120 x 160.
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
N, H, W, CLASSES = 32, 120, 160, 5


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def record_candidates(cin):
    """name -> (callable that enqueues the work once, useful FLOPs, kernel labels)."""
    h = L.handle(0)
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(5 + cin)
    x = torch.randn(N, H, W, cin, generator=gen).to(DEV)
    g8 = torch.randn(N, H, W, 8, generator=gen).to(DEV)
    g8[..., CLASSES:] = 0
    px = N * H * W
    keep, out = [x, g8], {}

    def oplist(ops, name, taps, issued=None):
        lst = L.OpList(ops)
        labels = lst.labels(h)
        out[name] = (lambda: lst.run(h, stream), 2.0 * taps * cin * CLASSES * px, labels, issued)

    def ws(op):
        nbytes = L.op_workspace(h, op)
        if nbytes:
            t = torch.empty(nbytes // 4, device=DEV)
            keep.append(t)
            op.p[L.RCV_P_PART] = t.data_ptr()
        return op

    # ---- 5x5
    w5 = (torch.randn(CLASSES, cin, 5, 5, generator=gen) * 0.1).to(DEV)
    wp, wd = torch.zeros(25 * cin * 16, device=DEV), torch.zeros(25 * 8 * 16, device=DEV)
    L.OpList([L.make_op(L.OP_PACK5, 0, cin=cin, cout=CLASSES, p_in=w5.data_ptr(), p_out=wp.data_ptr()),
              L.make_op(L.OP_PACK5, L.F_FLIP, cin=cin, cout=CLASSES, p_in=w5.data_ptr(), p_out=wd.data_ptr())]).run(h, stream)
    z, dx = torch.empty(N, H, W, 8, device=DEV), torch.empty(N, H, W, cin, device=DEV)
    dw5, db = torch.empty_like(w5), torch.empty(CLASSES, device=DEV)
    keep += [w5, wp, wd, z, dx, dw5, db]
    dims = dict(n=N, h=H, w=W, ho=H, wo=W, stride=1, dil=1)
    oplist([L.make_op(L.OP_CONV5, 0, cin=cin, cout=8, inmode=L.LOAD_PLAIN, p_in=x.data_ptr(), p_w=wp.data_ptr(), p_out=z.data_ptr(), **dims)],
           "conv5_fwd", 25, 2.0 * 25 * cin * 16 * px)
    oplist([L.make_op(L.OP_CONV5, 0, cin=8, cout=cin, inmode=L.LOAD_PLAIN, p_in=g8.data_ptr(), p_w=wd.data_ptr(), p_out=dx.data_ptr(), **dims)],
           "conv5_dgrad", 25, 2.0 * 25 * 8 * 16 * px)
    wop = ws(L.make_op(L.OP_WGRAD5, L.F_BIAS, cin=cin, cout=8, inmode=L.LOAD_PLAIN, inmode2=L.LOAD_PLAIN, p_in=x.data_ptr(),
                       p_in2=g8.data_ptr(), **dims))
    oplist([wop, L.make_op(L.OP_WGRAD5_REDUCE, 0, cin=cin, cout=CLASSES, nsplit=wop.i[L.RCV_I_NSPLIT], p_part=wop.p[L.RCV_P_PART],
                           p_out=dw5.data_ptr(), p_bias=db.data_ptr())], "wgrad5+reduce", 25, 2.0 * 25 * 16 * 16 * px)

    # ---- this package's 3x3 classifier records (engine.fwd_cls / bwd_cls, plain filter layout)
    w3 = (torch.randn(CLASSES, cin, 3, 3, generator=gen) * 0.1).to(DEV)
    dw3 = torch.empty_like(w3)

    def pack3(rows_from_d1, flip):
        rows, cols = (cin, CLASSES) if rows_from_d1 else (CLASSES, cin)
        rp, cp = (rows + 3) // 4 * 4, (cols + 15) // 16 * 16
        dst = torch.zeros(9 * rp * cp, device=DEV)
        job = L.RcvPackJob()
        job.src, job.dst, job.D0, job.D1 = w3.data_ptr(), dst.data_ptr(), CLASSES, cin
        job.rows_from_d1, job.flip, job.rows_pad, job.cols_pad, job.merged = int(rows_from_d1), int(flip), rp, cp, 0
        table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * 1)(job))), dtype=torch.uint8).to(DEV)
        L.OpList([L.make_op(L.OP_PACK, 0, count=1, aux0=9 * rp * cp, p_in=table.data_ptr())]).run(h, stream)
        torch.cuda.synchronize()
        keep.append(dst)
        return dst

    wp3, wd3 = pack3(True, False), pack3(False, True)
    keep += [w3, dw3]
    oplist([L.make_op(L.OP_CONV, 0, cin=cin, cout=8, inmode=L.LOAD_PLAIN, p_in=x.data_ptr(), p_w=wp3.data_ptr(), p_out=z.data_ptr(), **dims)],
           "conv3_fwd", 9)
    oplist([L.make_op(L.OP_CONV, 0, cin=8, cout=cin, inmode=L.LOAD_PLAIN, p_in=g8.data_ptr(), p_w=wd3.data_ptr(), p_out=dx.data_ptr(), **dims)],
           "conv3_dgrad", 9)
    wop3 = ws(L.make_op(L.OP_WGRAD, L.F_BIAS, cin=cin, cout=8, inmode=L.LOAD_PLAIN, inmode2=L.LOAD_PLAIN, p_in=x.data_ptr(),
                        p_in2=g8.data_ptr(), **dims))
    oplist([wop3, L.make_op(L.OP_WGRAD_REDUCE, 0, cin=cin, cout=CLASSES, nsplit=wop3.i[L.RCV_I_NSPLIT], p_part=wop3.p[L.RCV_P_PART],
                            p_out=dw3.data_ptr(), p_bias=db.data_ptr())], "wgrad3+reduce", 9)

    # ---- torch on the same card: conv2d 5x5 NCHW and its autograd
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    wt, bt = w5.clone().requires_grad_(), torch.zeros(CLASSES, device=DEV, requires_grad=True)
    gt = g8[..., :CLASSES].permute(0, 3, 1, 2).contiguous()
    keep += [xt, wt, bt, gt]

    def torch_fwd():
        with torch.no_grad():
            F.conv2d(xt, wt, bt, padding=2)

    def torch_fwd_bwd():
        xt.grad = wt.grad = bt.grad = None
        F.conv2d(xt, wt, bt, padding=2).backward(gt)

    out["torch_conv2d_fwd"] = (torch_fwd, 2.0 * 25 * cin * CLASSES * px, ["aten::conv2d"], None)
    out["torch_conv2d_fwd+bwd"] = (torch_fwd_bwd, 3 * 2.0 * 25 * cin * CLASSES * px, ["aten::conv2d + autograd"], None)
    out["_keep"] = keep
    return out


def bench_records(cin, reps, rounds, emit):
    cands = record_candidates(cin)
    names = [k for k in cands if not k.startswith("_")]
    for k in names:
        window(cands[k][0], 10)                  # warm-up: code objects, algorithm choice of the library
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for _ in range(rounds):                      # alternate the candidates: drift of the shared box hits all alike
        for k in names:
            times[k].append(window(cands[k][0], reps))
    for k in names:
        ms = statistics.median(times[k])
        emit({"what": "record", "name": k, "cin": cin, "N": N, "H": H, "W": W, "classes": CLASSES, "labels": cands[k][2],
              "ms": round(ms, 5), "ms_min": round(min(times[k]), 5), "ms_max": round(max(times[k]), 5), "reps": reps, "rounds": rounds,
              "useful_gflops": round(cands[k][1] / ms / 1e6, 1),
              "issued_gflops": round(cands[k][3] / ms / 1e6, 1) if cands[k][3] else None})


def bench_step(ksize, steps, warmup, emit):
    torch.manual_seed(12345678)
    model = M.PB_FCN(32, CLASSES, ksize, False, 0).to(DEV)
    tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=SGD(model, lr=1e-3, momentum=0.5, weight_decay=1e-3))
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=gen).to(DEV)
    t = torch.randint(0, CLASSES, (N, H, W), generator=gen).to(DEV)
    for _ in range(warmup):
        tr.step(x, t)
    torch.cuda.synchronize()
    ms = [window(lambda: tr.step(x, t), steps) for _ in range(3)]
    emit({"what": "step", "name": "PB_FCN(32,5,%d,False,0)" % ksize, "N": N, "H": H, "W": W, "ms_per_step": round(statistics.median(ms), 4),
          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": steps, "img_per_s": round(N / statistics.median(ms) * 1e3, 1),
          "loss": tr.pop_metrics()["loss"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls5_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cls5.py measures on the GPU; no HIP device is visible")
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))

    for cin in (8, 16):
        bench_records(cin, a.reps, a.rounds, emit)
    for k in (5, 3, 1):
        bench_step(k, a.steps, a.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
