#!/usr/bin/env python3
"""Per-frame device time of label propagation on predictions (infer.LabelPropagator, RCV_OP_LP_INPUT) at 120x160 on the GPU box.

    python scripts/bench_lp_stream.py [--only B] [--min-seconds 1.0] [--repeats 3] [--out profiles/lp_stream_bench.jsonl]

One JSON line per case and batch size (B = 1 and 32), all on the same build, in the same process, on one card:
  key_frame          ``seg.predict(imgs)``: what the driver runs on a key frame
  propagated         ``lp.predict(labelprop_next(imgs, plane, labels_prev, keep_plane=True)[0])``: the driver's propagated frame
  workaround         the same frame through the ops that existed before: the fake pair ``[cur, prev]``, labels ``[zeros,
                     prior.long()]``, ``labelprop_batch``, the even samples gathered contiguous, ``lp.predict``
  segmenter_always   ``seg.predict(imgs)`` on every frame (the same call as key_frame, timed in its own window: the spread between the
                     two is the noise of the box)
  propagated_soft    ``lp(labelprop_next(imgs, plane, logits_prev, keep_plane=True)[0])`` and the arg-max: the soft driver's frame
  eager_soft_prior   the soft prior in eager torch (softmax, scale, cat, NHWC re-layout), then ``lp(x)`` and the arg-max
  op_*               ``labelprop_next(keep_plane=True)`` alone (the Python call: two allocations, one ctypes call, one launch)
  op_*_x200          the RCV_OP_LP_INPUT record alone, 200 launches back to back in one ``rcv_run``, per launch, with the bytes it
                     must move and the share of the 8 TB/s HBM peak that is (the operands stay cache resident: not an HBM figure)
Each entry: median ms over --repeats windows of at least --min-seconds (device events, after warm-up), spread = max - min.  At B = 1
every case is a handful of launches of a few microseconds: the numbers are launch-bound and say so (``calls_per_window``)."""
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
HBM_PEAK = 8e12
H, W = 120, 160


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


def run(B, a):
    torch.manual_seed(12345678)
    seg, lp = M.ROBO_UNet().to(DEV).eval(), M.LabelProp(5, 32).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(7)
    imgs, prev_imgs = torch.randn(B, 3, H, W, device=DEV, generator=g), torch.randn(B, 3, H, W, device=DEV, generator=g)
    rows = []
    with torch.no_grad():
        labels_prev, logits_prev = seg.predict(prev_imgs), seg(prev_imgs)
        plane = prev_imgs[:, 0].contiguous()
        zeros = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)

        def propagated():
            x, _ = M.labelprop_next(imgs, plane, labels_prev, keep_plane=True)
            return lp.predict(x)

        def workaround():
            pair = torch.stack([imgs, prev_imgs], 1)
            lab2 = torch.stack([zeros, labels_prev.long()], 1)
            x = M.labelprop_batch(pair, lab2)[0].permute(0, 2, 3, 1)[0::2].contiguous().permute(0, 3, 1, 2)
            return lp.predict(x)

        def propagated_soft():
            x, _ = M.labelprop_next(imgs, plane, logits_prev, keep_plane=True)
            return torch.max(lp(x), 1)[1].to(torch.uint8)

        def eager_soft_prior():
            prior = torch.softmax(logits_prev, 1) * 2 - 1.0
            y, yp = imgs[:, 0:1], plane[:, None]
            x = torch.cat([y, yp, y - yp, prior], 1).contiguous(memory_format=torch.channels_last)
            return torch.max(lp(x), 1)[1].to(torch.uint8)

        same = bool(torch.equal(propagated(), workaround()))
        cases = [("key_frame", lambda: seg.predict(imgs)), ("propagated", propagated), ("workaround", workaround),
                 ("segmenter_always", lambda: seg.predict(imgs)), ("propagated_soft", propagated_soft), ("eager_soft_prior", eager_soft_prior)]
        for name, fn in cases:
            row = {"case": name, "B": B, "size": [H, W]}
            row.update(timed(fn, a.min_seconds, a.repeats))
            if name in ("propagated", "workaround"):
                row["labels_equal_other_path"] = same
            rows.append(row)
        n = B * H * W
        for name, prior, per_pixel in (("op_u8", labels_prev, 8 + 1 + 32 + 4), ("op_i64", labels_prev.long(), 8 + 8 + 32 + 4),
                                       ("op_logits", logits_prev, 8 + 20 + 32 + 4)):
            row = {"case": name, "B": B, "size": [H, W], "bytes_per_pixel": per_pixel}
            row.update(timed(lambda: M.labelprop_next(imgs, plane, prior, keep_plane=True), a.min_seconds / 2, a.repeats))
            row["roofline_us_at_8TBps"] = round(n * per_pixel / HBM_PEAK * 1e6, 3)
            row["share_of_8TBps_hbm_peak"] = round(n * per_pixel / (row["ms"] * 1e-3) / HBM_PEAK, 4)
            row["note"] = "includes the two torch.empty allocations of labelprop_next"
            rows.append(row)
            # the launch alone: one rcv_run of 200 identical records back to back (no Python, no allocation between them)
            out, keep = torch.empty(B, H, W, 8, device=DEV), torch.empty(B, H, W, device=DEV)
            op = L.make_op(L.OP_LP_INPUT, 0, n=B, h=H, w=W, cin=3, cout=5, inmode={1: 1, 8: 8, 4: 4}[prior.element_size()], aux1=1,
                           p_in=imgs.data_ptr(), p_in2=plane.data_ptr(), p_x0=prior.data_ptr(), p_out=out.data_ptr(), p_x1=keep.data_ptr())
            ops, h, stream = L.OpList([op] * 200), L.handle(0), torch.cuda.current_stream(DEV).cuda_stream
            row = {"case": name + "_x200", "B": B, "size": [H, W], "bytes_per_pixel": per_pixel}
            t = timed(lambda: ops.run(h, stream), a.min_seconds / 2, a.repeats)
            row.update({k: (round(v / 200, 6) if k.endswith("ms") else v) for k, v in t.items()})
            row["roofline_us_at_8TBps"] = round(n * per_pixel / HBM_PEAK * 1e6, 3)
            row["share_of_8TBps_hbm_peak"] = round(n * per_pixel / (row["ms"] * 1e-3) / HBM_PEAK, 4)
            row["note"] = "per launch of 200 back to back in one rcv_run; operands of 20-39 MB stay in the 256 MiB Infinity Cache"
            assert torch.equal(out.permute(0, 3, 1, 2), M.labelprop_next(imgs, plane, prior)) and torch.equal(keep, imgs[:, 0])
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lp_stream.py measures on the GPU; no HIP device here (nothing is timed on a CPU)")
    out = open(a.out, "w") if a.out else None
    for B in ([a.only] if a.only else [1, 32]):
        for row in run(B, a):
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
