#!/usr/bin/env python
"""Device time of one farneback_flow call (RCV_OP_FARNEBACK, csrc/flow.hip) on B pairs of 120x160 gray frames with the reference's
parameters (transform.py:185-187): HIP events, warmed up, median of --iters.  Every sample times, one after the other in the same loop,
the HIP path and -- the bar it has to beat -- the same algorithm composed from eager torch ops on the same card (separable conv2d,
interpolate, gather, avg_pool2d; `eager_flow` below, checked against the HIP result in every line).  Next to it what a user had before:
the frames taken to the host and the numpy restatement of the contract (tests/farneback_restatement.py, float64), timed on at most
--cpu-pairs pairs and scaled to the batch; and the device time of the label remap (RCV_OP_REMAP_LABELS) of the same batch.  One JSON
line per batch size, appended to --out.

    python scripts/bench_flow.py [--iters 30] [--warmup 5] [--batches 1,64] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import farneback_restatement as F  # noqa: E402
from robocupvision_amd import _lib as L  # noqa: E402
from robocupvision_amd import flow as FL  # noqa: E402

DEV = "cuda:0"
H, W = 120, 160


# ---- the same algorithm from eager torch ops (every function is its namesake of the restatement, batched) ------------------------------
def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32, device=DEV)


def _corr(a, taps, axis, mode):
    """a [N,C,H,W]; one 1-D correlation per channel along axis 2 (rows) or 3 (columns); taps [K, k]: K outputs per channel."""
    N, C, h, w = a.shape
    K, k = taps.shape
    r = (k - 1) // 2
    a = TF.pad(a, (r, r, 0, 0) if axis == 3 else (0, 0, r, r), mode=mode)
    wgt = taps.view(K, 1, 1, k) if axis == 3 else taps.view(K, 1, k, 1)
    return TF.conv2d(a, wgt.repeat(C, 1, 1, 1), groups=C)          # [N, C*K, h, w], channel c*K + j


def _resize(a, h, w):
    return TF.interpolate(a, size=(h, w), mode="bilinear", align_corners=False)


class EagerFlow:
    def __init__(self, levels=2, winsize=15, iterations=2, poly_n=7, poly_sigma=1.5):
        self.levels, self.winsize, self.iterations = levels, winsize, iterations
        g, xg, xxg = F.poly_taps(poly_n, poly_sigma)
        self.vert = _t(np.stack([g, xg, xxg]))
        self.gi = np.linalg.inv(F.normal_matrix(poly_n, poly_sigma))
        self.cache = {}

    def plane_consts(self, j, h, w):
        if (j, h, w) not in self.cache:
            ys, xs = torch.meshgrid(torch.arange(h, device=DEV, dtype=torch.float32), torch.arange(w, device=DEV, dtype=torch.float32),
                                    indexing="ij")
            self.cache[(j, h, w)] = (_t(F.blur_taps(j))[None], _t(F.border_scale(h, w, np.float64)), xs, ys)
        return self.cache[(j, h, w)]

    def poly_exp(self, img):
        v = _corr(img, self.vert, 2, "replicate")                    # [N, 3, h, w]: g, j g, j^2 g down the columns
        m = _corr(v, self.vert, 3, "replicate")                      # [N, 9, h, w]: channel 3 a + b = vertical a, horizontal b
        gi = self.gi
        m1, mx, mxx, my, mxy, myy = m[:, 0], m[:, 1], m[:, 2], m[:, 3], m[:, 4], m[:, 6]
        return torch.stack([gi[1, 1] * mx, gi[2, 2] * my, gi[3, 0] * m1 + gi[3, 3] * mxx + gi[3, 4] * myy,
                            gi[4, 0] * m1 + gi[4, 3] * mxx + gi[4, 4] * myy, gi[5, 5] * mxy], 1)

    def matrices(self, R0, R1, flow, scale, xs, ys):
        B, _, h, w = R0.shape
        dx, dy = flow[:, 0], flow[:, 1]
        fx, fy = xs + dx, ys + dy
        x1, y1 = torch.floor(fx), torch.floor(fy)
        ok = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
        a, b = (fx - x1)[:, None], (fy - y1)[:, None]
        idx = torch.where(ok, y1 * w + x1, torch.zeros_like(x1)).long().view(B, 1, h * w).expand(B, 5, h * w)
        flat = R1.reshape(B, 5, h * w)
        r00, r01 = flat.gather(2, idx).view(B, 5, h, w), flat.gather(2, idx + 1).view(B, 5, h, w)
        r10, r11 = flat.gather(2, idx + w).view(B, 5, h, w), flat.gather(2, idx + w + 1).view(B, 5, h, w)
        Rw = (r00 * (1 - a) + r01 * a) * (1 - b) + (r10 * (1 - a) + r11 * a) * b
        own = torch.cat([torch.zeros_like(R0[:, :2]), R0[:, 2:]], 1)
        Rw = torch.where(ok[:, None], Rw, own)
        bx, by = (R0[:, 0] - Rw[:, 0]) * 0.5, (R0[:, 1] - Rw[:, 1]) * 0.5
        axx, ayy, axy = (R0[:, 2] + Rw[:, 2]) * 0.5, (R0[:, 3] + Rw[:, 3]) * 0.5, (R0[:, 4] + Rw[:, 4]) * 0.25
        bx = bx + (axx * dx + axy * dy)
        by = by + (axy * dx + ayy * dy)
        bx, by, axx, ayy, axy = bx * scale, by * scale, axx * scale, ayy * scale, axy * scale
        return torch.stack([axx * axx + axy * axy, (axx + ayy) * axy, ayy * ayy + axy * axy, axx * bx + axy * by, axy * bx + ayy * by], 1)

    def __call__(self, p, q):
        B, Hh, Ww = p.shape
        frames = torch.cat([p, q]).float()[:, None]
        r = self.winsize // 2
        flow = None
        for j in range(F.n_coarse(Hh, Ww, self.levels), -1, -1):
            h, w = F.plane_size(Hh, Ww, j)
            taps, scale, xs, ys = self.plane_consts(j, h, w)
            img = _resize(_corr(_corr(frames, taps, 3, "reflect"), taps, 2, "reflect"), h, w)
            R = self.poly_exp(img)
            R0, R1 = R[:B], R[B:]
            flow = torch.zeros(B, 2, h, w, device=DEV) if flow is None else _resize(flow, h, w) * 2
            M = self.matrices(R0, R1, flow, scale, xs, ys)
            for it in range(self.iterations):
                Mb = TF.avg_pool2d(TF.pad(M, (r, r, r, r), mode="replicate"), self.winsize, stride=1)
                idet = 1.0 / (Mb[:, 0] * Mb[:, 2] - Mb[:, 1] * Mb[:, 1] + 1e-3)
                flow = torch.stack([(Mb[:, 2] * Mb[:, 3] - Mb[:, 1] * Mb[:, 4]) * idet, (Mb[:, 0] * Mb[:, 4] - Mb[:, 1] * Mb[:, 3]) * idet], 1)
                if it + 1 < self.iterations:
                    M = self.matrices(R0, R1, flow, scale, xs, ys)
        return flow


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--no-cpu", action="store_true", help="skip the host alternative")
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow.py needs the GPU: there is nothing to time without one")
    h = L.handle(0)
    eager = EagerFlow()
    for B in [int(b) for b in a.batches.split(",")]:
        rng = np.random.default_rng(11)
        pairs = [F.shifted_pair(rng, H, W, (int(rng.integers(-5, 6)), int(rng.integers(-5, 6)))) for _ in range(B)]
        p, q = np.stack([x for x, _ in pairs]), np.stack([y for _, y in pairs])
        pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
        lab = torch.randint(0, 5, (B, H, W), dtype=torch.uint8, device=DEV)
        flow = FL.farneback_flow(pd, qd)
        calls = {"hip": lambda: FL.farneback_flow(pd, qd), "eager": lambda: eager(pd, qd), "remap": lambda: FL.update_labels(lab, flow)}
        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(a.iters):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        res = {"B": B, "H": H, "W": W, "params": "levels 2, winsize 15, iterations 2, poly_n 7, poly_sigma 1.5", "iters": a.iters,
               "label": L.OpList([FL.FlowRecord(B, H, W).op]).labels(h)[0], "workspace_bytes": FL.FlowRecord(B, H, W).workspace_bytes(h)}
        for k, v in times.items():
            res[k + "_ms_median"] = round(statistics.median(v), 4)
            res[k + "_ms_min"] = round(min(v), 4)
        res["hip_pairs_per_s"] = round(B / statistics.median(times["hip"]) * 1e3, 1)
        res["eager_pairs_per_s"] = round(B / statistics.median(times["eager"]) * 1e3, 1)
        res["hip_over_eager"] = round(statistics.median(times["eager"]) / statistics.median(times["hip"]), 2)
        res["eager_vs_hip_max_px"] = float((eager(pd, qd) - flow).abs().max())
        if not a.no_cpu:
            nb = min(B, a.cpu_pairs)
            t0 = time.perf_counter()
            ref = np.stack([F.farneback_flow(pd[b].cpu().numpy(), qd[b].cpu().numpy()) for b in range(nb)])
            dt = time.perf_counter() - t0
            res["host_pairs"] = nb
            res["host_pairs_per_s"] = round(nb / dt, 1)
            res["host_ms_per_call"] = round(dt * 1e3 * B / nb, 1)
            res["hip_vs_host_max_px"] = float(np.abs(flow[:nb].cpu().numpy() - ref).max())
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
