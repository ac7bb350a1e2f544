#!/usr/bin/env python3
"""Images per second of whole training epochs of the RGB loader and of LabelProp frame pairs from a device-resident dataset
(``RGBEpochLoader`` / ``LPEpochLoader``, robocupvision_amd/data.py) on the GPU box, next to the training step alone and to the
upload-every-batch path they replace.  The method of scripts/bench_epoch.py: device events, windows of at least --min-seconds after
a warm-up, --repeats windows, the median with the slowest and the fastest window next to it.

    python scripts/bench_rgb_epoch.py [--section pbfcn|labelprop|ops|all] [--frames 1024] [--out profiles/rgb_epoch_bench.jsonl]

A synthetic store (seeded noise made on the device, ``ResidentDataset.from_tensors``; 480x640 -> 120x160); no files.  One section per
call keeps every call short (run each under its own ``timeout``); lines are APPENDED to --out, one JSON line per measurement.
  pbfcn      ``PB_FCN(32, 5, 1, False, 0)`` + ``optim.SGD`` at batch 32 (trainer.py):
               step    (a) ``Trainer.step`` alone on one fixed prepared batch
               epoch   (b) whole epochs through ``RGBEpochLoader``, ``check()`` after each; ``epoch_prefetch``: the same with ``prefetch=True``
               upload  (c) the path as it was: decoded frames (uint8) and labels (int32) wait in pinned host memory -> ``torch.stack``
                       into a pinned staging buffer (two, alternating) -> upload -> ``draw_color_jitter`` -> ``prepare_rgb_batch`` -> step
  labelprop  ``LabelProp(5, 32, 0)`` + ``optim.SGD`` at 8 pairs (labelPropTrain.py): (a') the step alone, (b') epochs through
             ``LPEpochLoader``, (c') upload of the 16 frames -> ``prepare_rgb_batch`` (every row repeated) -> ``labelprop_batch`` -> step
  ops        the two ops alone, microseconds per call as 256 copies of the record run by one library call (the device sets the pace),
             with and without the statistics launch, and the bytes they move against 8 TB/s
Ratios (b)/(a) and (b)/(c) are in each section's ``summary`` line."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd import _lib as L              # noqa: E402
from robocupvision_amd import data as D              # noqa: E402
from robocupvision_amd.optim import SGD              # noqa: E402
from robocupvision_amd.train import Trainer          # noqa: E402
from bench_epoch import rate, windows                # noqa: E402

PEAK_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["pbfcn", "labelprop", "ops", "all"])
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--size", type=int, nargs=2, default=(120, 160))
    ap.add_argument("--host-pool", type=int, default=128, help="decoded frames kept in pinned host memory for (c)")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_epoch_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rgb_epoch.py measures on the GPU only: no HIP device here (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    N, B, P2, src, size = a.frames, a.batch, a.pairs, tuple(a.src), tuple(a.size)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(what, row):
        row = dict({"what": what, "frames": N, "src": list(src), "size": list(size)}, **row)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    g = torch.Generator(device=dev).manual_seed(41)
    frames = torch.randint(0, 256, (N, src[0], src[1], 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 5, (N, src[0], src[1]), dtype=torch.uint8, device=dev, generator=g)
    store = D.ResidentDataset.from_tensors(frames, labels, size, chunk=64)
    Pn = min(a.host_pool, N)
    pool_f = [frames[i].cpu().pin_memory() for i in range(Pn)]
    pool_l = [labels[i].to(torch.int32).cpu().pin_memory() for i in range(Pn)]          # Image.convert("I") decodes to int32
    del frames, labels
    torch.cuda.empty_cache()
    random.seed(42)
    np.random.seed(42)

    def staged_upload(n):
        """-> fn(k) giving batch k of n decoded frames on the device: pinned pool -> stack into a pinned staging buffer -> upload."""
        stage = [(torch.empty((n,) + tuple(pool_f[0].shape), dtype=torch.uint8).pin_memory(),
                  torch.empty((n,) + tuple(pool_l[0].shape), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        order = torch.randperm(Pn, generator=torch.Generator().manual_seed(45)).tolist()

        def fn(k):
            sf, sl, ev = stage[k % 2]
            ev.synchronize()                                        # the copy that last read this staging buffer has finished
            pick = [order[(k * n + i) % Pn] for i in range(n)]
            torch.stack([pool_f[i] for i in pick], out=sf)
            torch.stack([pool_l[i] for i in pick], out=sl)
            f, lab = sf.to(dev, non_blocking=True), sl.to(dev, non_blocking=True)
            ev.record()
            return f, lab
        return fn

    def three_paths(tag, tr, fixed, make_loader, per_epoch, per_batch, upload_step):
        loader = make_loader(False)
        step = rate(windows(lambda: tr.step(*fixed), 1, a.min_seconds, a.repeats, a.warmup), per_batch)
        emit(tag + "_step", step)

        def epoch():
            for x, t in loader:
                tr.step(x, t)
            store.check()
        ep = rate(windows(epoch, 1, a.min_seconds, a.repeats, 1), per_epoch)
        ep["batches_per_epoch"] = len(loader)
        emit(tag + "_epoch", ep)
        # ... with the next epoch's host work (permutation, draw_color_jitter_rows, two uploads) done at the end of the running one
        loader_p = make_loader(True)

        def epoch_prefetch():
            for x, t in loader_p:
                tr.step(x, t)
            store.check()
        ep_pre = rate(windows(epoch_prefetch, 1, a.min_seconds, a.repeats, 1), per_epoch)
        emit(tag + "_epoch_prefetch", ep_pre)
        t0 = time.perf_counter()
        loader._draw_epoch()
        torch.cuda.synchronize()
        host_ms = round((time.perf_counter() - t0) * 1e3, 3)          # the host work of one epoch on an idle device
        state = {"k": 0}

        def upload():
            state["k"] += 1
            upload_step(state["k"])
        up = rate(windows(upload, 1, a.min_seconds, a.repeats, a.warmup), per_batch)
        emit(tag + "_upload", up)
        emit(tag + "_summary", {"epoch_over_step": round(ep["img_per_s"] / step["img_per_s"], 4),
                                "epoch_over_step_slowest_fastest": [round(ep["img_per_s_min"] / step["img_per_s_max"], 4),
                                                                    round(ep["img_per_s_max"] / step["img_per_s_min"], 4)],
                                "epoch_over_upload": round(ep["img_per_s"] / up["img_per_s"], 3),
                                "epoch_over_upload_slowest_fastest": [round(ep["img_per_s_min"] / up["img_per_s_max"], 3),
                                                                      round(ep["img_per_s_max"] / up["img_per_s_min"], 3)],
                                "epoch_prefetch_over_step": round(ep_pre["img_per_s"] / step["img_per_s"], 4),
                                "epoch_prefetch_over_step_slowest_fastest": [round(ep_pre["img_per_s_min"] / step["img_per_s_max"], 4),
                                                                             round(ep_pre["img_per_s_max"] / step["img_per_s_min"], 4)],
                                "step_ms": step["ms"], "epoch_ms_per_batch": round(ep["ms"] / len(loader), 5),
                                "epoch_prefetch_ms_per_batch": round(ep_pre["ms"] / len(loader), 5), "upload_ms_per_batch": up["ms"],
                                "host_ms_per_epoch": host_ms, "batches_per_epoch": len(loader),
                                "host_ms_per_epoch_over_batches": round(host_ms / len(loader), 5)})

    if a.section in ("pbfcn", "all"):
        torch.manual_seed(12345678)
        model = M.PB_FCN(32, 5, 1, False, 0).to(dev)
        tr = Trainer(model, class_weights=[1, 6, 1.5, 3, 3], optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))

        def make_loader(prefetch):
            return D.RGBEpochLoader(store, B, generator=torch.Generator().manual_seed(44), prefetch=prefetch)
        fixed = D.prepare_rgb_batch(store.frames, store.labels, img_size=size, params=D.draw_color_jitter_rows(B),
                                    index=torch.arange(B, device=dev), bad_index=store.bad_index)
        up_fn = staged_upload(B)

        def upload_step(k):
            f, lab = up_fn(k)
            tr.step(*D.prepare_rgb_batch(f, lab, img_size=size, params=D.draw_color_jitter(B)))
        three_paths("pbfcn_b%d" % B, tr, fixed, make_loader, N, B, upload_step)

    if a.section in ("labelprop", "all"):
        torch.manual_seed(12345678)
        model = M.LabelProp(5, 32, 0).to(dev)
        tr = Trainer(model, class_weights=(1, 6, 1, 3, 2), optimizer=SGD(model, lr=2e-1, momentum=0.5, weight_decay=1e-3))
        wins = torch.stack([torch.arange(N - 1), torch.arange(N - 1) + 1], 1)

        def make_loader(prefetch):
            return D.LPEpochLoader(store, wins, P2, generator=torch.Generator().manual_seed(44), drop_last=True, prefetch=prefetch)
        fixed = D.prepare_lp_pairs(store.frames, store.labels, wins[:P2].to(dev), params=D.draw_color_jitter_rows(P2), bad_index=store.bad_index)
        up_fn = staged_upload(2 * P2)

        def upload_step(k):
            f, lab = up_fn(k)
            x, t = D.prepare_rgb_batch(f, lab, img_size=size, params=D.draw_color_jitter(P2).repeat_interleave(2, 0))
            tr.step(*M.labelprop_batch(x.view(P2, 2, 3, size[0], size[1]), t.view(P2, 2, size[0], size[1])))
        three_paths("labelprop_p%d" % P2, tr, fixed, make_loader, ((N - 1) // P2) * 2 * P2, 2 * P2, upload_step)

    if a.section in ("ops", "all"):
        h = L.handle(dev.index)
        stream = torch.cuda.current_stream(dev).cuda_stream
        H, W = size
        fx, kx, fy, ky, lx, ly = D._device_tables(H, W, H, W, dev)
        K = 256
        lab_b = store.labels.element_size()
        for what, n_rows, make, nbytes in (
                ("rgb_prep_idx_b%d" % B, B,
                 lambda st, rows, idx, out, tgt: L.make_op(
                     L.OP_RGB_PREP_IDX, n=B, stride=N, inmode=8, h=H, w=W, ho=H, wo=W, cin=kx, cout=ky, inmode2=lab_b, aux0=1, aux1=0, count=st,
                     p_in=store.frames.data_ptr(), p_in2=store.labels.data_ptr(), p_in_aux=idx.data_ptr(), p_epi_aux=store.bad_index.data_ptr(),
                     p_out=out.data_ptr(), p_x0=tgt.data_ptr(), p_x1=fx.data_ptr(), p_x2=fy.data_ptr(), p_x3=lx.data_ptr(), p_x4=ly.data_ptr(),
                     p_in_c=rows.data_ptr()),
                 B * H * W * (3 + lab_b + 12 + 8)),
                ("lp_pair_prep_p%d" % P2, P2,
                 lambda st, rows, idx, out, tgt: L.make_op(
                     L.OP_LP_PAIR_PREP, n=P2, stride=N, inmode=8, h=H, w=W, ho=H, wo=W, cout=5, inmode2=lab_b, aux0=1, count=st,
                     p_in=store.frames.data_ptr(), p_in2=store.labels.data_ptr(), p_in_aux=idx.data_ptr(), p_epi_aux=store.bad_index.data_ptr(),
                     p_out=out.data_ptr(), p_x0=tgt.data_ptr(), p_in_c=rows.data_ptr()),
                 2 * P2 * H * W * (3 + lab_b + 32 + 8))):
            pair = what.startswith("lp")
            rows = D.draw_color_jitter_rows(n_rows).to(dev)
            idx = torch.randperm(N, generator=torch.Generator().manual_seed(43))[:2 * n_rows if pair else n_rows].to(dev)
            out = torch.empty(2 * P2 * H * W * 8 if pair else B * 3 * H * W, dtype=torch.float32, device=dev)
            tgt = torch.empty(2 * P2 * H * W if pair else B * H * W, dtype=torch.int64, device=dev)
            res = {}
            for st in (1, 0):          # with the statistics launch (every drawn row holds a contrast) / told that none does: blends towards 0
                op = make(st, rows, idx, out, tgt)
                need = L.op_workspace(h, op)
                ws = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
                op.p[L.RCV_P_PART] = ws.data_ptr()
                ops = L.OpList([op] * K)
                r = windows(lambda: ops.run(h, stream), K, a.min_seconds, a.repeats, a.warmup)
                res["two_launches" if st else "main_launch_alone"] = dict(r, us=round(r["ms"] * 1e3, 3))
            stat_bytes = (2 * P2 if pair else B) * H * W * 3
            main_us, both_us = res["main_launch_alone"]["us"], res["two_launches"]["us"]
            emit(what, dict(res, MB_moved_main=round(nbytes / 1e6, 3), MB_read_statistics=round(stat_bytes / 1e6, 3),
                            main_TBps=round(nbytes / (main_us * 1e-6) / 1e12, 3), main_share_of_peak=round(nbytes / (main_us * 1e-6) / 1e12 / PEAK_TBPS, 4),
                            us_at_peak=round((nbytes + stat_bytes) / (PEAK_TBPS * 1e12) * 1e6, 3), statistics_launch_us=round(both_us - main_us, 3)))
        store.check()


if __name__ == "__main__":
    main()
