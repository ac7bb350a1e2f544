#!/usr/bin/env python3
"""Images per second of whole training epochs from a device-resident dataset (``ResidentDataset`` + ``EpochLoader``,
robocupvision_amd/data.py) on the GPU box, next to the training step alone and to the upload-every-batch path it replaces.

    python scripts/bench_epoch.py [--frames 4096] [--batch 64] [--min-seconds 0.5] [--repeats 5] [--out profiles/epoch_bench.jsonl]

A synthetic store (seeded noise made on the device, ``ResidentDataset.from_tensors``; default 4096 frames 480x640 -> 120x160, batch
64), the default ``ROBO_UNet`` and ``Trainer``; no files.  Everything runs in one process; every figure is the median of --repeats
windows of at least --min-seconds, timed with device events after a warm-up, with the spread (max - min) of the windows next to it.
One JSON line per measurement (stdout and --out), then the table of DESIGN 4.13:
  step          (a) ``Trainer.step`` alone on one fixed prepared batch
  epoch         (b) whole epochs through ``EpochLoader``: one ``prepare_batch(index=)`` + one ``Trainer.step`` per batch, ``check()`` per epoch
  upload        (c) the documented per-batch path with decoding excluded: decoded frames (uint8) and labels (int32) wait in pinned host
                memory -> ``torch.stack`` into a pinned staging buffer (two, alternating) -> upload -> ``draw_jitter`` -> ``prepare_batch``
                -> ``Trainer.step``
  epoch_without_check  (b') the same epochs with ``check()`` once per window, not per epoch: the device never drains while the host
                draws the next epoch
  epoch_prefetch  (b'') as (b), ``check()`` per epoch, with ``EpochLoader(prefetch=True)``: the next epoch's host work is done at the end
                of the running one
  prep_launch   ms per launch of the indexed no-resize kernel at B = --batch on the store, next to the plain no-resize kernel on the
                same bytes gathered into a contiguous batch (windows alternated): ``launch_*`` are 256 copies of the record run by one
                library call (the device sets the pace), ``python_call_*`` are ``prepare_batch`` calls one by one (the Python caller
                sets it), the last of them from the full-size frames
  ingest        frames per second of ``resize_u8`` on device-resident chunks, and the wall time of building the whole store
  draws         host ms of ``draw_jitter_rows(N)`` against ``draw_jitter(N)``
Ratios (b)/(a) and (b)/(c) are in the ``summary`` line."""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robocupvision_amd.model as M                  # noqa: E402
from robocupvision_amd import _lib as L              # noqa: E402
from robocupvision_amd import data as D              # noqa: E402
from robocupvision_amd.train import Trainer          # noqa: E402


def windows(fn, units_per_call, min_seconds, repeats, warmup):
    """fn() enqueues `units_per_call` units of work; -> ms per unit (median, spread, min, max) over `repeats` windows >= min_seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    n = max(1, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / (n * units_per_call))
    return summarise(out, n)


def summarise(out, n):
    out = sorted(out)
    return {"ms": round(out[len(out) // 2], 5), "spread_ms": round(out[-1] - out[0], 5), "min_ms": round(out[0], 5), "max_ms": round(out[-1], 5),
            "calls_per_window": n, "repeats": len(out)}


def rate(row, images_per_unit):
    row["img_per_s"] = round(images_per_unit / (row["ms"] * 1e-3), 1)
    row["img_per_s_min"] = round(images_per_unit / (row["max_ms"] * 1e-3), 1)
    row["img_per_s_max"] = round(images_per_unit / (row["min_ms"] * 1e-3), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--size", type=int, nargs=2, default=(120, 160))
    ap.add_argument("--host-pool", type=int, default=256, help="decoded frames kept in pinned host memory for (c)")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_epoch.py measures on the GPU only: no HIP device here (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    N, B, src, size = a.frames, a.batch, tuple(a.src), tuple(a.size)
    rows_out = []

    def emit(what, row):
        row = dict({"what": what, "frames": N, "batch": B, "src": list(src), "size": list(size)}, **row)
        rows_out.append(row)
        print(json.dumps(row), flush=True)

    g = torch.Generator(device=dev).manual_seed(41)
    frames = torch.randint(0, 256, (N, src[0], src[1], 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 5, (N, src[0], src[1]), dtype=torch.uint8, device=dev, generator=g)
    torch.cuda.synchronize()

    # ---- ingest: resize_u8 on a device-resident chunk, and the whole store
    ing = windows(lambda: D.resize_u8(frames[:B], labels[:B], size), B, a.min_seconds, a.repeats, a.warmup)
    ing = {"resize_u8_" + k: v for k, v in ing.items()}
    ing["resize_u8_frames_per_s"] = round(1e3 / ing["resize_u8_ms"], 1)
    ing["resize_u8_source_GBps"] = round(src[0] * src[1] * 4 / (ing["resize_u8_ms"] * 1e-3) / 1e9, 1)
    t0 = time.perf_counter()
    store = D.ResidentDataset.from_tensors(frames, labels, size, chunk=B)
    torch.cuda.synchronize()
    ing["store_build_s"] = round(time.perf_counter() - t0, 4)
    ing["store_MB"] = round((store.frames.numel() + store.labels.numel() * store.labels.element_size()) / 1e6, 1)
    emit("ingest", ing)

    # ---- (c) needs decoded frames on the host; take them before the full-size frames leave the device
    P = min(a.host_pool, N)
    pool_f = [frames[i].cpu().pin_memory() for i in range(P)]
    pool_l = [labels[i].to(torch.int32).cpu().pin_memory() for i in range(P)]          # Image.convert("I") decodes to int32
    full_f, full_l = frames[:B].clone(), labels[:B].to(torch.int32)
    del frames, labels
    torch.cuda.empty_cache()

    # ---- the prep launch: indexed from the store / plain on the same bytes gathered / plain from the full-size frames
    random.seed(42)
    torch.manual_seed(42)
    rows = D.draw_jitter_rows(B).to(dev)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(43))[:B].to(dev)
    gat_f, gat_l = store.frames[idx].contiguous(), store.labels[idx].contiguous()
    xi, ti = D.prepare_batch(store.frames, store.labels, size, params=rows, index=idx, bad_index=store.bad_index)
    xp, tp = D.prepare_batch(gat_f, gat_l, size, params=rows)
    same = bool(torch.equal(xi, xp) and torch.equal(ti, tp))
    wi, wp = [], []
    for _ in range(a.repeats):          # alternate the two forms window by window
        r = windows(lambda: D.prepare_batch(store.frames, store.labels, size, params=rows, index=idx, bad_index=store.bad_index), 1,
                    a.min_seconds, 1, a.warmup)
        wi.append(r["ms"])
        n_calls = r["calls_per_window"]
        wp.append(windows(lambda: D.prepare_batch(gat_f, gat_l, size, params=rows), 1, a.min_seconds, 1, a.warmup)["ms"])
    ri, rp = summarise(wi, n_calls), summarise(wp, n_calls)
    full = windows(lambda: D.prepare_batch(full_f, full_l, size, params=rows), 1, a.min_seconds, a.repeats, a.warmup)
    # ... and the launches alone: 256 copies of each record run by ONE library call, so the device and not the Python caller sets the pace
    fx, kx, fy, ky, lx, ly = D._device_tables(size[0], size[1], size[0], size[1], dev)
    norm = D._device_norm(False, dev)
    common = dict(n=B, h=size[0], w=size[1], ho=size[0], wo=size[1], cin=kx, cout=ky, inmode2=store.labels.element_size(), aux0=1, aux1=0,
                  p_out=xi.data_ptr(), p_x0=ti.data_ptr(), p_x1=fx.data_ptr(), p_x2=fy.data_ptr(), p_x3=lx.data_ptr(), p_x4=ly.data_ptr(),
                  p_x5=norm.data_ptr(), p_in_c=rows.data_ptr())
    rec_i = L.make_op(L.OP_BATCH_PREP_IDX, count=N, inmode=idx.element_size(), p_in=store.frames.data_ptr(), p_in2=store.labels.data_ptr(),
                      p_in_aux=idx.data_ptr(), p_epi_aux=store.bad_index.data_ptr(), **common)
    rec_p = L.make_op(L.OP_BATCH_PREP, p_in=gat_f.data_ptr(), p_in2=gat_l.data_ptr(), **common)
    K = 256
    h = L.handle(dev.index)
    stream = torch.cuda.current_stream(dev).cuda_stream
    li, lp = L.OpList([rec_i] * K), L.OpList([rec_p] * K)
    ki, kp = [], []
    for _ in range(a.repeats):
        r = windows(lambda: li.run(h, stream), K, a.min_seconds, 1, a.warmup)
        ki.append(r["ms"])
        n_lists = r["calls_per_window"]
        kp.append(windows(lambda: lp.run(h, stream), K, a.min_seconds, 1, a.warmup)["ms"])
    ki, kp = summarise(ki, n_lists * K), summarise(kp, n_lists * K)
    nbytes = B * size[0] * size[1] * (3 + store.labels.element_size() + 12 + 8)
    diff, both = ki["ms"] - kp["ms"], max(ki["spread_ms"], kp["spread_ms"])
    emit("prep_launch", {"launch_indexed_no_resize": ki, "launch_plain_no_resize": kp, "launch_indexed_minus_plain_ms": round(diff, 5),
                         "launch_spread_of_the_two_ms": round(both, 5), "indexed_not_slower_beyond_spread": bool(diff <= both),
                         "launch_MB_moved": round(nbytes / 1e6, 2), "launch_indexed_TBps": round(nbytes / (ki["ms"] * 1e-3) / 1e12, 2),
                         "python_call_indexed_no_resize": ri, "python_call_plain_no_resize": rp, "python_call_plain_from_full_size": full,
                         "outputs_equal": same})

    # ---- (a) the step alone
    torch.manual_seed(12345678)
    tr = Trainer(M.ROBO_UNet().to(dev))
    step = rate(windows(lambda: tr.step(xi, ti), 1, a.min_seconds, a.repeats, a.warmup), B)
    emit("step", step)

    # ---- (b) whole epochs from the store
    loader = D.EpochLoader(store, B, train=True, generator=torch.Generator().manual_seed(44))

    def epoch():
        for x, t in loader:
            tr.step(x, t)
        store.check()
    per_epoch = len(loader) * B if N % B == 0 else N
    ep = rate(windows(epoch, 1, a.min_seconds, a.repeats, 1), per_epoch)
    ep["batches_per_epoch"] = len(loader)
    emit("epoch", ep)

    # ... and the same epochs with nothing synchronised between them (check() once per window): what the per-epoch host work -- the
    # permutation, draw_jitter_rows(N), two uploads -- costs when the device has drained before it starts
    def epoch_no_check():
        for x, t in loader:
            tr.step(x, t)
    ep_free = rate(windows(epoch_no_check, 1, a.min_seconds, a.repeats, 1), per_epoch)
    store.check()
    emit("epoch_without_check", ep_free)

    # ... and epochs checked one by one again, with the next epoch's host work done at the end of the running one (prefetch=True)
    loader_p = D.EpochLoader(store, B, train=True, generator=torch.Generator().manual_seed(44), prefetch=True)

    def epoch_prefetch():
        for x, t in loader_p:
            tr.step(x, t)
        store.check()
    ep_pre = rate(windows(epoch_prefetch, 1, a.min_seconds, a.repeats, 1), per_epoch)
    emit("epoch_prefetch", ep_pre)

    # ---- (c) upload every batch: pinned decoded frames -> stack -> upload -> draw_jitter -> prepare_batch -> step
    stage = [(torch.empty((B,) + tuple(pool_f[0].shape), dtype=torch.uint8).pin_memory(),
              torch.empty((B,) + tuple(pool_l[0].shape), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
    order = torch.randperm(P, generator=torch.Generator().manual_seed(45)).tolist()
    state = {"k": 0}

    def upload_batch():
        k = state["k"]
        state["k"] = k + 1
        sf, sl, ev = stage[k % 2]
        ev.synchronize()                                        # the copy that last read this staging buffer has finished
        pick = [order[(k * B + i) % P] for i in range(B)]
        torch.stack([pool_f[i] for i in pick], out=sf)
        torch.stack([pool_l[i] for i in pick], out=sl)
        f, lab = sf.to(dev, non_blocking=True), sl.to(dev, non_blocking=True)
        ev.record()
        x, t = D.prepare_batch(f, lab, size, params=D.draw_jitter(B))
        tr.step(x, t)
    up = rate(windows(upload_batch, 1, a.min_seconds, a.repeats, a.warmup), B)
    up["MB_uploaded_per_batch"] = round(B * src[0] * src[1] * (3 + 4) / 1e6, 1)
    emit("upload", up)

    # ---- the draws of an epoch on the host
    def host_ms(fn):
        random.seed(46)
        torch.manual_seed(46)
        t0 = time.perf_counter()
        fn(N)
        return round((time.perf_counter() - t0) * 1e3, 3)
    emit("draws", {"draw_jitter_rows_ms": sorted(host_ms(D.draw_jitter_rows) for _ in range(3))[1],
                   "draw_jitter_ms": sorted(host_ms(D.draw_jitter) for _ in range(3))[1], "rows": N})

    prep_share = ki["ms"] / (ki["ms"] + step["ms"])
    summary = {"epoch_over_step": round(ep["img_per_s"] / step["img_per_s"], 4), "epoch_over_upload": round(ep["img_per_s"] / up["img_per_s"], 3),
               "prep_launch_share_of_prep_plus_step": round(prep_share, 4),
               "epoch_ms_per_batch": round(ep["ms"] / len(loader), 5), "step_ms": step["ms"], "indexed_prep_launch_ms": ki["ms"],
               "epoch_ms_per_batch_minus_step_and_prep": round(ep["ms"] / len(loader) - step["ms"] - ki["ms"], 5),
               "epoch_without_check_over_step": round(ep_free["img_per_s"] / step["img_per_s"], 4),
               "epoch_without_check_ms_per_batch": round(ep_free["ms"] / len(loader), 5),
               "epoch_prefetch_over_step": round(ep_pre["img_per_s"] / step["img_per_s"], 4),
               "epoch_prefetch_ms_per_batch": round(ep_pre["ms"] / len(loader), 5)}
    emit("summary", summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows_out:
            f.write(json.dumps(row) + "\n")

    def cell(r):
        return "%.0f (%.0f .. %.0f)" % (r["img_per_s"], r["img_per_s_min"], r["img_per_s_max"])
    print("\n| path | images/s: median (slowest .. fastest window) | ms per batch |")
    print("|---|---|---|")
    print("| (a) `Trainer.step` alone, fixed tensors | %s | %.3f |" % (cell(step), step["ms"]))
    print("| (b) epochs through `EpochLoader`, `check()` after each | %s | %.3f |" % (cell(ep), ep["ms"] / len(loader)))
    print("| (b') the same, `check()` once per window | %s | %.3f |" % (cell(ep_free), ep_free["ms"] / len(loader)))
    print("| (b'') as (b) with `prefetch=True` | %s | %.3f |" % (cell(ep_pre), ep_pre["ms"] / len(loader)))
    print("| (c) pinned decoded frames -> stack -> upload -> `prepare_batch` -> step | %s | %.3f |" % (cell(up), up["ms"]))
    print("| (b) / (a) | %.3f | |" % summary["epoch_over_step"])
    print("| (b) / (c) | %.2f | |" % summary["epoch_over_upload"])
    print("\n| prep launch, B = %d | ms: median (spread) |" % B)
    print("|---|---|")
    print("| launch: indexed, no resize, from the store | %.4f (%.4f) |" % (ki["ms"], ki["spread_ms"]))
    print("| launch: plain, no resize, the same bytes gathered | %.4f (%.4f) |" % (kp["ms"], kp["spread_ms"]))
    print("| Python call: `prepare_batch(index=)`, no resize | %.4f (%.4f) |" % (ri["ms"], ri["spread_ms"]))
    print("| Python call: `prepare_batch`, no resize, gathered | %.4f (%.4f) |" % (rp["ms"], rp["spread_ms"]))
    print("| Python call: `prepare_batch` from the full-size frames | %.4f (%.4f) |" % (full["ms"], full["spread_ms"]))
    print("| `resize_u8` ingest | %.0f frames/s; store of %d built in %.2f s |" % (ing["resize_u8_frames_per_s"], N, ing["store_build_s"]))


if __name__ == "__main__":
    main()
