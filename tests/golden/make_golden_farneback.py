"""Writes tests/golden/farneback.json: what the numpy restatement of the optical-flow contract (tests/farneback_restatement.py) itself gives
on the seeded scenes of the tests, on the CPU.

  gpu_cases      per device case, e32 = the largest deviation of the restatement's float32 run from its float64 run (the device's bound is
                 8 x e32, tests/test_gpu_farneback.py), the largest |flow| and how many warps left the plane
  ground_truth   per (shape, shift): the median interior error against the known motion and the interior accuracy of the moved labels
  sequences      how many pixels of propagate_labels differ between the float32 and the float64 run (the test inputs must give 0)

    python tests/golden/make_golden_farneback.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import farneback_restatement as F  # noqa: E402

TWO_PLANE = [(120, 160), (64, 64), (66, 70)]
ONE_PLANE = [(48, 64), (33, 47)]
SHIFTS = [(3, -2), (1, 1), (-5, 4)]
INTERIOR = 12


def ground_truth_scene(H, W, d):
    """p, q, labels of p, labels of q for a whole-pixel shift d (seeded by shape and shift)."""
    rng = np.random.default_rng(H * 1000003 + W * 1009 + (d[0] + 16) * 37 + (d[1] + 16))
    margin = 8
    tex = np.rint(F.texture(rng, H, W, margin)).astype(np.uint8)
    lab = F.label_blobs(rng, H + 2 * margin, W + 2 * margin)
    p, q = F.crop_pair(tex, H, W, d, margin)
    lp, lq = F.crop_pair(lab, H, W, d, margin)
    return p, q, lp, lq


def ground_truth_figures(H, W, d, dtype=np.float64):
    p, q, lp, lq = ground_truth_scene(H, W, d)
    flow = F.farneback_flow(p, q, dtype=dtype)
    m = INTERIOR
    err = np.abs(flow - np.array(d, dtype=np.float32)[:, None, None]).max(0)[m:-m, m:-m]
    moved = F.update_labels(lq, flow)           # labels of the next frame pulled back to the previous one
    return float(np.median(err)), float((moved == lp)[m:-m, m:-m].mean())


def main():
    out = {"gpu_cases": {}, "ground_truth": {}, "sequences": {}}
    for name in F.GPU_CASES:
        p, q, params = F.gpu_case(name)
        e32, amax, oob = 0.0, 0.0, 0
        for b in range(p.shape[0]):
            stats = {}
            f64 = F.farneback_flow(p[b], q[b], dtype=np.float64, stats=stats, **params)
            f32 = F.farneback_flow(p[b], q[b], dtype=np.float32, **params)
            e32 = max(e32, float(np.abs(f64.astype(np.float64) - f32).max()))
            amax = max(amax, float(np.abs(f64).max()))
            oob += stats["oob"]
        out["gpu_cases"][name] = {"e32": e32, "max_abs_flow": amax, "warps_out_of_plane": oob}
        print(name, out["gpu_cases"][name])
    for shapes, shifts in ((TWO_PLANE, SHIFTS), (ONE_PLANE, [(1, 1)])):
        for H, W in shapes:
            for d in shifts:
                med, acc = ground_truth_figures(H, W, d)
                out["ground_truth"]["%dx%d_%d_%d" % (H, W, d[0], d[1])] = {"median_interior_error": med, "label_interior_accuracy": acc}
                print(H, W, d, med, acc)
    pred, gray = F.sequences()
    differ = 0
    for s in range(pred.shape[0]):
        differ += int((F.propagate_labels(pred[s], gray[s], dtype=np.float32) != F.propagate_labels(pred[s], gray[s])).sum())
    out["sequences"] = {"shape": list(pred.shape), "float32_vs_float64_pixels": differ}
    print(out["sequences"])
    with open(os.path.join(HERE, "farneback.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
