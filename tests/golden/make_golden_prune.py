"""Golden vectors of the prune stage's mask builders (reference model.py:45-57 pruneModelNew, :621-642 pruneModel, :644-672
pruneModel2).  Runs ONLY where the reference exists: it imports the reference's ``model.py`` (pure PyTorch) and calls the three
functions on seeded CPU tensors, in the style of ``make_golden_bnn.py``.  Nothing from the reference's source text is stored: tensors
only.

    python tests/golden/make_golden_prune.py          # writes prune.npz next to this script

The tensor list is tests/prune_restatement.py SHAPES (seven tensors, 16 366 floats, one of them 1-D: no rule touches it).  Stored:
the weights ``w<k>``, and per run the weights afterwards and the returned masks: ``r0_*`` pruneModelNew(ratio 0.1), ``r1_*``
pruneModel(73, 77), ``r2_*`` pruneModel2(0.3, 300, 2000) and ``r2b_*`` a second round pruneModel2(0.38, 300, 2000) on the output of
the first (the zeros of round one are what topk re-selects first).  The values are tie free in magnitude and non-zero, so
torch.topk's answer is unique; in round two the only ties are the exact zeros, which are all selected.

pruneModel's loop need not end; a seed is taken only if the restatement's search ends on every tensor, and only if the restatement
reproduces the reference's masks exactly (param.std() of an fp32 CPU tensor against the float64 two-pass value: an observation, not
a law).  The first seed from 1 upward that passes is used and printed; no case had to be dropped.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.environ.get("GOLDEN_OUT") or os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prune_restatement as R  # noqa: E402


def tensors(arrs):
    return [torch.from_numpy(a.copy()) for a in arrs]


def run(fn, arrs, *args):
    ts = tensors(arrs)
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        masks = fn(ts, *args)
    return [t.numpy() for t in ts], [m.numpy() for m in masks]


def main():
    sys.path.insert(0, REF)
    import model as ref
    torch.set_num_threads(8)
    for seed in range(1, 65):
        rng = np.random.default_rng(seed)
        ws = [R.tie_free(rng, s) for s in R.SHAPES]
        big = [w for w in ws if w.ndim > 1]
        if any(R.rule1(w, R.LOWER, R.UPPER)[6] != R.ST_OK for w in big):
            continue
        out = {"seed": np.int64(seed)}
        for k, w in enumerate(ws):
            out["w%d" % k] = w
        runs = {"r0": (ref.pruneModelNew, ws, (R.RATIO0,)), "r1": (ref.pruneModel, ws, (R.LOWER, R.UPPER)),
                "r2": (ref.pruneModel2, ws, (R.RATIO2, R.LT, R.HT))}
        for tag, (fn, src, args) in runs.items():
            after, masks = run(fn, src, *args)
            for k, a in enumerate(after):
                out["%s_w%d" % (tag, k)] = a
            for j, m in enumerate(masks):
                out["%s_m%d" % (tag, j)] = m
        after2 = [out["r2_w%d" % k] for k in range(len(ws))]
        after, masks = run(ref.pruneModel2, after2, R.RATIO2B, R.LT, R.HT)
        for k, a in enumerate(after):
            out["r2b_w%d" % k] = a
        for j, m in enumerate(masks):
            out["r2b_m%d" % j] = m
        ok = all(np.array_equal(R.rule1(w, R.LOWER, R.UPPER)[1], out["r1_m%d" % j]) for j, w in enumerate(big))
        if not ok:
            print("seed %d: the reference's std differs from the float64 two-pass value on some tensor; next seed" % seed)
            continue
        np.savez_compressed(os.path.join(HERE, "prune.npz"), **out)
        print("prune.npz written, seed %d, %d arrays" % (seed, len(out)))
        return
    raise SystemExit("no seed passed")


if __name__ == "__main__":
    main()
