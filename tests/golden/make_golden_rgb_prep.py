#!/usr/bin/env python3
"""Goldens of the RGB batch preparation (RCV_OP_RGB_PREP, ``prepare_rgb_batch``): tests/golden/rgb_prep.npz + rgb_prep.json.

    python tests/golden/make_golden_rgb_prep.py

Steps 1-3 are made with Pillow's own calls (``Image.resize``, ``Image.transpose``, ``ImageEnhance.Brightness / Contrast / Color``,
``convert("HSV")`` / ``convert("RGB")``: what torchvision's PIL ColorJitter calls), step 4 with the float64 definition of
tests/rgb_prep_restatement.py (``to_yuv``), the labels with ``Image.resize(NEAREST)`` on mode ``I`` and ``mask_label``.  Needs Pillow
and numpy; the frames are the seeded synthetic ones of tests/batch_prep_restatement.py.  Per config: the parameter rows, the bytes
after step 3, the float32 output and the targets of training mode, the targets of validation mode, and a sha256 over outputs and targets of
each mode."""
import hashlib
import itertools
import json
import os
import random
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import rgb_prep_restatement as R  # noqa: E402
from robocupvision_amd import data as D  # noqa: E402

# tag -> B, source (Hs, Ws), output (H, W), seeds, maskLabel flag set (index into R.FLAG_SETS), label range
CONFIGS = {
    "perm24": dict(B=24, src=(33, 47), size=(16, 23), frame_seed=11, draw_seed=21, flags=0, full_range_labels=False),
    "ragged": dict(B=2, src=(97, 131), size=(40, 33), frame_seed=12, draw_seed=22, flags=5, full_range_labels=True),
    "ident": dict(B=2, src=(45, 67), size=(45, 67), frame_seed=13, draw_seed=23, flags=10, full_range_labels=True),
}


def sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def rows_for(tag, c):
    random.seed(c["draw_seed"])
    np.random.seed(c["draw_seed"])
    rows = D.draw_color_jitter(c["B"]).numpy()
    if tag == "perm24":          # one image per order of the four operations, both flips mixed
        for b, perm in enumerate(itertools.permutations(range(4))):
            rows[b, 2] = 4
            rows[b, 3:7] = perm
            rows[b, 0], rows[b, 1] = float(b & 1), float((b >> 1) & 1)
    return rows


def main():
    arrays, meta = {}, {"pillow": PIL.__version__, "configs": {}}
    for tag, c in CONFIGS.items():
        frames, labels = R.synthetic_frames(c["B"], c["src"][0], c["src"][1], c["frame_seed"], full_range_labels=c["full_range_labels"],
                                            cover_size=c["size"])
        rows = rows_for(tag, c)
        flags = R.FLAG_SETS[c["flags"]]
        tr = [R.pillow_image(frames[b], labels[b], c["size"], rows[b], flags) for b in range(c["B"])]
        va = [R.pillow_image(frames[b], labels[b], c["size"], None, flags) for b in range(c["B"])]
        ti, tt, tb = (np.stack([o[k] for o in tr]) for k in range(3))
        vi, vt, _ = (np.stack([o[k] for o in va]) for k in range(3))
        arrays[tag + "/params"] = rows
        arrays[tag + "/train_bytes"] = tb
        arrays[tag + "/train_imgs"] = ti
        arrays[tag + "/train_labels"] = tt.astype(np.int16)
        arrays[tag + "/val_labels"] = vt.astype(np.int16)
        meta["configs"][tag] = dict(c, train_sha256=sha(ti, tt), val_sha256=sha(vi, vt))
    # float32 outputs that differ between c = byte / 255.0 (the definition) and c = byte * (1 / 255.0), over all 2^24 colours
    total = colours = 0
    for hi in range(256):
        k = np.arange(1 << 16, dtype=np.uint32)
        rgb = np.stack([np.full_like(k, hi), (k >> 8) & 255, k & 255], -1).astype(np.uint8)
        d = R.to_yuv(rgb).view(np.uint32) != R.to_yuv(rgb, reciprocal=True).view(np.uint32)
        total += int(d.sum())
        colours += int(d.any(0).sum())
    meta["reciprocal_form"] = {"outputs_that_differ": total, "colours_that_differ": colours}
    # the listing of SSDataSet (dataset.py:135-164): natural order and the camera filter
    files = ["img10.png", "img2.png", "img1.png", "b_3.png", "a12x.png", "a2x.png"]
    txt = {"img10.png": "u", "img2.png": "b", "img1.png": "u", "b_3.png": "b", "a12x.png": "u", "a2x.png": "x"}
    order = ["a2x.png", "a12x.png", "b_3.png", "img1.png", "img2.png", "img10.png"]
    meta["listing"] = {"files": files, "txt": txt, "cameras": {"both": order, "top": [n for n in order if txt[n] == "u"],
                                                               "bottom": [n for n in order if txt[n] == "b"]}}
    np.savez_compressed(os.path.join(HERE, "rgb_prep.npz"), **arrays)
    with open(os.path.join(HERE, "rgb_prep.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote rgb_prep.npz (%d bytes), rgb_prep.json" % os.path.getsize(os.path.join(HERE, "rgb_prep.npz")))


if __name__ == "__main__":
    main()
