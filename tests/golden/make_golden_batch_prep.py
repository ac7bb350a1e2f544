"""Golden vectors of the batch preparation (dataset.py:107-133 ``SSYUVDataset.__getitem__`` with ``ColorJitter``, dataset.py:19-39, and
train.py:43-46 ``maskLabel``, transform.py:26-49).  Runs ONLY in the build container, where the reference and Pillow exist: it imports
the reference's ``dataset.py`` and ``transform.py`` and indexes the reference's ``SSYUVDataset`` over seeded frames written as PNGs, in
the style of ``make_golden_labelprop_train.py``.  Nothing of the reference's source text is stored: tensors and numbers only.

    python tests/golden/make_golden_batch_prep.py      # writes batch_prep.npz / batch_prep.json next to this script

``cv2``, ``skimage`` and ``progressbar`` are stubbed (imported at the top of those files, used by none of the code that runs here).
``torchvision`` is not installed; its three transforms that the class calls are stood in for below, each written as torchvision
documents it: ``Resize((h, w), interpolation)`` = ``Image.resize((w, h), interpolation)``, ``functional.to_tensor`` (uint8 HWC -> CHW
float32 ``div(255)``; mode ``I`` -> int32, not scaled) and ``Normalize`` (``sub_(mean).div_(std)`` per channel on a clone).

Per configuration (tests/batch_prep_restatement.py ``synthetic_frames``): the validation-mode item of every index, the training-mode
item under ``random.seed(seed); torch.manual_seed(seed)`` indexed in order, the values the reference drew while it did so (recorded by
wrapping ``torch.rand``, ``random.uniform`` and ``torch.einsum`` for the duration of the call: the flip draw, b_val, c_val and the 2x2
matrix), and the reference's ``maskLabel`` of the stacked validation labels for all 16 flag sets.  The two full-size configurations
store only the sha256 of the validation-mode batch.  A small tree of empty-named files records the class's listing per camera."""
import hashlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image
import PIL

REF = "/root/reference"
HERE = os.environ.get("GOLDEN_OUT") or os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import batch_prep_restatement as R      # noqa: E402  (tests/: the seeded frame generator the tests share)

# tag -> (B, (Hs, Ws), (H, W), frame seed, draw seed, finetune, labels hold every value 0..255)
CONFIGS = {
    "down4": (3, (96, 128), (24, 32), 11, 101, False, False),
    "down2": (2, (96, 128), (48, 64), 12, 102, True, False),
    "ident": (2, (24, 32), (24, 32), 13, 103, False, True),
    "ragged": (2, (97, 131), (40, 33), 14, 104, False, True),
}
FULL = {"full_120x160": (2, (480, 640), (120, 160), 21), "full_240x320": (2, (480, 640), (240, 320), 22)}
LISTING = ["img10.png", "img2.png", "img1.png", "a3.png", "img2b.png"]
LISTING_TXT = {"img10.png": "u", "img2.png": "b", "img1.png": "u", "a3.png": "b", "img2b.png": "x"}


class Resize:
    def __init__(self, size, interpolation=Image.BILINEAR):
        self.size, self.interpolation = size, interpolation

    def __call__(self, img):
        return img.resize((self.size[1], self.size[0]), self.interpolation)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        t = t.clone()
        mean = torch.as_tensor(self.mean, dtype=t.dtype)
        std = torch.as_tensor(self.std, dtype=t.dtype)
        return t.sub_(mean[:, None, None]).div_(std[:, None, None])


def to_tensor(pic):
    if pic.mode == "I":
        img = torch.from_numpy(np.array(pic, np.int32, copy=True))
    else:
        img = torch.from_numpy(np.array(pic, np.uint8, copy=True))
    img = img.view(pic.size[1], pic.size[0], len(pic.getbands())).permute((2, 0, 1)).contiguous()
    return img.to(torch.float32).div(255) if img.dtype == torch.uint8 else img


def install_stubs():
    for name in ("cv2", "skimage", "skimage.color", "progressbar"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.color"].rgb2yuv = None
    tv, tr, fn = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    fn.to_tensor = to_tensor
    tr.Resize, tr.Normalize, tr.functional = Resize, Normalize, fn
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"], sys.modules["torchvision.transforms.functional"] = tv, tr, fn


def write_tree(root, frames, labels, finetune):
    base = os.path.join(root, "FinetuneHorizon") if finetune else root
    for split in ("train", "val"):
        os.makedirs(os.path.join(base, split, "images"))
        os.makedirs(os.path.join(base, split, "labels"))
        for i in range(len(frames)):
            Image.fromarray(frames[i]).save(os.path.join(base, split, "images", "f%d.png" % i))
            Image.fromarray(labels[i].astype(np.uint8)).save(os.path.join(base, split, "labels", "f%d.png" % i))


class Recorder:
    """Passes torch.rand / random.uniform / torch.einsum through and keeps what went by."""

    def __enter__(self):
        self.rand, self.uniform, self.mtx = [], [], []
        self._rand, self._uniform, self._einsum = torch.rand, random.uniform, torch.einsum

        def rand(*a, **k):
            v = self._rand(*a, **k)
            self.rand.append(v.clone())
            return v

        def uniform(a, b):
            v = self._uniform(a, b)
            self.uniform.append(v)
            return v

        def einsum(eq, m, x):
            self.mtx.append(m.clone())
            return self._einsum(eq, m, x)
        torch.rand, random.uniform, torch.einsum = rand, uniform, einsum
        return self

    def __exit__(self, *exc):
        torch.rand, random.uniform, torch.einsum = self._rand, self._uniform, self._einsum


def batch_sha(imgs, targets):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(imgs, np.float32).tobytes())
    h.update(np.ascontiguousarray(targets, np.int64).tobytes())
    return h.hexdigest()


def val_items(ds_mod, root, size, finetune, B):
    ds = ds_mod.SSYUVDataset(root, img_size=size, train=False, finetune=finetune)
    assert len(ds) == B
    items = [ds[i] for i in range(B)]
    return torch.stack([i[0] for i in items]), torch.stack([i[1] for i in items])


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    install_stubs()
    import dataset as ds_mod          # the reference, imported (never copied)
    import transform as tr_mod
    out, meta = {}, {"pillow": PIL.__version__, "torch": torch.__version__, "configs": {}, "full": {}}
    for tag, (B, src, size, fseed, dseed, finetune, full_range) in CONFIGS.items():
        frames, labels = R.synthetic_frames(B, src[0], src[1], fseed, full_range_labels=full_range, cover_size=size)
        with tempfile.TemporaryDirectory() as td:
            write_tree(td, frames, labels, finetune)
            vi, vl = val_items(ds_mod, td, size, finetune, B)
            ds = ds_mod.SSYUVDataset(td, img_size=size, train=True, finetune=finetune)
            random.seed(dseed)
            torch.manual_seed(dseed)
            with Recorder() as rec:
                items = [ds[i] for i in range(B)]
        assert len(rec.rand) == B and len(rec.uniform) == 4 * B and len(rec.mtx) == B
        rows = np.zeros((B, 8), np.float32)
        for i in range(B):
            rows[i, 0] = 1.0 if rec.rand[i].item() > 0.5 else 0.0
            rows[i, 1:3] = torch.FloatTensor([rec.uniform[4 * i], rec.uniform[4 * i + 1]]).numpy()
            rows[i, 3:7] = rec.mtx[i].numpy().reshape(4)
        ti, tl = torch.stack([i[0] for i in items]), torch.stack([i[1] for i in items])
        assert vl.dtype == torch.int32 and int(vl.min()) >= 0 and int(vl.max()) <= 255
        masked = np.stack([tr_mod.maskLabel(vl.long().clone(), *flags).numpy() for flags in R.FLAG_SETS])
        assert masked.min() >= 0 and masked.max() <= 255
        out[tag + "/val_imgs"], out[tag + "/val_labels"] = vi.numpy(), vl.numpy().astype(np.uint8)
        out[tag + "/train_imgs"], out[tag + "/train_labels"] = ti.numpy(), tl.numpy().astype(np.uint8)
        out[tag + "/params"], out[tag + "/masked"] = rows, masked.astype(np.uint8)
        meta["configs"][tag] = {"B": B, "src": list(src), "size": list(size), "frame_seed": fseed, "draw_seed": dseed, "finetune": finetune,
                                "full_range_labels": full_range, "flips": [int(r) for r in rows[:, 0]],
                                "val_sha256": batch_sha(vi.numpy(), vl.long().numpy())}
        print(tag, "flips", meta["configs"][tag]["flips"], "val", tuple(vi.shape), "labels up to", int(vl.max()))
    for tag, (B, src, size, fseed) in FULL.items():
        frames, labels = R.synthetic_frames(B, src[0], src[1], fseed)
        with tempfile.TemporaryDirectory() as td:
            write_tree(td, frames, labels, False)
            vi, vl = val_items(ds_mod, td, size, False, B)
        meta["full"][tag] = {"B": B, "src": list(src), "size": list(size), "frame_seed": fseed, "val_sha256": batch_sha(vi.numpy(), vl.long().numpy())}
        print(tag, meta["full"][tag]["val_sha256"][:16])
    with tempfile.TemporaryDirectory() as td:          # the listing: natural order and the camera filter
        for split in ("train", "val"):
            os.makedirs(os.path.join(td, split, "images"))
            os.makedirs(os.path.join(td, split, "labels"))
            for name in LISTING:
                for sub in ("images", "labels"):
                    open(os.path.join(td, split, sub, name), "wb").close()
                with open(os.path.join(td, split, "images", name[:-4] + ".txt"), "w") as f:
                    f.write(LISTING_TXT[name])
        meta["listing"] = {"files": LISTING, "txt": LISTING_TXT,
                           "cameras": {cam: ds_mod.SSYUVDataset(td, train=True, camera=cam).images for cam in ("both", "top", "bottom")}}
        os.remove(os.path.join(td, "val", "images", LISTING[0][:-4] + ".txt"))          # a missing .txt switches the filter off
        meta["listing"]["val_without_one_txt"] = ds_mod.SSYUVDataset(td, train=False, camera="top").images
    np.savez_compressed(os.path.join(HERE, "batch_prep.npz"), **out)
    with open(os.path.join(HERE, "batch_prep.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
