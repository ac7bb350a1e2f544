"""Training batches prepared on the device: the per-image work of the reference's loader (``SSYUVDataset.__getitem__``,
dataset.py:107-133), its ``ColorJitter`` (dataset.py:19-39) and the training loop's ``maskLabel`` (transform.py:26-49, train.py:43-46)
as ONE launch per batch (RCV_OP_BATCH_PREP, csrc/batch_prep.hip).

    ds = SSYUVDataset(root, img_size=(120, 160), train=True)            # decodes only: (uint8 [Hs,Ws,3], int32 [Hs,Ws]) per index
    frames, labels = ...                                                # stacked and uploaded as decoded
    imgs, targets = prepare_batch(frames, labels, (120, 160), params=draw_jitter(len(frames)))
    trainer.step(imgs, targets)

That form uploads every frame at its decoded size for every batch, every epoch.  The way to run EPOCHS is the resident form: the
dataset is decoded and resized ONCE (``resize_u8``, RCV_OP_RESIZE_U8: Pillow's resize ends in a uint8 and everything random comes after
it), the resized bytes stay on the device, and a batch is one launch that picks its images from the store by index
(``prepare_batch(..., index=)``, RCV_OP_BATCH_PREP_IDX) -- no upload, no host tensor work and no synchronisation per batch:

    store = ResidentDataset(ds, img_size=(120, 160), device="cuda")     # decode (<= 16 threads) -> upload in chunks -> resize_u8, once
    loader = EpochLoader(store, batch_size=64, train=True)              # one permutation + one draw_jitter_rows upload per epoch
    for epoch in range(epochs):
        for imgs, targets in loader:                                    # each: one prepare_batch(index=perm_dev[a:b], params=rows_dev[a:b])
            trainer.step(imgs, targets)
        store.check()                                                   # the one synchronisation: no index fell outside the store

Pinned: the stored bytes (to Pillow, byte for byte: tests/test_resident.py, tests/test_gpu_resident.py) and the batch (bit for bit
``prepare_batch`` of the full-size frames gathered by the same indices with the same rows).  The project's own definition: the epoch
order (``torch.randperm(N, generator=)`` on the host) and the sharding (``perm[rank::world]``) -- the order of the reference's
multi-worker ``DataLoader`` cannot be reproduced by any single process; row ``i`` of an epoch's draws belongs to the ``i``-th sample
visited, the order a single-process reference loader draws in.

The resize is Pillow's (8-bit BILINEAR frames, NEAREST mode-``I`` labels), restated as integer tables that are built here on the host
and cached on the device per (Hs, Ws, H, W); the restatement was compared with ``Image.resize`` of Pillow 12.2.0 byte for byte
(tests/test_batch_prep.py).  Random numbers and trigonometry stay on the host (``draw_jitter``): the kernel draws nothing.

The RGB loader of the older scripts (``SSDataSet`` with the transforms of trainer.py:75-123; the same chain in pruner.py,
labelPropTrain.py, tester.py, makeLPImages.py, classTrainer.py, classVal.py, objDetEval.py) is ``prepare_rgb_batch`` (RCV_OP_RGB_PREP,
csrc/rgb_prep.hip): ``Scale`` -> ``HorizontalFlip`` -> ``VerticalFlip`` -> torchvision's PIL ``ColorJitter`` -> ``rgb2yuv`` -> ``ToTensor`` ->
``Normalize([.5, 0, 0], [.5, .5, .5])``, with ``draw_color_jitter`` for the draws and ``SSDataSet`` for the listing.

    ds = SSDataSet(root, "train", camera="both")                        # decodes only
    imgs, targets = prepare_rgb_batch(frames, labels, scale=4, params=draw_color_jitter(len(frames)))

What of it is pinned and what is the project's definition:
  * pinned to Pillow 12.2.0, byte for byte (tests/test_rgb_prep.py): the resize, ``Image.blend`` and with it ``ImageEnhance.Brightness /
    Contrast / Color``, ``convert("L")``, and ``convert("HSV")`` / ``convert("RGB")`` of the hue shift;
  * stated, not pinned (neither torchvision nor skimage can be run next to this package): the order of the draws in
    ``draw_color_jitter`` (the ``random``-module ``ColorJitter.get_params`` the reference was written for), ``hue_shift =
    int(hue_factor * 255) & 255`` (``np.uint8(hue_factor * 255)`` added to the H plane with wrap-around), and step 4 -- ``rgb2yuv`` in
    float64 as ``c = byte / 255.0`` and the three products of a matrix row summed left to right, then ``Normalize`` and one rounding
    to float32 (skimage's BLAS order and its byte-to-float form are not pinned; DESIGN 4.10 has the count of float32 outputs the
    other byte-to-float form changes).

EPOCHS of that loader run from the same resident store, built at the SCALED size (``Scale`` is the first transform of every RGB list,
trainer.py:75-104, labelPropTrain.py:36-66; it ends in a uint8 and both flips and ``ColorJitter`` come after it, so the store holds exactly
the bytes the chain continues from): ``prepare_rgb_batch(..., index=)`` (RCV_OP_RGB_PREP_IDX) behind ``RGBEpochLoader``, and for LabelProp
``prepare_lp_pairs`` (RCV_OP_LP_PAIR_PREP) behind ``LPEpochLoader`` -- both frames of a pair with ONE ``draw_color_jitter`` row, Y only,
straight to the 8-channel input of labelPropTrain.py:162-193:

    store = ResidentDataset(SSDataSet(root, "train"), img_size=(120, 160))
    for imgs, targets in RGBEpochLoader(store, 32): ...                  # each: one prepare_rgb_batch(index=, params=)
    lp = LPDataSet(root, train=True)                                    # the listing of dataset.py:191-228
    store = ResidentDataset(lp.frames, img_size=(120, 160))
    for inputs, targets in LPEpochLoader(store, lp.windows, 8): ...      # each: one prepare_lp_pairs

Not covered (it keeps raising): ``LPDataSet.__getitem__`` (cv2 ``cvtColor``; labelPropTrain.py does not use it)."""
from __future__ import annotations

import math
import os
import os.path as osp
import random
import re

import numpy as np
import torch

from . import _lib as L

__all__ = ["prepare_batch", "prepare_frames", "draw_jitter", "SSYUVDataset", "bilinear_table", "nearest_table", "norm_table",
           "prepare_rgb_batch", "draw_color_jitter", "SSDataSet", "resize_u8", "draw_jitter_rows", "ResidentDataset", "EpochLoader", "prepare_lp_pairs", "draw_color_jitter_rows", "RGBEpochLoader",
           "LPDataSet", "LPEpochLoader"]

PRECISION_BITS = 22          # Pillow's 8-bit resampling: 32 - 8 - 2
MEAN = {False: [0.36269532, 0.41144562, 0.282713], True: [0.34190056, 0.4833289, 0.48565758]}      # dataset.py:74 (key: finetune)
STD = {False: [0.31111388, 0.21010718, 0.34060917], True: [0.47421749, 0.13846053, 0.1714848]}     # dataset.py:75


def bilinear_table(in_size: int, out_size: int) -> np.ndarray:
    """int32 [out_size][2 + K] rows {first tap, tap count, K coefficients}: Pillow's precompute_coeffs (double) and
    normalize_coeffs_8bpc (22-bit integers, rounded half away from zero) for the BILINEAR filter; K = ceil(max(in / out, 1)) * 2 + 1.
    Equal sizes give the one-tap rows {i, 1, 2^22}: the byte comes back unchanged, as from the pass Pillow skips."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    tab = np.zeros((out_size, 2 + ksize), np.int32)
    if in_size == out_size:
        tab[:, 0] = np.arange(out_size)
        tab[:, 1] = 1
        tab[:, 2] = 1 << PRECISION_BITS
        return tab
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        tab[xx, 0], tab[xx, 1] = xmin, n
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            tab[xx, 2 + x] = int(0.5 + v * (1 << PRECISION_BITS))          # (bilinear weights are never negative)
    return tab


def nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """int32 [out_size]: the source index of Pillow's NEAREST resize, ``xo = a0 * 0.5; tab[x] = int(xo); xo += a0`` in double."""
    a0 = float(in_size) / out_size
    tab = np.zeros(out_size, np.int32)
    xo = a0 * 0.5
    for x in range(out_size):
        tab[x] = min(int(xo), in_size - 1)
        xo += a0
    return tab


def norm_table(finetune: bool = False) -> torch.Tensor:
    """float32 [3][256]: ``to_tensor`` + ``Normalize(mean, std)`` of every byte value per channel, made with the same torch calls
    (uint8 -> float32, ``div(255)``, ``sub(mean)``, ``div(std)``), so a lookup equals them bit for bit."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN[bool(finetune)], dtype=torch.float32)
    std = torch.as_tensor(STD[bool(finetune)], dtype=torch.float32)
    return ((v[None, :] - mean[:, None]) / std[:, None]).contiguous()


_tables = {}          # (Hs, Ws, H, W, device) -> (frame_x, kx, frame_y, ky, label_x, label_y) on the device
_norms = {}           # (finetune, device) -> float32 [3][256] on the device


def _device_tables(Hs, Ws, H, W, dev):
    key = (Hs, Ws, H, W, str(dev))
    t = _tables.get(key)
    if t is None:
        fx, fy = bilinear_table(Ws, W), bilinear_table(Hs, H)
        t = (torch.from_numpy(fx).to(dev), fx.shape[1] - 2, torch.from_numpy(fy).to(dev), fy.shape[1] - 2,
             torch.from_numpy(nearest_table(Ws, W)).to(dev), torch.from_numpy(nearest_table(Hs, H)).to(dev))
        _tables[key] = t
    return t


def _device_norm(finetune, dev):
    key = (bool(finetune), str(dev))
    t = _norms.get(key)
    if t is None:
        t = _norms[key] = norm_table(finetune).to(dev)
    return t


_bad_counters = {}    # device -> int32 [1] on the device: images whose index fell outside the store (prepare_batch(index=) without bad_index=)


def _handle(dev):
    """The library handle of the HIP device ``dev`` (a ``torch.device``; without an index: the current one)."""
    return L.handle(dev.index if dev.index is not None else torch.cuda.current_device())


def prepare_batch(frames, labels, img_size=(120, 160), finetune=False, train=True, params=None, no_ball=False, no_robot=False,
                  no_goal=False, no_line=False, index=None, bad_index=None):
    """``frames`` uint8 [B,Hs,Ws,3] (decoded RGB) and ``labels`` uint8 or int32 [B,Hs,Ws], both on the HIP device -> ``(imgs, targets)``:
    float32 [B,3,H,W] and int64 [B,H,W], what ``Trainer.step`` / ``Trainer.evaluate`` take.  One launch.

    ``train=True`` needs ``params``, the float32 [B,8] rows of ``draw_jitter`` (host or device): flip, then ``(y + b) * c`` and the 2x2
    U/V matrix.  ``train=False`` is the validation loader: resize, normalise, maskLabel.  ``no_ball .. no_line`` are ``maskLabel``'s
    nb, nr, ng, nl.  Exact where the reference's arithmetic is (everything but U/V, which are within 2^-23 (|m0 U| + |m1 V|) of exact,
    as the reference's einsum is).

    ``index`` (int32 or int64 [B], on the device): ``frames`` / ``labels`` are then a STORE of N images and image ``b`` of the batch is
    ``store[index[b]]``; ``B = len(index)`` and ``params`` is [B,8] (RCV_OP_BATCH_PREP_IDX).  The result is bit for bit that of the call
    without ``index`` on ``frames[index]``, ``labels[index]``.  An index outside [0, N) reads nothing: that image comes back as zeros
    with targets 0, and ``bad_index`` (int32 [1] on the device; one per device is kept here if none is given) is incremented -- by the
    kernel, with nothing synchronised; ``ResidentDataset.check`` reads it.  Without ``index`` the call is what it always was.

    Stated difference: when exactly one of ``H == Hs``, ``W == Ws`` holds the reference skips the resize altogether
    (dataset.py:118-121 joins the two comparisons with ``and``) and hands the network a frame of the wrong size; here that raises."""
    if not (torch.is_tensor(frames) and torch.is_tensor(labels)):
        raise TypeError("prepare_batch: frames and labels must be tensors")
    if frames.dtype != torch.uint8 or labels.dtype not in (torch.uint8, torch.int32):
        raise TypeError("prepare_batch: frames must be uint8 and labels uint8 or int32 (got %s, %s)" % (frames.dtype, labels.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or labels.dim() != 3:
        raise ValueError("prepare_batch: frames must be [B,Hs,Ws,3] and labels [B,Hs,Ws] (got %s, %s)" % (tuple(frames.shape), tuple(labels.shape)))
    B, Hs, Ws, _ = frames.shape
    H, W = int(img_size[0]), int(img_size[1])
    if tuple(labels.shape) != (B, Hs, Ws) or B < 1 or Hs < 1 or Ws < 1 or H < 1 or W < 1:
        raise ValueError("prepare_batch: labels %s do not match frames %s (or an empty size)" % (tuple(labels.shape), tuple(frames.shape)))
    if (H == Hs) != (W == Ws):
        raise ValueError("prepare_batch: %d x %d -> %d x %d keeps exactly one axis: the reference skips the resize of such a frame altogether "
                         "(dataset.py:118-121 tests `h != Hs and w != Ws`) and feeds the network the wrong size; resize the frames first"
                         % (Hs, Ws, H, W))
    if frames.device.type != "cuda" or labels.device != frames.device:
        raise L.RcvError("prepare_batch runs on the HIP device only (frames on %s, labels on %s)" % (frames.device, labels.device))
    if not (frames.is_contiguous() and labels.is_contiguous()):
        raise ValueError("prepare_batch: frames and labels must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    N = B
    if index is not None:
        _check_index("prepare_batch", index, 1)
        bad_index = _index_args("prepare_batch", index, bad_index, dev, 1)
        B = int(index.shape[0])
    if train:
        if params is None:
            raise ValueError("prepare_batch: train=True needs params (draw_jitter(B))")
        if not torch.is_tensor(params) or params.dtype != torch.float32 or tuple(params.shape) != (B, 8):
            raise TypeError("prepare_batch: params must be a float32 [B,8] tensor (draw_jitter)")
        params = params.to(dev).contiguous()
    fx, kx, fy, ky, lx, ly = _device_tables(Hs, Ws, H, W, dev)
    norm = _device_norm(finetune, dev)
    imgs = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    targets = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    mask = (1 if no_ball else 0) | (2 if no_robot else 0) | (4 if no_goal else 0) | (8 if no_line else 0)
    h = _handle(dev)
    if index is not None:
        L.check(L.load().rcv_batch_prep_indexed(h, frames.data_ptr(), labels.data_ptr(), labels.element_size(), N, index.data_ptr(),
                                                index.element_size(), B, Hs, Ws, H, W, fx.data_ptr(), kx, fy.data_ptr(), ky, lx.data_ptr(),
                                                ly.data_ptr(), norm.data_ptr(), params.data_ptr() if train else None, 1 if train else 0,
                                                mask, imgs.data_ptr(), targets.data_ptr(), bad_index.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "rcv_batch_prep_indexed")
        return imgs, targets
    L.check(L.load().rcv_batch_prep(h, frames.data_ptr(), labels.data_ptr(), labels.element_size(), B, Hs, Ws, H, W, fx.data_ptr(), kx,
                                    fy.data_ptr(), ky, lx.data_ptr(), ly.data_ptr(), norm.data_ptr(),
                                    params.data_ptr() if train else None, 1 if train else 0, mask, imgs.data_ptr(), targets.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream), "rcv_batch_prep")
    return imgs, targets


def prepare_frames(frames, img_size=(120, 160), finetune=False):
    """``frames`` uint8 [B,Hs,Ws,3] (decoded RGB) on the HIP device -> float32 [B,3,H,W]: the validation loader's resize and
    normalisation for frames that have no labels (detect.py:125-130), one launch (RCV_OP_FRAME_PREP).  Bit for bit the ``imgs`` of
    ``prepare_batch(frames, labels, img_size, finetune, train=False)``; the same refusals, the one-axis-kept size among them."""
    if not torch.is_tensor(frames):
        raise TypeError("prepare_frames: frames must be a tensor")
    if frames.dtype != torch.uint8:
        raise TypeError("prepare_frames: frames must be uint8 (got %s)" % frames.dtype)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("prepare_frames: frames must be [B,Hs,Ws,3] (got %s)" % (tuple(frames.shape),))
    B, Hs, Ws, _ = frames.shape
    H, W = int(img_size[0]), int(img_size[1])
    if B < 1 or Hs < 1 or Ws < 1 or H < 1 or W < 1:
        raise ValueError("prepare_frames: frames %s -> %d x %d: an empty size" % (tuple(frames.shape), H, W))
    if (H == Hs) != (W == Ws):
        raise ValueError("prepare_frames: %d x %d -> %d x %d keeps exactly one axis: the reference skips the resize of such a frame altogether "
                         "(dataset.py:118-121 tests `h != Hs and w != Ws`) and feeds the network the wrong size; resize the frames first"
                         % (Hs, Ws, H, W))
    if frames.device.type != "cuda":
        raise L.RcvError("prepare_frames runs on the HIP device only (frames on %s)" % frames.device)
    if not frames.is_contiguous():
        raise ValueError("prepare_frames: frames must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    fx, kx, fy, ky, _, _ = _device_tables(Hs, Ws, H, W, dev)
    norm = _device_norm(finetune, dev)
    imgs = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    h = _handle(dev)
    L.check(L.load().rcv_frame_prep(h, frames.data_ptr(), B, Hs, Ws, H, W, fx.data_ptr(), kx, fy.data_ptr(), ky, norm.data_ptr(),
                                    imgs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rcv_frame_prep")
    return imgs


def resize_u8(frames, labels=None, img_size=(120, 160), label_dtype=torch.uint8):
    """``frames`` uint8 [B,Hs,Ws,3] and ``labels`` uint8 or int32 [B,Hs,Ws] (or None), on the HIP device -> ``(bytes, labels_out)``:
    uint8 [B,H,W,3] and ``label_dtype`` (uint8 or int32) [B,H,W] (None without labels).  The resize stage of ``prepare_batch`` alone, one
    launch (RCV_OP_RESIZE_U8): ``bytes`` are what ``Image.fromarray(f).resize((W, H), BILINEAR)`` holds and ``labels_out`` what the
    mode-``I`` label's ``resize((W, H), NEAREST)`` holds, byte for byte -- gathered, not masked.  ``prepare_batch`` of them at their own
    size equals ``prepare_batch`` of the full-size frames bit for bit.  ``label_dtype=torch.uint8`` keeps the low byte of an int32
    label: the caller has seen that every value is <= 255 (``ResidentDataset`` checks it on the host array).  ``H == Hs and W == Ws``
    copies.  Same refusals as ``prepare_batch``."""
    if not torch.is_tensor(frames) or (labels is not None and not torch.is_tensor(labels)):
        raise TypeError("resize_u8: frames (and labels) must be tensors")
    if frames.dtype != torch.uint8 or (labels is not None and labels.dtype not in (torch.uint8, torch.int32)):
        raise TypeError("resize_u8: frames must be uint8 and labels uint8 or int32 (got %s, %s)"
                        % (frames.dtype, None if labels is None else labels.dtype))
    if label_dtype not in (torch.uint8, torch.int32):
        raise TypeError("resize_u8: label_dtype must be torch.uint8 or torch.int32 (got %s)" % (label_dtype,))
    if frames.dim() != 4 or frames.shape[3] != 3 or (labels is not None and labels.dim() != 3):
        raise ValueError("resize_u8: frames must be [B,Hs,Ws,3] and labels [B,Hs,Ws] (got %s, %s)"
                         % (tuple(frames.shape), None if labels is None else tuple(labels.shape)))
    B, Hs, Ws, _ = frames.shape
    H, W = int(img_size[0]), int(img_size[1])
    if (labels is not None and tuple(labels.shape) != (B, Hs, Ws)) or B < 1 or Hs < 1 or Ws < 1 or H < 1 or W < 1:
        raise ValueError("resize_u8: labels %s do not match frames %s (or an empty size)"
                         % (None if labels is None else tuple(labels.shape), tuple(frames.shape)))
    if (H == Hs) != (W == Ws):
        raise ValueError("resize_u8: %d x %d -> %d x %d keeps exactly one axis: the reference skips the resize of such a frame altogether "
                         "(dataset.py:118-121 tests `h != Hs and w != Ws`) and feeds the network the wrong size; resize the frames first"
                         % (Hs, Ws, H, W))
    if frames.device.type != "cuda" or (labels is not None and labels.device != frames.device):
        raise L.RcvError("resize_u8 runs on the HIP device only (frames on %s, labels on %s)"
                         % (frames.device, None if labels is None else labels.device))
    if not (frames.is_contiguous() and (labels is None or labels.is_contiguous())):
        raise ValueError("resize_u8: frames and labels must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    fx, kx, fy, ky, lx, ly = _device_tables(Hs, Ws, H, W, dev)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    lab_out = None if labels is None else torch.empty(B, H, W, dtype=label_dtype, device=dev)
    h = _handle(dev)
    L.check(L.load().rcv_resize_u8(h, frames.data_ptr(), None if labels is None else labels.data_ptr(),
                                   0 if labels is None else labels.element_size(), B, Hs, Ws, H, W, fx.data_ptr(), kx, fy.data_ptr(), ky,
                                   lx.data_ptr(), ly.data_ptr(), out.data_ptr(), None if lab_out is None else lab_out.data_ptr(),
                                   0 if lab_out is None else lab_out.element_size(), torch.cuda.current_stream(dev).cuda_stream),
            "rcv_resize_u8")
    return out, lab_out


def draw_jitter_rows(n, b=0.3, c=0.3, s=0.3, h=3.1415 / 6):
    """The rows of ``draw_jitter(n)`` for a whole epoch in one call: bit for bit the same float32 [n,8] host tensor under the same
    ``random`` / ``torch`` seeds, and both generators are left where ``draw_jitter(n)`` leaves them.  The draws are the same ones in
    the same order on each generator (``torch.rand(n)`` is the ``n`` single draws of the CPU generator; the four ``random.uniform`` per
    image); the rounding to float32 is one array conversion, not three tensor constructions per image.  cos / sin stay numpy's SCALAR
    calls on the Python float, as in ``draw_jitter``: a vectorised call may take another code path of numpy and need not round alike."""
    p = torch.rand(n) if n else torch.zeros(0)
    u = random.uniform
    d = np.array([(u(-b, b), u(1 - c, 1 + c), u(1 - s, 1 + s), u(-h, h)) for _ in range(n)], np.float64).reshape(n, 4)
    hv = d[:, 3].tolist()
    cos = np.array([np.cos(v) for v in hv], np.float64)
    sin = np.array([np.sin(v) for v in hv], np.float64)
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0] = (p > 0.5).numpy()
    rows[:, 1], rows[:, 2] = d[:, 0], d[:, 1]
    rows[:, 3] = rows[:, 6] = d[:, 2] * cos
    rows[:, 4], rows[:, 5] = -sin, sin
    rows[:, 7] = 0.0 if (s > 0 and h > 0) else 1.0
    return torch.from_numpy(rows)


def draw_jitter(B, b=0.3, c=0.3, s=0.3, h=3.1415 / 6):
    """The random draws of ``B`` consecutive ``SSYUVDataset.__getitem__`` calls in training mode, in the reference's order: per image
    ``torch.rand(1).item()`` (flip iff > 0.5, dataset.py:127-128), then the four ``random.uniform`` draws of ``ColorJitter.__call__``
    (dataset.py:28-31).  Returns the host tensor float32 [B,8] = {flip, b_val, c_val, m00, m01, m10, m11, uv_off}; the matrix is built in
    float64 with numpy's cos / sin and rounded through ``torch.FloatTensor`` as dataset.py:33 does (the off-diagonal -sin / +sin are not
    scaled by s_val, as there).  uv_off = 1 when ``s > 0 and h > 0`` is false (dataset.py:36); the four values are drawn all the same."""
    rows = torch.zeros(B, 8, dtype=torch.float32)
    for i in range(B):
        p = torch.rand(1).item()
        b_val = random.uniform(-b, b)
        c_val = random.uniform(1 - c, 1 + c)
        s_val = random.uniform(1 - s, 1 + s)
        h_val = random.uniform(-h, h)
        mtx = torch.FloatTensor([[s_val * np.cos(h_val), -np.sin(h_val)], [np.sin(h_val), s_val * np.cos(h_val)]])
        rows[i, 0] = 1.0 if p > 0.5 else 0.0
        rows[i, 1:3] = torch.FloatTensor([b_val, c_val])
        rows[i, 3:7] = mtx.reshape(4)
        rows[i, 7] = 0.0 if (s > 0 and h > 0) else 1.0
    return rows


OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3          # op codes of a draw_color_jitter row
_workspaces = {}          # (device, bytes) -> uint32 partial sums of the statistics launch (reused: every call overwrites what it reads)


def _check_color_rows(rows, who):
    """The host check of ``draw_color_jitter`` rows (numpy [n,12]): codes 0..3, each at most once.  Returns bool [n]: the row holds a
    contrast among its operations."""
    n, ops = rows[:, 2], rows[:, 3:7]
    used = np.arange(4)[None, :] < n[:, None]
    ok = (n == np.floor(n)) & (n >= 0) & (n <= 4) & (~used | ((ops == np.floor(ops)) & (ops >= 0) & (ops <= 3))).all(1)
    for code in range(4):
        ok &= (used & (ops == code)).sum(1) <= 1
    if not ok.all():
        b = int(np.argmin(ok))
        raise ValueError("%s: row %d: n_ops %r with operations %r (codes 0..3, each at most once)"
                         % (who, b, float(n[b]), [float(v) for v in ops[b]]))
    return (used & (ops == OP_CONTRAST)).any(1)


def _check_index(who, index, dim):
    """The check ``prepare_batch`` makes of the form of ``index``; ``dim`` 1: [B], 2: pairs [B,2]."""
    if not torch.is_tensor(index) or index.dtype not in (torch.int32, torch.int64) or index.dim() != dim or index.shape[0] < 1 \
            or (dim == 2 and index.shape[1] != 2):
        raise TypeError("%s: %s must be a non-empty int32 or int64 %s tensor" % ((who,) + (("index", "[B]") if dim == 1 else ("pairs", "[B,2]"))))


def _index_args(who, index, bad_index, dev, dim):
    """The checks ``prepare_batch`` makes of where ``index`` lives and of ``bad_index``.  Returns the counter."""
    if index.device != dev or not index.is_contiguous():
        raise ValueError("%s: %s must be contiguous and on the device of the store (%s; got %s)"
                         % (who, "index" if dim == 1 else "pairs", dev, index.device))
    if bad_index is None:
        bad_index = _bad_counters.get(str(dev))
        if bad_index is None:
            bad_index = _bad_counters[str(dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
    elif not torch.is_tensor(bad_index) or bad_index.dtype != torch.int32 or bad_index.numel() < 1 or bad_index.device != dev:
        raise TypeError("%s: bad_index must be an int32 tensor on the device of the store" % who)
    return bad_index


def _workspace(dev, need):
    if not need:
        return None
    ws = _workspaces.get((str(dev), need))
    if ws is None:
        ws = _workspaces[(str(dev), need)] = torch.empty(need // 4, dtype=torch.int32, device=dev)
    return ws


def prepare_rgb_batch(frames, labels=None, scale=4, train=True, params=None, no_ball=False, no_robot=False, no_goal=False, no_line=False,
                      img_size=None, index=None, bad_index=None, contrast=None):
    """``frames`` uint8 [B,Hs,Ws,3] (decoded RGB) and ``labels`` uint8 or int32 [B,Hs,Ws] or None, on the HIP device -> ``(imgs,
    targets)``: float32 YUV [B,3,H,W] and int64 [B,H,W] (None without labels: the patch chain of classTrainer.py / objDetEval.py).
    ``H = int(Hs / scale)``, ``W = int(Ws / scale)`` as transform.py:8-19 ``Scale``; ``scale == 1`` means no resize.  ``img_size=(H, W)``
    in place of ``scale`` names any output size the tables allow (no axis shrinks by more than 8).

    ``train=True`` needs ``params``, the float32 [B,12] rows of ``draw_color_jitter`` (host or device): the two flips, then up to four
    operations on the uint8 pixel in the row's order, exactly as Pillow computes them.  ``train=False`` is the validation chain:
    resize, YUV, normalise, maskLabel -- the same as training mode with no flip and ``n_ops = 0``.  Rows given on the host are checked
    (codes 0..3, each at most once) and the statistics launch is skipped when none of them holds a contrast; rows given on the device
    are taken as they are.  Every output element is exact to the contract of the module docstring.  Same refusals as
    ``prepare_batch``.

    ``index`` (int32 or int64 [B], on the device): ``frames`` / ``labels`` are then a STORE of N images and image ``b`` of the batch is
    ``store[index[b]]``; ``B = len(index)`` and ``params`` is [B,12] (RCV_OP_RGB_PREP_IDX).  The result is bit for bit that of the call
    without ``index`` on ``frames[index]``, ``labels[index]``.  An index outside [0, N) reads nothing in either launch: that image comes
    back as zeros with targets 0 and ``bad_index`` (int32 [1] on the device; one per device is kept here if none is given) is
    incremented by the kernel, with nothing synchronised.  Without ``index`` the call is what it always was.

    ``contrast`` (None, or a bool for rows given on the DEVICE, which cannot be looked at without a synchronisation): the caller's word
    on whether any of these rows holds a contrast -- ``RGBEpochLoader`` checked the epoch's rows once on the host and knows it per
    slice.  False skips the statistics launch (a row that holds one anyway blends towards 0, rcv.h i[COUNT])."""
    if not torch.is_tensor(frames) or (labels is not None and not torch.is_tensor(labels)):
        raise TypeError("prepare_rgb_batch: frames (and labels) must be tensors")
    if frames.dtype != torch.uint8 or (labels is not None and labels.dtype not in (torch.uint8, torch.int32)):
        raise TypeError("prepare_rgb_batch: frames must be uint8 and labels uint8 or int32 (got %s, %s)"
                        % (frames.dtype, None if labels is None else labels.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or (labels is not None and labels.dim() != 3):
        raise ValueError("prepare_rgb_batch: frames must be [B,Hs,Ws,3] and labels [B,Hs,Ws] (got %s, %s)"
                         % (tuple(frames.shape), None if labels is None else tuple(labels.shape)))
    B, Hs, Ws, _ = frames.shape
    N = B
    if index is not None:
        _check_index("prepare_rgb_batch", index, 1)
    if not scale >= 1:
        raise ValueError("prepare_rgb_batch: scale %r must be >= 1" % (scale,))
    H, W = (Hs, Ws) if scale == 1 else (int(Hs / scale), int(Ws / scale))
    if img_size is not None:
        H, W = int(img_size[0]), int(img_size[1])
    if (labels is not None and tuple(labels.shape) != (B, Hs, Ws)) or B < 1 or Hs < 1 or Ws < 1 or H < 1 or W < 1:
        raise ValueError("prepare_rgb_batch: labels %s do not match frames %s (or an empty size)"
                         % (None if labels is None else tuple(labels.shape), tuple(frames.shape)))
    if (H == Hs) != (W == Ws):
        raise ValueError("prepare_rgb_batch: %d x %d -> %d x %d keeps exactly one axis; resize the frames first" % (Hs, Ws, H, W))
    if index is not None:
        B = int(index.shape[0])
    stats = 0
    if train:
        if params is None:
            raise ValueError("prepare_rgb_batch: train=True needs params (draw_color_jitter(B))")
        if not torch.is_tensor(params) or params.dtype != torch.float32 or tuple(params.shape) != (B, 12):
            raise TypeError("prepare_rgb_batch: params must be a float32 [B,12] tensor (draw_color_jitter)")
        stats = 1
        if params.device.type == "cpu":
            stats = int(_check_color_rows(params.numpy(), "prepare_rgb_batch").any())
        elif contrast is not None:
            stats = 1 if contrast else 0
    if frames.device.type != "cuda" or (labels is not None and labels.device != frames.device):
        raise L.RcvError("prepare_rgb_batch runs on the HIP device only (frames on %s, labels on %s)"
                         % (frames.device, None if labels is None else labels.device))
    if not (frames.is_contiguous() and (labels is None or labels.is_contiguous())):
        raise ValueError("prepare_rgb_batch: frames and labels must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    if index is not None:
        bad_index = _index_args("prepare_rgb_batch", index, bad_index, dev, 1)
    if train:
        params = params.to(dev).contiguous()
    fx, kx, fy, ky, lx, ly = _device_tables(Hs, Ws, H, W, dev)
    imgs = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    targets = None if labels is None else torch.empty(B, H, W, dtype=torch.int64, device=dev)
    mask = (1 if no_ball else 0) | (2 if no_robot else 0) | (4 if no_goal else 0) | (8 if no_line else 0)
    h = _handle(dev)
    lab_bytes = 0 if labels is None else labels.element_size()
    if index is not None:
        op = L.make_op(L.OP_RGB_PREP_IDX, n=B, stride=N, inmode=index.element_size(), h=Hs, w=Ws, ho=H, wo=W, cin=kx, cout=ky, inmode2=lab_bytes,
                       aux0=1 if train else 0, aux1=mask, count=stats, p_x1=fx.data_ptr(), p_x2=fy.data_ptr(), p_x3=lx.data_ptr(),
                       p_x4=ly.data_ptr(), p_in_aux=index.data_ptr(), p_epi_aux=bad_index.data_ptr())
        need = L.op_workspace(h, op)
        ws = _workspace(dev, need)
        L.check(L.load().rcv_rgb_prep_indexed(h, frames.data_ptr(), None if labels is None else labels.data_ptr(), lab_bytes, N, index.data_ptr(),
                                              index.element_size(), B, Hs, Ws, H, W, fx.data_ptr(), kx, fy.data_ptr(), ky, lx.data_ptr(),
                                              ly.data_ptr(), params.data_ptr() if train else None, 1 if train else 0, stats, mask,
                                              imgs.data_ptr(), None if targets is None else targets.data_ptr(), bad_index.data_ptr(),
                                              None if ws is None else ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
                "rcv_rgb_prep_indexed")
        return imgs, targets
    op = L.make_op(L.OP_RGB_PREP, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=kx, cout=ky, inmode2=lab_bytes, aux0=1 if train else 0, aux1=mask,
                   count=stats, p_x1=fx.data_ptr(), p_x2=fy.data_ptr(), p_x3=lx.data_ptr(), p_x4=ly.data_ptr())
    need = L.op_workspace(h, op)
    ws = _workspace(dev, need)
    L.check(L.load().rcv_rgb_prep(h, frames.data_ptr(), None if labels is None else labels.data_ptr(), lab_bytes, B, Hs, Ws, H, W,
                                  fx.data_ptr(), kx, fy.data_ptr(), ky, lx.data_ptr(), ly.data_ptr(), params.data_ptr() if train else None,
                                  1 if train else 0, stats, mask, imgs.data_ptr(), None if targets is None else targets.data_ptr(),
                                  None if ws is None else ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), "rcv_rgb_prep")
    return imgs, targets


def draw_color_jitter(B, brightness=0.5, contrast=0.5, saturation=0.4, hue=0.3, vflip=True, reseed=True):
    """The random draws of ``B`` consecutive ``SSDataSet.__getitem__`` calls under the training transforms of trainer.py:88-104, as a
    STATED definition (it cannot be compared with torchvision here): the ``random``-module ``ColorJitter.get_params`` the reference was
    written for -- later torchvision versions draw from torch's generator, under which the ``random.seed(seed)`` of dataset.py:176-183
    no longer ties the label's flips to the frame's.  Per image, in this order:
      1. with ``reseed``: ``np.random.randint(2147483647)`` and ``random.seed`` of it (dataset.py:176-177; the label's transforms
         re-seed with the same value, so both flip draws are shared by frame and label);
      2. ``random.random() < 0.5``: horizontal flip (transform.py:70);  3. the same for the vertical flip, if ``vflip``;
      4. for each strength > 0, in the order b, c, s, h: ``random.uniform(max(0, 1 - b), 1 + b)``, likewise contrast and saturation,
         then ``random.uniform(-h, h)`` for the hue;  5. ``random.shuffle`` of the list of operations.
    Returns the host tensor float32 [B,12] = {hflip, vflip, n_ops, op0, op1, op2, op3, f_brightness, f_contrast, f_saturation, hue_shift,
    0}; op codes 0 = brightness, 1 = contrast, 2 = saturation, 3 = hue, -1 = unused; a factor that was not drawn is 1.0;
    ``hue_shift = int(hue_factor * 255) & 255`` (truncated toward zero: the ``np.uint8(hue_factor * 255)`` of ``adjust_hue``)."""
    rows = torch.zeros(B, 12, dtype=torch.float32)
    for i in range(B):
        if reseed:
            random.seed(np.random.randint(2147483647))
        hf = random.random() < 0.5
        vf = (random.random() < 0.5) if vflip else False
        ops, fac, shift = [], [1.0, 1.0, 1.0], 0
        for code, strength in ((OP_BRIGHTNESS, brightness), (OP_CONTRAST, contrast), (OP_SATURATION, saturation)):
            if strength > 0:
                fac[code] = random.uniform(max(0, 1 - strength), 1 + strength)
                ops.append(code)
        if hue > 0:
            shift = int(random.uniform(-hue, hue) * 255) & 255
            ops.append(OP_HUE)
        random.shuffle(ops)
        rows[i, 0], rows[i, 1], rows[i, 2] = float(hf), float(vf), float(len(ops))
        rows[i, 3:7] = torch.FloatTensor((ops + [-1] * 4)[:4])
        rows[i, 7:10] = torch.FloatTensor(fac)
        rows[i, 10] = float(shift)
    return rows


def draw_color_jitter_rows(n, brightness=0.5, contrast=0.5, saturation=0.4, hue=0.3, vflip=True, reseed=True):
    """The rows of ``draw_color_jitter(n, ...)`` for a whole epoch in one call: bit for bit the same float32 [n,12] host tensor under the
    same ``random`` / ``np.random`` seeds, and both generators are left where ``draw_color_jitter(n)`` leaves them.  The draws are the
    same calls in the same order (nothing is vectorised: ``random.seed`` between two images makes every image's draws its own); the
    rounding to float32 is one array conversion, not three tensor constructions per image."""
    out = []
    for _ in range(n):
        if reseed:
            random.seed(np.random.randint(2147483647))
        hf = random.random() < 0.5
        vf = (random.random() < 0.5) if vflip else False
        ops, fac, shift = [], [1.0, 1.0, 1.0], 0
        for code, strength in ((OP_BRIGHTNESS, brightness), (OP_CONTRAST, contrast), (OP_SATURATION, saturation)):
            if strength > 0:
                fac[code] = random.uniform(max(0, 1 - strength), 1 + strength)
                ops.append(code)
        if hue > 0:
            shift = int(random.uniform(-hue, hue) * 255) & 255
            ops.append(OP_HUE)
        random.shuffle(ops)
        out.append([float(hf), float(vf), float(len(ops))] + (ops + [-1] * 4)[:4] + fac + [float(shift), 0.0])
    return torch.from_numpy(np.array(out, np.float64).reshape(n, 12).astype(np.float32))


def prepare_lp_pairs(frames, labels, pairs, train=True, params=None, bad_index=None, contrast=None, num_class=5):
    """LabelProp's input straight from a resident store, one op (RCV_OP_LP_PAIR_PREP): the per-pair work of the loader
    (labelPropTrain.py:36-66) and of the batch assembly (labelPropTrain.py:162-193).

    ``frames`` uint8 [N,H,W,3] and ``labels`` uint8 or int32 [N,H,W]: the store, already at the network's size (``ResidentDataset(...,
    img_size=(H, W))``; another size is refused).  ``pairs`` int32 or int64 [B,2] on the device: the store indices of frame a and frame
    b.  ``params`` float32 [B,12]: ONE ``draw_color_jitter`` row per pair (host rows are checked as ``prepare_rgb_batch`` checks them).
    Returns ``(inputs, targets)``: ``inputs`` of logical shape [2B,8,H,W] whose memory is NHWC, what ``labelprop_batch`` returns and
    ``LabelProp`` reads without a copy, and ``targets`` int64 [2B,H,W].

    Bit for bit ``labelprop_batch(imgs.view(B,2,3,H,W), tgts.view(B,2,H,W))`` of ``imgs, tgts = prepare_rgb_batch(frames[pairs.flatten()],
    labels[pairs.flatten()], img_size=(H, W), params=params.repeat_interleave(2, 0))``: both frames and both label planes of a pair are
    mirrored alike, both frames get the same colour operations with the contrast mean of EACH FRAME ON ITS OWN, only Y is computed, a
    label outside [0, 5) gives -1 in all five class channels, and there is no ``maskLabel``.  That one shared row per pair is the
    project's own definition (the ``LPDataSet(root, split=, img_transform=, label_transform=)`` that labelPropTrain.py:79 calls is not in
    the reference; ``Ya - Yb`` needs both frames mirrored alike, which is all the script fixes).  A pair with either index outside
    [0, N) comes back as zeros (both samples, all 8 channels, targets 0) and is counted once in ``bad_index``.  ``contrast``: as
    ``prepare_rgb_batch``."""
    if num_class != 5:
        raise ValueError("prepare_lp_pairs: num_class must be 5 (LabelProp's first conv reads 3 + 5 channels), got %r" % (num_class,))
    if not (torch.is_tensor(frames) and torch.is_tensor(labels)):
        raise TypeError("prepare_lp_pairs: frames and labels must be tensors")
    if frames.dtype != torch.uint8 or labels.dtype not in (torch.uint8, torch.int32):
        raise TypeError("prepare_lp_pairs: frames must be uint8 and labels uint8 or int32 (got %s, %s)" % (frames.dtype, labels.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or labels.dim() != 3 or tuple(labels.shape) != tuple(frames.shape[:3]) or frames.shape[0] < 1:
        raise ValueError("prepare_lp_pairs: frames must be [N,H,W,3] and labels [N,H,W] (got %s, %s)" % (tuple(frames.shape), tuple(labels.shape)))
    N, H, W, _ = frames.shape
    _check_index("prepare_lp_pairs", pairs, 2)
    B = int(pairs.shape[0])
    stats = 0
    if train:
        if params is None:
            raise ValueError("prepare_lp_pairs: train=True needs params (draw_color_jitter(B): one row per pair)")
        if not torch.is_tensor(params) or params.dtype != torch.float32 or tuple(params.shape) != (B, 12):
            raise TypeError("prepare_lp_pairs: params must be a float32 [B,12] tensor (draw_color_jitter: one row per pair)")
        stats = 1
        if params.device.type == "cpu":
            stats = int(_check_color_rows(params.numpy(), "prepare_lp_pairs").any())
        elif contrast is not None:
            stats = 1 if contrast else 0
    if frames.device.type != "cuda" or labels.device != frames.device:
        raise L.RcvError("prepare_lp_pairs runs on the HIP device only (frames on %s, labels on %s)" % (frames.device, labels.device))
    if not (frames.is_contiguous() and labels.is_contiguous()):
        raise ValueError("prepare_lp_pairs: frames and labels must be contiguous (no hidden copy of a store)")
    dev = frames.device
    bad_index = _index_args("prepare_lp_pairs", pairs, bad_index, dev, 2)
    if train:
        params = params.to(dev).contiguous()
    inputs = torch.empty(2 * B, H, W, 8, dtype=torch.float32, device=dev)
    targets = torch.empty(2 * B, H, W, dtype=torch.int64, device=dev)
    h = _handle(dev)
    op = L.make_op(L.OP_LP_PAIR_PREP, n=B, stride=N, h=H, w=W, ho=H, wo=W, cout=num_class, inmode2=labels.element_size(),
                   inmode=pairs.element_size(), aux0=1 if train else 0, count=stats, p_in_aux=pairs.data_ptr(), p_epi_aux=bad_index.data_ptr())
    need = L.op_workspace(h, op)
    ws = _workspace(dev, need)
    L.check(L.load().rcv_lp_pair_prep(h, frames.data_ptr(), labels.data_ptr(), labels.element_size(), N, pairs.data_ptr(), pairs.element_size(),
                                      B, H, W, H, W, num_class, params.data_ptr() if train else None, 1 if train else 0, stats,
                                      inputs.data_ptr(), targets.data_ptr(), bad_index.data_ptr(), None if ws is None else ws.data_ptr(), need,
                                      torch.cuda.current_stream(dev).cuda_stream), "rcv_lp_pair_prep")
    return inputs.permute(0, 3, 1, 2), targets


def _tryint(s):
    try:
        return int(s)
    except ValueError:
        return s


def _natural_key(s):
    return [_tryint(c) for c in re.split("([0-9]+)", s)]


class SSYUVDataset:
    """The file listing of the reference's ``SSYUVDataset`` (dataset.py:66-105: ``<data_dir>[/FinetuneHorizon]/{train,val}/{images,
    labels}/*.png`` in natural order; where every image has a ``.txt`` next to it, ``camera`` "top" keeps the files whose text is "u" and
    "bottom" those whose text is "b") with a ``__getitem__`` that only decodes: ``(uint8 [Hs,Ws,3], int32 [Hs,Ws])`` numpy arrays.
    Resize, normalisation and augmentation are ``prepare_batch``'s.  Pillow is imported on first decode."""

    def __init__(self, data_dir, img_size=(120, 160), train=True, finetune=False, camera="both"):
        self.img_size = img_size
        self.train = train
        self.finetune = finetune
        self.images, self.labels = [], []
        if finetune:
            data_dir = osp.join(data_dir, "FinetuneHorizon")
        data_dir = osp.join(data_dir, "train" if train else "val")
        self.img_dir = osp.join(data_dir, "images")
        self.lab_dir = osp.join(data_dir, "labels")
        img_files = self._list(self.img_dir, ".png")
        txt_files = self._list(self.img_dir, ".txt")
        lab_files = self._list(self.lab_dir, ".png")
        if len(txt_files) == len(img_files):
            for img, lab, txt in zip(img_files, lab_files, txt_files):
                with open(osp.join(self.img_dir, txt)) as f:
                    char = f.read()
                if camera == "both" or (camera == "top" and char == "u") or (camera == "bottom" and char == "b"):
                    self.images.append(img)
                    self.labels.append(lab)
        else:
            for img, lab in zip(img_files, lab_files):
                self.images.append(img)
                self.labels.append(lab)

    @staticmethod
    def _list(d, ext):          # glob.glob1(d, "*" + ext) in natural order
        names = [n for n in os.listdir(d) if n.endswith(ext) and not n.startswith(".")] if osp.isdir(d) else []
        return sorted(names, key=_natural_key)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        from PIL import Image
        with Image.open(osp.join(self.img_dir, self.images[index])) as im:
            frame = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(osp.join(self.lab_dir, self.labels[index])) as im:
            label = np.asarray(im.convert("I"), dtype=np.int32)
        return np.ascontiguousarray(frame), np.ascontiguousarray(label)


class SSDataSet:
    """The file listing of the reference's ``SSDataSet`` (dataset.py:135-164: ``<root>/<split>/{images,labels}/*.png`` in natural order,
    the ``camera`` filter of ``SSYUVDataset``) with a ``__getitem__`` that only decodes: ``(uint8 [Hs,Ws,3], int32 [Hs,Ws])`` numpy
    arrays.  The transforms are ``prepare_rgb_batch``'s, the draws ``draw_color_jitter``'s.  Pillow is imported on first decode."""

    def __init__(self, root, split="train", camera="both"):
        self.root = root
        self.split = split
        self.images, self.labels = [], []
        data_dir = osp.join(root, split)
        self.img_dir = osp.join(data_dir, "images")
        self.lab_dir = osp.join(data_dir, "labels")
        img_files = SSYUVDataset._list(self.img_dir, ".png")
        txt_files = SSYUVDataset._list(self.img_dir, ".txt")
        lab_files = SSYUVDataset._list(self.lab_dir, ".png")
        if len(txt_files) == len(img_files):
            for img, lab, txt in zip(img_files, lab_files, txt_files):
                with open(osp.join(self.img_dir, txt)) as f:
                    char = f.read()
                if camera == "both" or (camera == "top" and char == "u") or (camera == "bottom" and char == "b"):
                    self.images.append(img)
                    self.labels.append(lab)
        else:
            for img, lab in zip(img_files, lab_files):
                self.images.append(img)
                self.labels.append(lab)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        from PIL import Image
        with Image.open(osp.join(self.img_dir, self.images[index])) as im:
            frame = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(osp.join(self.lab_dir, self.labels[index])) as im:
            label = np.asarray(im.convert("I"), dtype=np.int32)
        return np.ascontiguousarray(frame), np.ascontiguousarray(label)


class ResidentDataset:
    """A whole dataset as resized bytes on the device: ``frames`` uint8 [N,H,W,3] and ``labels`` [N,H,W], made once.

    ``dataset[i]`` gives ``(uint8 [Hs,Ws,3], integer [Hs,Ws])`` arrays (``SSYUVDataset``; any sequence of such pairs).  Every item is
    decoded once on the host (at most 16 threads), uploaded in chunks of ``chunk`` items and resized there with ``resize_u8``; a chunk is
    cut where the source size changes, so mixed source sizes are allowed (a frame that keeps exactly one axis raises, as
    ``prepare_batch`` does).  Labels are kept as uint8 when every decoded value is in 0..255 -- checked on the host array of every chunk
    -- and as int32 otherwise.

    Pinned: the stored bytes are Pillow's, byte for byte, so ``prepare_batch(store.frames, store.labels, img_size, index=...)`` is bit
    for bit ``prepare_batch`` of the full-size frames gathered by the same indices.  ``bad_index`` (int32 [1] on the device) counts the
    images a batch asked for outside [0, N); ``check()`` reads it."""

    MAX_THREADS = 16

    def __init__(self, dataset, img_size=(120, 160), device="cuda", chunk=64):
        from concurrent.futures import ThreadPoolExecutor
        self._start(img_size, device, chunk)
        n = len(dataset)
        with ThreadPoolExecutor(max_workers=max(1, min(self.MAX_THREADS, os.cpu_count() or 1))) as pool:
            for a in range(0, n, self.chunk):
                items = list(pool.map(dataset.__getitem__, range(a, min(n, a + self.chunk))))
                k = 0
                while k < len(items):          # runs of one source size
                    e = k + 1
                    while e < len(items) and np.shape(items[e][0]) == np.shape(items[k][0]):
                        e += 1
                    fr = np.stack([np.asarray(it[0], np.uint8) for it in items[k:e]])
                    lb = np.stack([np.asarray(it[1]) for it in items[k:e]])
                    small = lb.size == 0 or (int(lb.min()) >= 0 and int(lb.max()) <= 255)
                    lb = lb.astype(np.uint8 if small else np.int32, copy=False)
                    self._add(torch.from_numpy(fr), torch.from_numpy(lb), small)
                    k = e
        self._finish()

    @classmethod
    def from_tensors(cls, frames, labels, img_size=(120, 160), device=None, chunk=64):
        """The same store from tensors already in memory: ``frames`` uint8 [N,Hs,Ws,3] and ``labels`` uint8 or int32 [N,Hs,Ws], on the
        host or on the device (``device`` defaults to theirs if they are on one, else to "cuda")."""
        if not (torch.is_tensor(frames) and torch.is_tensor(labels)) or frames.dim() != 4 or labels.dim() != 3 \
                or frames.shape[:3] != labels.shape:
            raise ValueError("ResidentDataset.from_tensors: frames must be a [N,Hs,Ws,3] tensor and labels [N,Hs,Ws]")
        self = cls.__new__(cls)
        self._start(img_size, device if device is not None else (frames.device if frames.device.type == "cuda" else "cuda"), chunk)
        small = labels.dtype == torch.uint8 or labels.numel() == 0 or (int(labels.min()) >= 0 and int(labels.max()) <= 255)
        for a in range(0, frames.shape[0], self.chunk):
            self._add(frames[a:a + self.chunk], labels[a:a + self.chunk], small)
        self._finish()
        return self

    def _start(self, img_size, device, chunk):
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.chunk = max(1, int(chunk))
        self._parts = []

    def _add(self, frames, labels, small):
        f = frames.to(self.device).contiguous()
        lab = labels.to(self.device).contiguous()
        self._parts.append(resize_u8(f, lab, self.img_size, label_dtype=torch.uint8 if small else torch.int32))

    def _finish(self):
        if not self._parts:
            raise ValueError("ResidentDataset: the dataset is empty")
        wide = any(p[1].dtype == torch.int32 for p in self._parts)
        self.frames = torch.cat([p[0] for p in self._parts]).contiguous()
        self.labels = torch.cat([p[1].to(torch.int32) if wide else p[1] for p in self._parts]).contiguous()
        self.bad_index = torch.zeros(1, dtype=torch.int32, device=self.device)
        del self._parts

    def __len__(self):
        return int(self.frames.shape[0])

    def check(self):
        """Reads the bad-index counter (this synchronises: call it once an epoch, not once a batch) and raises if a batch asked for an
        image outside the store; the counter is cleared so the next epoch starts clean."""
        bad = int(self.bad_index.item())
        if bad:
            self.bad_index.zero_()
            raise IndexError("ResidentDataset: %d images were asked for outside [0, %d): they came back as zeros with targets 0" % (bad, len(self)))


class EpochLoader:
    """One epoch of training (or validation) batches per ``iter()`` from a ``ResidentDataset``, with no host tensor work and no
    synchronisation per batch: the epoch's permutation (``torch.randperm(N, generator=generator)`` on the host, or ``arange`` without
    ``shuffle``) and, with ``train``, its ``draw_jitter_rows`` are uploaded once from pinned memory, and every ``next()`` is one
    ``prepare_batch(store.frames, store.labels, index=perm_dev[a:b], params=rows_dev[a:b])``.

    The project's own definition (the order of the reference's multi-worker ``DataLoader`` cannot be reproduced by any single process):
    rank ``rank`` of ``world`` takes ``perm[rank::world]``, and row ``i`` of its draws belongs to the ``i``-th sample it visits -- the
    order a single-process reference loader draws in.  Pinned: every batch, bit for bit, to ``prepare_batch`` of the full-size frames
    gathered by the same indices with the same rows.  ``last_index`` / ``last_rows`` keep the host copies of the running epoch.
    ``len()`` is ``DataLoader``'s: ``ceil(n / batch_size)``, ``floor`` with ``drop_last``, ``n`` = this rank's share.

    An epoch's host work (for 4096 samples about 4 ms, nearly all of it the draws) is done when its first batch is asked for; after a
    synchronisation at the end of the epoch before (``check()``, reading metrics) the device waits for it with nothing queued.
    ``prefetch=True`` does that work for the NEXT epoch when an epoch has been iterated to its end, while the device still runs the
    steps just enqueued: the same draws from the same generators in the same order, only earlier -- so one epoch's worth is drawn
    after the last epoch and never used, and anything else that draws from ``random`` / ``torch`` / ``generator`` between two epochs
    now draws after them.  Off by default for that reason."""

    def __init__(self, resident, batch_size, train=True, shuffle=True, finetune=False, no_ball=False, no_robot=False, no_goal=False,
                 no_line=False, jitter=(0.3, 0.3, 0.3, 3.1415 / 6), generator=None, drop_last=False, rank=0, world=1, prefetch=False):
        if int(batch_size) < 1 or int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("EpochLoader: batch_size %r, rank %r of world %r" % (batch_size, rank, world))
        self.resident = resident
        self.batch_size = int(batch_size)
        self.train, self.shuffle, self.finetune = bool(train), bool(shuffle), bool(finetune)
        self.flags = dict(no_ball=no_ball, no_robot=no_robot, no_goal=no_goal, no_line=no_line)
        self.jitter = tuple(jitter)
        self.generator = generator
        self.drop_last = bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        self.prefetch = bool(prefetch)
        self.last_index = self.last_rows = self._next = None

    def _share_len(self, n):
        return len(range(self.rank, n, self.world))

    def __len__(self):
        n = self._share_len(len(self.resident))
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def share(self, epoch_perm):
        """This rank's part of an epoch's permutation, in the order it is visited."""
        return epoch_perm[self.rank::self.world]

    def plan(self, epoch_perm):
        """Host only: the ``(a, b)`` slices of ``share(epoch_perm)`` (and of the epoch's rows) that make the batches, in order."""
        n, bs = self._share_len(len(epoch_perm)), self.batch_size
        return [(a, min(n, a + bs)) for a in range(0, n, bs) if not self.drop_last or a + bs <= n]

    def _draw_epoch(self):
        """The host work of one epoch: permutation, share, draws, slices, and the two uploads from pinned memory."""
        res = self.resident
        n = len(res)
        perm = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        index = self.share(perm).contiguous()
        rows = draw_jitter_rows(int(index.shape[0]), *self.jitter) if self.train else None
        slices = self.plan(perm)
        index_dev = rows_dev = None
        if slices:
            index_dev = index.pin_memory().to(res.device, non_blocking=True)
            rows_dev = rows.pin_memory().to(res.device, non_blocking=True) if self.train else None
        return index, rows, slices, index_dev, rows_dev

    def __iter__(self):
        res = self.resident
        epoch, self._next = self._next if self._next is not None else self._draw_epoch(), None
        self.last_index, self.last_rows, slices, index_dev, rows_dev = epoch
        for a, b in slices:
            yield prepare_batch(res.frames, res.labels, res.img_size, finetune=self.finetune, train=self.train,
                                params=rows_dev[a:b] if self.train else None, index=index_dev[a:b], bad_index=res.bad_index, **self.flags)
        if self.prefetch:          # the consumer has enqueued its last step and asks for more: the device is busy, the host is free
            self._next = self._draw_epoch()


class RGBEpochLoader(EpochLoader):
    """``EpochLoader`` for the RGB loader (trainer.py:75-123; pruner.py, classTrainer.py): one epoch of ``prepare_rgb_batch`` batches per
    ``iter()`` from a ``ResidentDataset`` built at the SCALED size.  The bookkeeping is ``EpochLoader``'s, unchanged in meaning
    (``randperm`` with ``generator`` on the host, ``perm[rank::world]``, row ``i`` belongs to the ``i``-th sample visited, ``last_index``
    / ``last_rows``, ``plan``, ``share``, ``len``, ``prefetch``); the rows are ``draw_color_jitter_rows(n, *jitter, vflip=vflip)``, checked
    ONCE on the host (codes 0..3, each at most once), and every ``next()`` is one ``prepare_rgb_batch(store.frames, store.labels,
    img_size=store.img_size, index=perm_dev[a:b], params=rows_dev[a:b], bad_index=store.bad_index)`` that is told whether its slice
    holds a contrast, so the statistics launch is skipped where it has nothing to do.  No host tensor work and no synchronisation per
    batch.  Pinned: every batch, bit for bit, to ``prepare_rgb_batch`` of the full-size frames gathered by the same indices with the same
    rows."""

    def __init__(self, resident, batch_size, train=True, shuffle=True, jitter=(0.5, 0.5, 0.4, 0.3), vflip=True, no_ball=False, no_robot=False,
                 no_goal=False, no_line=False, generator=None, drop_last=False, rank=0, world=1, prefetch=False):
        EpochLoader.__init__(self, resident, batch_size, train=train, shuffle=shuffle, no_ball=no_ball, no_robot=no_robot, no_goal=no_goal,
                             no_line=no_line, jitter=jitter, generator=generator, drop_last=drop_last, rank=rank, world=world,
                             prefetch=prefetch)
        self.vflip = bool(vflip)

    def _count(self):
        return len(self.resident)

    def __len__(self):
        n = self._share_len(self._count())
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _pick(self, share):
        """What a sample of this rank's share is on the device: its store index."""
        return share.contiguous()

    def _draw_epoch(self):
        """The host work of one epoch: permutation, share, draws and their check, slices with their contrast hints, the two uploads."""
        dev = self.resident.device
        n = self._count()
        perm = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        index = self._pick(self.share(perm))
        slices = self.plan(perm)
        rows = hints = None
        if self.train:
            rows = draw_color_jitter_rows(int(index.shape[0]), *self.jitter, vflip=self.vflip)
            has = _check_color_rows(rows.numpy(), type(self).__name__)
            hints = [bool(has[a:b].any()) for a, b in slices]
        index_dev = rows_dev = None
        if slices:
            index_dev = index.pin_memory().to(dev, non_blocking=True)
            rows_dev = rows.pin_memory().to(dev, non_blocking=True) if self.train else None
        return index, rows, slices, index_dev, rows_dev, hints

    def _batch(self, index, rows, hint):
        res = self.resident
        return prepare_rgb_batch(res.frames, res.labels, img_size=res.img_size, train=self.train, params=rows, index=index,
                                 bad_index=res.bad_index, contrast=hint, **self.flags)

    def __iter__(self):
        epoch, self._next = self._next if self._next is not None else self._draw_epoch(), None
        self.last_index, self.last_rows, slices, index_dev, rows_dev, hints = epoch
        for k, (a, b) in enumerate(slices):
            yield self._batch(index_dev[a:b], rows_dev[a:b] if self.train else None, hints[k] if self.train else None)
        if self.prefetch:
            self._next = self._draw_epoch()


class _LPFrames:
    """The flat sequence of decoded ``(uint8 [Hs,Ws,3], int32 [Hs,Ws])`` items of an ``LPDataSet``: what ``ResidentDataset`` takes."""

    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        from PIL import Image
        with Image.open(self.images[index]) as im:
            frame = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(self.labels[index]) as im:
            label = np.asarray(im.convert("I"), dtype=np.int32)
        return np.ascontiguousarray(frame), np.ascontiguousarray(label)


class LPDataSet:
    """The file listing of the reference's ``LPDataSet`` (dataset.py:191-228): ``<root>/LabelProp/{Real,Synthetic}/{train,val}/<dir>/
    {images,labels}/*.png`` (``Real`` with ``finetune``), natural-key order within a directory, ``len()`` = sum over the directories of
    ``len(dir) - len_seq + 1`` windows of ``len_seq`` consecutive frames.  Stated difference: the directories are visited in natural-key
    order; the reference takes ``os.listdir`` order, which is not defined.

    ``frames``: the flat sequence of all frames, directory after directory, as ``(uint8 [Hs,Ws,3], int32 [Hs,Ws])`` items that only
    decode -- what ``ResidentDataset`` takes.  ``windows``: int64 [len(), len_seq], the flat indices of each window; no window crosses
    a directory.  ``LPEpochLoader`` runs epochs from the two.  ``__getitem__`` (dataset.py:230-270: cv2-converted YUV) is not built."""

    def __init__(self, root, train=True, finetune=True, len_seq=2):
        if int(len_seq) < 1:
            raise ValueError("LPDataSet: len_seq %r must be >= 1" % (len_seq,))
        self.finetune, self.len_seq = bool(finetune), int(len_seq)
        self.root = osp.join(root, "LabelProp")
        self.split = "train" if train else "val"
        data_dir = osp.join(self.root, "Real" if finetune else "Synthetic", self.split)
        self.images, self.labels = [], []          # per directory, as the reference keeps them
        dirs = sorted((d for d in os.listdir(data_dir) if osp.isdir(osp.join(data_dir, d))), key=_natural_key) if osp.isdir(data_dir) else []
        flat_i, flat_l, win = [], [], []
        for d in dirs:
            img_dir, lab_dir = osp.join(data_dir, d, "images"), osp.join(data_dir, d, "labels")
            imgs = [osp.join(img_dir, f) for f in SSYUVDataset._list(img_dir, ".png")]
            labs = [osp.join(lab_dir, f) for f in SSYUVDataset._list(lab_dir, ".png")]
            if len(imgs) != len(labs):
                raise ValueError("LPDataSet: %s holds %d images and %d labels" % (osp.join(data_dir, d), len(imgs), len(labs)))
            self.images.append(imgs)
            self.labels.append(labs)
            base = len(flat_i)
            win += [[base + k + i for i in range(self.len_seq)] for k in range(len(imgs) - self.len_seq + 1)]
            flat_i += imgs
            flat_l += labs
        self.frames = _LPFrames(flat_i, flat_l)
        self.windows = torch.tensor(win, dtype=torch.int64).reshape(len(win), self.len_seq)

    def __len__(self):
        return int(self.windows.shape[0])

    def __getitem__(self, index):
        raise NotImplementedError("LPDataSet.__getitem__ (dataset.py:230-270) converts with cv2.cvtColor: OpenCV is not available to pin a "
                                  "restatement against, and labelPropTrain.py does not use it; decode with .frames[i], run epochs with "
                                  "ResidentDataset(.frames) + LPEpochLoader(store, .windows)")


class LPEpochLoader(RGBEpochLoader):
    """One epoch of LabelProp batches per ``iter()``: ``windows`` (int64 [n,2], ``LPDataSet.windows``: store indices of frame a and
    frame b) are permuted -- the bookkeeping of ``EpochLoader`` over WINDOWS: ``randperm(n, generator=)``, ``perm[rank::world]``, row ``i``
    of ``draw_color_jitter_rows`` belongs to the ``i``-th window visited -- the permuted [n,2] pairs and the rows are uploaded once, and
    every ``next()`` is one ``prepare_lp_pairs(store.frames, store.labels, pairs_dev[a:b], params=rows_dev[a:b])`` of ``batch_size``
    pairs, i.e. ``2 batch_size`` samples (labelPropTrain.py:91: batch 8).  ``last_index`` is the epoch's [n,2] pairs on the host.
    Windows longer than 2 are refused: the network reads one pair."""

    def __init__(self, resident, windows, batch_size=8, train=True, shuffle=True, jitter=(0.5, 0.5, 0.4, 0.3), vflip=True, generator=None,
                 drop_last=False, rank=0, world=1, prefetch=False):
        if not torch.is_tensor(windows) or windows.dtype not in (torch.int32, torch.int64) or windows.dim() != 2:
            raise TypeError("LPEpochLoader: windows must be an int32 or int64 [n,2] tensor (LPDataSet.windows)")
        if windows.shape[1] != 2:
            raise ValueError("LPEpochLoader: windows of %d frames: only pairs are built (LPDataSet(len_seq=2)); LabelProp reads the two "
                             "frames of one pair" % int(windows.shape[1]))
        RGBEpochLoader.__init__(self, resident, batch_size, train=train, shuffle=shuffle, jitter=jitter, vflip=vflip, generator=generator,
                                drop_last=drop_last, rank=rank, world=world, prefetch=prefetch)
        self.windows = windows.cpu().contiguous()

    def _count(self):
        return int(self.windows.shape[0])

    def _pick(self, share):
        return self.windows[share].contiguous()

    def _batch(self, index, rows, hint):
        res = self.resident
        return prepare_lp_pairs(res.frames, res.labels, index, train=self.train, params=rows, bad_index=res.bad_index, contrast=hint)
