"""Training batches prepared on the device: the per-image work of the reference's loader (``SSYUVDataset.__getitem__``,
dataset.py:107-133), its ``ColorJitter`` (dataset.py:19-39) and the training loop's ``maskLabel`` (transform.py:26-49, train.py:43-46)
as ONE launch per batch (RCV_OP_BATCH_PREP, csrc/batch_prep.hip).

    ds = SSYUVDataset(root, img_size=(120, 160), train=True)            # decodes only: (uint8 [Hs,Ws,3], int32 [Hs,Ws]) per index
    frames, labels = ...                                                # stacked and uploaded as decoded
    imgs, targets = prepare_batch(frames, labels, (120, 160), params=draw_jitter(len(frames)))
    trainer.step(imgs, targets)

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

Not covered (it keeps raising): ``LPDataSet`` (cv2 ``cvtColor``)."""
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
           "prepare_rgb_batch", "draw_color_jitter", "SSDataSet"]

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


def prepare_batch(frames, labels, img_size=(120, 160), finetune=False, train=True, params=None, no_ball=False, no_robot=False,
                  no_goal=False, no_line=False):
    """``frames`` uint8 [B,Hs,Ws,3] (decoded RGB) and ``labels`` uint8 or int32 [B,Hs,Ws], both on the HIP device -> ``(imgs, targets)``:
    float32 [B,3,H,W] and int64 [B,H,W], what ``Trainer.step`` / ``Trainer.evaluate`` take.  One launch.

    ``train=True`` needs ``params``, the float32 [B,8] rows of ``draw_jitter`` (host or device): flip, then ``(y + b) * c`` and the 2x2
    U/V matrix.  ``train=False`` is the validation loader: resize, normalise, maskLabel.  ``no_ball .. no_line`` are ``maskLabel``'s
    nb, nr, ng, nl.  Exact where the reference's arithmetic is (everything but U/V, which are within 2^-23 (|m0 U| + |m1 V|) of exact,
    as the reference's einsum is).

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
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
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
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    L.check(L.load().rcv_frame_prep(h, frames.data_ptr(), B, Hs, Ws, H, W, fx.data_ptr(), kx, fy.data_ptr(), ky, norm.data_ptr(),
                                    imgs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rcv_frame_prep")
    return imgs


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


def prepare_rgb_batch(frames, labels=None, scale=4, train=True, params=None, no_ball=False, no_robot=False, no_goal=False, no_line=False,
                      img_size=None):
    """``frames`` uint8 [B,Hs,Ws,3] (decoded RGB) and ``labels`` uint8 or int32 [B,Hs,Ws] or None, on the HIP device -> ``(imgs,
    targets)``: float32 YUV [B,3,H,W] and int64 [B,H,W] (None without labels: the patch chain of classTrainer.py / objDetEval.py).
    ``H = int(Hs / scale)``, ``W = int(Ws / scale)`` as transform.py:8-19 ``Scale``; ``scale == 1`` means no resize.  ``img_size=(H, W)``
    in place of ``scale`` names any output size the tables allow (no axis shrinks by more than 8).

    ``train=True`` needs ``params``, the float32 [B,12] rows of ``draw_color_jitter`` (host or device): the two flips, then up to four
    operations on the uint8 pixel in the row's order, exactly as Pillow computes them.  ``train=False`` is the validation chain:
    resize, YUV, normalise, maskLabel -- the same as training mode with no flip and ``n_ops = 0``.  Rows given on the host are checked
    (codes 0..3, each at most once) and the statistics launch is skipped when none of them holds a contrast; rows given on the device
    are taken as they are.  Every output element is exact to the contract of the module docstring.  Same refusals as
    ``prepare_batch``."""
    if not torch.is_tensor(frames) or (labels is not None and not torch.is_tensor(labels)):
        raise TypeError("prepare_rgb_batch: frames (and labels) must be tensors")
    if frames.dtype != torch.uint8 or (labels is not None and labels.dtype not in (torch.uint8, torch.int32)):
        raise TypeError("prepare_rgb_batch: frames must be uint8 and labels uint8 or int32 (got %s, %s)"
                        % (frames.dtype, None if labels is None else labels.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or (labels is not None and labels.dim() != 3):
        raise ValueError("prepare_rgb_batch: frames must be [B,Hs,Ws,3] and labels [B,Hs,Ws] (got %s, %s)"
                         % (tuple(frames.shape), None if labels is None else tuple(labels.shape)))
    B, Hs, Ws, _ = frames.shape
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
    stats = 0
    if train:
        if params is None:
            raise ValueError("prepare_rgb_batch: train=True needs params (draw_color_jitter(B))")
        if not torch.is_tensor(params) or params.dtype != torch.float32 or tuple(params.shape) != (B, 12):
            raise TypeError("prepare_rgb_batch: params must be a float32 [B,12] tensor (draw_color_jitter)")
        stats = 1
        if params.device.type == "cpu":
            rows = params.numpy()
            n, ops = rows[:, 2], rows[:, 3:7]
            used = np.arange(4)[None, :] < n[:, None]
            ok = (n == np.floor(n)) & (n >= 0) & (n <= 4) & (~used | ((ops == np.floor(ops)) & (ops >= 0) & (ops <= 3))).all(1)
            for code in range(4):
                ok &= (used & (ops == code)).sum(1) <= 1
            if not ok.all():
                b = int(np.argmin(ok))
                raise ValueError("prepare_rgb_batch: row %d: n_ops %r with operations %r (codes 0..3, each at most once)"
                                 % (b, float(n[b]), [float(v) for v in ops[b]]))
            stats = int((used & (ops == OP_CONTRAST)).any())
    if frames.device.type != "cuda" or (labels is not None and labels.device != frames.device):
        raise L.RcvError("prepare_rgb_batch runs on the HIP device only (frames on %s, labels on %s)"
                         % (frames.device, None if labels is None else labels.device))
    if not (frames.is_contiguous() and (labels is None or labels.is_contiguous())):
        raise ValueError("prepare_rgb_batch: frames and labels must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    if train:
        params = params.to(dev).contiguous()
    fx, kx, fy, ky, lx, ly = _device_tables(Hs, Ws, H, W, dev)
    imgs = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    targets = None if labels is None else torch.empty(B, H, W, dtype=torch.int64, device=dev)
    mask = (1 if no_ball else 0) | (2 if no_robot else 0) | (4 if no_goal else 0) | (8 if no_line else 0)
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    lab_bytes = 0 if labels is None else labels.element_size()
    op = L.make_op(L.OP_RGB_PREP, n=B, h=Hs, w=Ws, ho=H, wo=W, cin=kx, cout=ky, inmode2=lab_bytes, aux0=1 if train else 0, aux1=mask,
                   count=stats, p_x1=fx.data_ptr(), p_x2=fy.data_ptr(), p_x3=lx.data_ptr(), p_x4=ly.data_ptr())
    need = L.op_workspace(h, op)
    ws = None
    if need:
        ws = _workspaces.get((str(dev), need))
        if ws is None:
            ws = _workspaces[(str(dev), need)] = torch.empty(need // 4, dtype=torch.int32, device=dev)
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
