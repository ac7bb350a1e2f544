"""Class maps to colour images on the device: the reference's ``labelcolormap`` / ``Colorize`` (transform.py:139-170) and the batch
form ``colorize`` (RCV_OP_CLS_LABEL, source form 2; csrc/cls_label.hip)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

__all__ = ["labelcolormap", "colorize", "Colorize", "device_palette", "PALETTE_ROWS"]

PALETTE_ROWS = 8          # rows of the device palette (rcv.h RCV_OP_CLS_LABEL: uint8[8][3])
# transform.py:139-156, in the channel order stored there: background, ball, robot, goal, line.  detect.py:133 permutes Colorize's
# [3,H,W] to HWC and cv2.imwrite reads that as BGR -- what the file shows is the caller's business.
_CMAP5 = ((0, 0, 0), (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255))


def labelcolormap(N=5):
    """uint8 [N,3] numpy table: the reference's five rows (transform.py:139-156); rows beyond the fifth are black."""
    N = int(N)
    if N < 1:
        raise ValueError("labelcolormap: N must be >= 1 (got %d)" % N)
    cmap = np.zeros((N, 3), dtype=np.uint8)
    cmap[:min(N, 5)] = np.asarray(_CMAP5[:min(N, 5)], dtype=np.uint8)
    return cmap


_default = {}          # device -> the default palette, uint8 [8,3]


def device_palette(palette, dev):
    """``palette`` (None, or uint8 [k,3] with k <= 8: tensor or numpy array) as the contiguous uint8 [8,3] device tensor the kernels
    read; missing rows are black.  The default -- the reference's five rows -- is cached per device."""
    dev = torch.device(dev)
    if palette is None:
        t = _default.get(str(dev))
        if t is None:
            t = _default[str(dev)] = device_palette(labelcolormap(5), dev)
        return t
    if (torch.is_tensor(palette) and palette.dtype == torch.uint8 and tuple(palette.shape) == (PALETTE_ROWS, 3) and palette.device == dev
            and palette.is_contiguous()):
        return palette          # already in the kernels' form (Segmenter pads and uploads its palette once)
    if isinstance(palette, np.ndarray):
        palette = torch.from_numpy(np.ascontiguousarray(palette))
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8:
        raise TypeError("palette must be a uint8 [k,3] tensor or numpy array, k <= %d" % PALETTE_ROWS)
    if palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= PALETTE_ROWS:
        raise ValueError("palette must be [k,3] with 1 <= k <= %d (got %s)" % (PALETTE_ROWS, tuple(palette.shape)))
    full = torch.zeros(PALETTE_ROWS, 3, dtype=torch.uint8, device=dev)
    full[:palette.shape[0]] = palette.to(dev)
    return full


def colorize(labels, palette=None):
    """``labels`` uint8 or int64 [N,H,W] (or [H,W]) on the HIP device -> uint8 [N,H,W,3] (or [H,W,3]) = ``palette[labels]``, one launch.
    A class outside the palette's eight rows is black, as ``Colorize`` leaves pixels no mask matches."""
    if not torch.is_tensor(labels):
        raise TypeError("colorize: labels must be a tensor")
    if labels.dtype not in (torch.uint8, torch.int64):
        raise TypeError("colorize: labels must be uint8 or int64 (got %s)" % labels.dtype)
    if labels.dim() not in (2, 3) or labels.numel() == 0:
        raise ValueError("colorize: labels must be a non-empty [N,H,W] or [H,W] class map (got %s)" % (tuple(labels.shape),))
    if labels.device.type != "cuda":
        raise L.RcvError("colorize runs on the HIP device only (labels on %s); there is no CPU path" % labels.device)
    dev = labels.device
    pal = device_palette(palette, dev)
    lab = labels.contiguous()
    shape = tuple(lab.shape)
    N, H, W = shape if len(shape) == 3 else (1,) + shape
    out = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    L.check(L.load().rcv_colorize(h, lab.data_ptr(), lab.element_size(), N, H, W, out.data_ptr(), pal.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "rcv_colorize")
    return out


class Colorize:
    """The reference's ``Colorize`` (transform.py:158-170) by name and return layout: ``Colorize()(gray_image)`` -> uint8 [3,H,W] with
    the colours of classes ``0..n-1``; everything else stays 0.  ``gray_image``: a class map [H,W] or [1,H,W], uint8 or int64.
    Stated difference: the result stays on the input's device (the reference returns a CPU ByteTensor); ``.cpu()`` it for OpenCV."""

    def __init__(self, n=5):
        self.n = int(n)
        if not 1 <= self.n <= PALETTE_ROWS:
            raise ValueError("Colorize: n must be in 1..%d (got %d)" % (PALETTE_ROWS, self.n))
        self.cmap = torch.from_numpy(labelcolormap(self.n))

    def __call__(self, gray_image):
        if torch.is_tensor(gray_image) and gray_image.dim() == 3 and gray_image.shape[0] == 1:
            gray_image = gray_image[0]
        if not torch.is_tensor(gray_image) or gray_image.dim() != 2:
            raise ValueError("Colorize: gray_image must be a [H,W] or [1,H,W] class map")
        return colorize(gray_image, self.cmap).permute(2, 0, 1)
