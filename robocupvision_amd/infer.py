"""Segmentation of decoded frames on the device: the loop body of the reference's detect.py:125-138 as two launches plus the network.

    seg = Segmenter(model)                               # puts the model in eval mode
    labels, colour = seg(frames)                         # frames uint8 [B,Hs,Ws,3] on the HIP device

``labels`` uint8 [B,H,W] is what ``SegmentationMetrics.update`` / ``DetectionMetrics.update`` take; ``colour`` uint8 [B,H,W,3] is
``Colorize`` of every map, HWC as detect.py:133 permutes it (cv2.imwrite reads it as BGR).  File writing stays with the caller."""
from __future__ import annotations

from . import _lib as L
from .data import prepare_frames
from .palette import device_palette

__all__ = ["Segmenter"]


class Segmenter:
    """``Segmenter(model)(frames)`` = ``model.predict(prepare_frames(frames, img_size, finetune), colour=True, palette=palette)``.
    ``model``: a ROBO_UNet, PB_FCN, PB_FCN_2 (segmentation mode) on the HIP device; it is put in eval mode here, once -- a caller
    that trains it afterwards calls ``.eval()`` again before the next frame."""

    def __init__(self, model, img_size=(120, 160), finetune=False, palette=None):
        if not hasattr(model, "predict"):
            raise TypeError("Segmenter: model must be one of this package's networks (it has no predict)")
        if getattr(model, "classify", False):
            raise L.RcvError("Segmenter: this model is in classify mode (one class per patch, not a class map)")
        self.model = model.eval()
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.finetune = bool(finetune)
        self._palette = palette
        self._device_palettes = {}          # device -> the palette padded to uint8 [8,3], uploaded once
        if palette is not None:
            device_palette(palette, "cpu")          # a wrong palette is refused at construction

    def __call__(self, frames):
        imgs = prepare_frames(frames, self.img_size, self.finetune)
        pal = None
        if self._palette is not None:
            pal = self._device_palettes.get(imgs.device)
            if pal is None:
                pal = self._device_palettes[imgs.device] = device_palette(self._palette, imgs.device)
        return self.model.predict(imgs, colour=True, palette=pal)
