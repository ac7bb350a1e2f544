"""Object patches on the device: the step between ``find_objects`` and the patch classifiers (``BNNL`` / ``BNNMC`` /
``PB_FCN(classify=1)`` / ``PB_FCN_2(True)``, the verifiers of the reference's objDetEval.py, classVal.py and classTrainer.py).

    objs = find_objects(labels, **DBCONVERT)                      # boxes in class-map pixels, on the device
    p = object_patches(frames, objs, map_size=labels.shape[1:])   # Patches: images float32 [P,3,32,32], P = N (C-1) M slots
    cls = classify_objects(frames, objs, BNNMC().to(dev).eval(), map_size=labels.shape[1:])      # uint8 [N,C-1,M], 255 = no object

One launch (RCV_OP_OBJECT_PATCHES, csrc/patches.hip), one workgroup per slot; nothing synchronises and nothing goes through the host.
The contract (include/rcv.h ``rcv_object_patches``; restated in tests/patches_restatement.py): the box of a valid slot, widened by
``margin`` map pixels and clamped to the map, is scaled to frame pixels in float64 and resized exactly as Pillow's
``Image.resize((Sw, Sh), BILINEAR, box=...)`` resizes it, then converted as step 4 of ``prepare_rgb_batch`` converts (rgb2yuv +
``Normalize([.5, 0, 0], [.5, .5, .5])``).  Slots past a class's emitted count are zero.  There is no CPU path."""
from __future__ import annotations

import torch

from . import _lib as L

__all__ = ["object_patches", "classify_objects", "classify_patches", "Patches", "PatchesRecord", "NO_OBJECT"]

NO_OBJECT = 255          # the class byte of a slot that holds no object


def _as_int(x, what):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or int(x) != x:
        raise L.RcvError("object_patches: %s: %r is not an integer" % (what, x))
    if not -(1 << 31) <= int(x) < (1 << 31):
        raise L.RcvError("object_patches: %s: %r does not fit 32 bits" % (what, x))
    return int(x)


def _pair(v, what):
    if not isinstance(v, (tuple, list, torch.Size)) or len(v) != 2:
        raise L.RcvError("object_patches: %s must be a pair (rows, columns), got %r" % (what, v))
    return _as_int(v[0], what), _as_int(v[1], what)


class PatchesRecord:
    """One RCV_OP_OBJECT_PATCHES record for frames [N,Hs,Ws,3] and boxes [N,Cm1,M] that live in a map of ``map_size``."""

    def __init__(self, N, Hs, Ws, Cm1, M, map_size=None, size=(32, 32), margin=0):
        self.map_size = (int(Hs), int(Ws)) if map_size is None else _pair(map_size, "map_size")
        self.size = _pair(size, "size")
        self.margin = _as_int(margin, "margin")
        self.op = L.make_op(L.OP_OBJECT_PATCHES, 0, n=N, h=Hs, w=Ws, ho=self.map_size[0], wo=self.map_size[1], cout=Cm1, count=M,
                            aux0=self.size[0], aux1=self.size[1], cin=self.margin)

    def check(self, h) -> None:
        """rcv_op_workspace: refuses the record (RcvError with the library's message) exactly as an enqueue would; no workspace."""
        L.op_workspace(h, self.op)


class Patches:
    """The result of ``object_patches``: ``images`` float32 [P,3,Sh,Sw] (what the patch classifiers read), ``bytes`` uint8
    [P,Sh,Sw,3] (the resized RGB patch) or None, ``shape_nkm`` = (N, C-1, M) with P their product in the order of ``Objects.rows``.
    ``valid`` is device arithmetic on ``counts``; nothing here synchronises."""

    def __init__(self, images, byts, counts, shape_nkm):
        self.images, self.bytes, self.counts, self.shape_nkm = images, byts, counts, tuple(shape_nkm)

    @property
    def valid(self):           # bool [N, C-1, M]: slot k of a class holds an object
        M = self.shape_nkm[2]
        k = torch.arange(M, dtype=torch.int32, device=self.counts.device)
        return k[None, None, :] < self.counts[..., 3].clamp(max=M)[..., None]


def _rows_counts(objects):
    if hasattr(objects, "rows") and hasattr(objects, "counts"):
        return objects.rows, objects.counts
    if isinstance(objects, (tuple, list)) and len(objects) == 2:
        return objects[0], objects[1]
    raise TypeError("object_patches: objects must be an Objects or a (rows, counts) pair")


def object_patches(frames, objects, map_size=None, size=(32, 32), margin=0, return_bytes=False) -> Patches:
    """``frames`` uint8 [N,Hs,Ws,3] (decoded RGB, full resolution) and ``objects`` (an ``Objects`` or its ``(rows, counts)`` int32
    tensors [N,C-1,M,8] / [N,C-1,4]) on the HIP device -> ``Patches``.  ``map_size=(H, W)``: the size of the class map the boxes
    live in (default: the frames' own size; never larger than the frames).  ``size=(Sh, Sw)``: the patch, each side 1..64.
    ``margin`` >= 0 widens every box by that many map pixels on each side before it is clamped to the map.  Enqueued on the
    current stream; nothing synchronises; every output element is written by the launch."""
    rows, counts = _rows_counts(objects)
    if not (torch.is_tensor(frames) and torch.is_tensor(rows) and torch.is_tensor(counts)):
        raise TypeError("object_patches: frames, rows and counts must be tensors")
    if frames.dtype != torch.uint8 or rows.dtype != torch.int32 or counts.dtype != torch.int32:
        raise TypeError("object_patches: frames must be uint8, rows and counts int32 (got %s, %s, %s)" % (frames.dtype, rows.dtype, counts.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or rows.dim() != 4 or rows.shape[3] != 8 or counts.dim() != 3 or counts.shape[2] != 4:
        raise ValueError("object_patches: frames must be [N,Hs,Ws,3], rows [N,C-1,M,8] and counts [N,C-1,4] (got %s, %s, %s)"
                         % (tuple(frames.shape), tuple(rows.shape), tuple(counts.shape)))
    N, Hs, Ws, _ = frames.shape
    _, Cm1, M, _ = rows.shape
    if rows.shape[0] != N or tuple(counts.shape[:2]) != (N, Cm1):
        raise ValueError("object_patches: rows %s / counts %s do not match %d frames" % (tuple(rows.shape), tuple(counts.shape), N))
    rec = PatchesRecord(N, Hs, Ws, Cm1, M, map_size, size, margin)
    if frames.device.type != "cuda" or rows.device != frames.device or counts.device != frames.device:
        rec.check(L.planner_handle())       # bad arguments are refused with the library's message first
        raise L.RcvError("object_patches runs on the HIP device only (frames on %s, rows on %s, counts on %s); there is no CPU path"
                         % (frames.device, rows.device, counts.device))
    if not (frames.is_contiguous() and rows.is_contiguous() and counts.is_contiguous()):
        raise ValueError("object_patches: frames, rows and counts must be contiguous (no hidden copy of a batch)")
    dev = frames.device
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    rec.check(h)
    Sh, Sw = rec.size
    P = N * Cm1 * M
    images = torch.empty(P, 3, Sh, Sw, dtype=torch.float32, device=dev)
    byts = torch.empty(P, Sh, Sw, 3, dtype=torch.uint8, device=dev) if return_bytes else None
    op = rec.op
    op.p[L.RCV_P_IN], op.p[L.RCV_P_IN2], op.p[L.RCV_P_X0], op.p[L.RCV_P_OUT] = frames.data_ptr(), rows.data_ptr(), counts.data_ptr(), images.data_ptr()
    op.p[L.RCV_P_X1] = byts.data_ptr() if return_bytes else None
    L.OpList([op]).run(h, torch.cuda.current_stream(dev).cuda_stream)
    return Patches(images, byts, counts, (N, Cm1, M))


def _patch_classes(classifier, images):
    """uint8 [P]: the class of every patch.  BNNL / BNNMC through their ``predict``; any other module in eval mode under no_grad, its
    [P,k,1,1] logits through ``torch.max(..., 1)`` (PB_FCN(..., classify=1), PB_FCN_2(True))."""
    P = images.shape[0]
    from .bnn import BNNL, BNNMC
    if isinstance(classifier, (BNNL, BNNMC)):
        out = classifier.predict(images)
        if out.numel() != P:
            raise L.RcvError("classify_objects: the classifier gives a %s plane per patch, one class per patch expected (32x32 patches)"
                             % (tuple(out.shape[1:]),))
        return out.reshape(P)
    was_training = classifier.training
    classifier.eval()
    try:
        with torch.no_grad():
            logits = classifier(images)
    finally:
        classifier.train(was_training)
    if not torch.is_tensor(logits) or logits.dim() != 4 or logits.shape[0] != P or tuple(logits.shape[2:]) != (1, 1):
        raise L.RcvError("classify_objects: the classifier returned %s, logits [P,k,1,1] expected (a patch-classification head)"
                         % (tuple(logits.shape) if torch.is_tensor(logits) else type(logits).__name__,))
    return torch.max(logits, 1)[1].reshape(P).to(torch.uint8)


def classify_objects(frames, objects, classifier, **patch_kw):
    """The patch class of every found object: uint8 [N,C-1,M], ``NO_OBJECT`` (255) where a slot holds none.  ``classifier``: a
    ``BNNL`` / ``BNNMC`` in eval mode, or any module that maps float32 [P,3,Sh,Sw] to logits [P,k,1,1]; ``patch_kw``: the keywords of
    ``object_patches``.  Every slot is classified (the batch has a fixed size: nothing waits for the counts); the classes of invalid
    slots are replaced on the device."""
    return classify_patches(object_patches(frames, objects, **patch_kw), classifier)


def classify_patches(patches, classifier):
    """``classify_objects`` for ``Patches`` that are already cut."""
    cls = _patch_classes(classifier, patches.images).reshape(patches.shape_nkm)
    return torch.where(patches.valid, cls, torch.full_like(cls, NO_OBJECT))


def check_keywords(patch_kw, map_size, what):
    """``patch_kw``: a dict of the ``object_patches`` keywords size / margin / return_bytes for boxes that live in maps of ``map_size``;
    refused where it is wrong, with the library's message (used by ``Segmenter`` at construction).  Returns a copy."""
    allowed = ("size", "margin", "return_bytes")
    if not isinstance(patch_kw, dict) or not set(patch_kw) <= set(allowed):
        raise L.RcvError("%s: patches must be a dict of the object_patches keywords %s (map_size is the Segmenter's img_size)"
                         % (what, ", ".join(allowed)))
    kw = dict(patch_kw)
    H, W = map_size
    PatchesRecord(1, H, W, 1, 1, map_size, kw.get("size", (32, 32)), kw.get("margin", 0)).check(L.planner_handle())
    return kw
