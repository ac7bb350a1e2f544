"""Segmentation of decoded frames on the device: the loop body of the reference's detect.py:125-138 as two launches plus the network.

    seg = Segmenter(model)                               # puts the model in eval mode
    labels, colour = seg(frames)                         # frames uint8 [B,Hs,Ws,3] on the HIP device

``labels`` uint8 [B,H,W] is what ``SegmentationMetrics.update`` / ``DetectionMetrics.update`` take; ``colour`` uint8 [B,H,W,3] is
``Colorize`` of every map, HWC as detect.py:133 permutes it (cv2.imwrite reads it as BGR).  File writing stays with the caller.

What a user then does with a class map -- find the ball, the robots, the goal posts in it (test.py:43-67: components, cv2.boundingRect,
the box centre; DBConvert.py:47-102: the per-class area rules of the detection data set) -- is ``find_objects``, one op on the device:

    objs = find_objects(labels, **DBCONVERT)             # Objects: rows / counts stay on the device
    seg = Segmenter(model, objects=DBCONVERT)            # labels, colour, objs = seg(frames)
    objs.to_list()                                       # the one host copy: per image [(class, x, y, w, h, area), ...]

and the boxes go on to the patch classifiers without leaving the device (``patches.py``: ``object_patches``, ``classify_objects``):

    seg = Segmenter(model, objects=DBCONVERT, patches={}, classifier=BNNMC().to(dev))
    labels, colour, objs, cut, classes = seg(frames)     # cut.images float32 [P,3,32,32]; classes uint8 [B,C-1,M], 255 = no object

A video stream need not run the segmenter on every frame: ``LabelPropagator`` (makeLPImages.py:94-102, validLabelProp.py:116-135) runs it
on key frames and ``LabelProp`` in between, fed with what was said about the frame before (``model.labelprop_next``, RCV_OP_LP_INPUT):

    prop = LabelPropagator(seg_model, lp_model, key_every=30)      # soft=True: the previous logits, not the class map, are the prior
    labels = prop(imgs)                                  # imgs: a prepared float32 [B,C,H,W] batch, channel 0 = Y"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from . import _lib as L
from .data import prepare_frames
from .palette import colorize, device_palette
from .patches import check_keywords, classify_patches, object_patches

__all__ = ["Segmenter", "LabelPropagator", "find_objects", "Objects", "ObjectsRecord", "DBCONVERT", "majority_filter", "erode_map",
           "open_map", "close_map", "trim_pseudo_labels"]


class _Rules(dict):
    """Keyword arguments of ``find_objects`` with a docstring of their own."""

    def __init__(self, doc, **kw):
        super().__init__(**kw)
        self.__doc__ = doc


DBCONVERT = _Rules(
    """The per-class rules of DBConvert.py:52-100 for the five-class maps (classes 1..4: ball, robot, goal post, line), as keywords of
    ``find_objects`` / ``Segmenter(objects=...)``: minimum area (25, 200, 30, -), minimum share of the class's largest blob (0.05, 0.05,
    0.2, -), at most (6, 5, 2, 0) boxes; lines give no boxes.  Two known differences from that script: (1) area is the PIXEL area of
    the 8-connected component, not ``cv2.contourArea`` of its outline (the polygon area through the pixel centres, smaller by about
    half the perimeter); (2) where a class has more blobs than its cap, the LARGEST are kept (area descending, ties by component number),
    not the first of the script's walk over the contours in ascending area.""",
    num_class=5, min_area=(25, 200, 30, 0), min_ratio=(0.05, 0.05, 0.2, 0.0), max_objects=(6, 5, 2, 0))


def _per_class(v, n, what, conv):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise L.RcvError("find_objects: %s has %d entries, one per class 1..%d expected" % (what, len(v), n))
        seq = list(v)
    else:
        seq = [v] * n
    try:
        return [conv(x) for x in seq]
    except (TypeError, ValueError) as e:
        raise L.RcvError("find_objects: %s: %s" % (what, e)) from None


def _as_int(x):
    if isinstance(x, bool) or int(x) != x:
        raise ValueError("%r is not an integer" % (x,))
    if not -(1 << 31) <= int(x) < (1 << 31):
        raise ValueError("%r does not fit 32 bits" % (x,))
    return int(x)


class ObjectsRecord:
    """One RCV_OP_OBJECTS record and the host arrays (min_ratio double[C-1], min_area / cap int32[C-1]) it points to, kept alive with
    it.  ``form``: 0 = the library routes by shape, 1 / 2 force the general / the single-launch LDS kernels (tests and A/B timing)."""

    def __init__(self, N: int, H: int, W: int, num_class: int = 5, min_area=0, min_ratio=0.0, max_objects=8, elem_bytes: int = 1,
                 form: int = 0):
        try:
            num_class = _as_int(num_class)
        except (TypeError, ValueError) as e:
            raise L.RcvError("find_objects: num_class: %s" % e) from None
        nc = min(max(num_class - 1, 0), 64)      # (the library refuses num_class outside 2..8)
        area = _per_class(min_area, nc, "min_area", _as_int)
        ratio = _per_class(min_ratio, nc, "min_ratio", float)
        cap = _per_class(max_objects, nc, "max_objects", _as_int)
        self.C = num_class
        # a per-class sequence gives the caps and M is its maximum (at least one row); a scalar is both
        self.M = max([1] + cap) if isinstance(max_objects, (list, tuple)) else _per_class(max_objects, 1, "max_objects", _as_int)[0]
        self.min_area = (ctypes.c_int32 * max(nc, 1))(*area)
        self.min_ratio = (ctypes.c_double * max(nc, 1))(*ratio)
        self.cap = (ctypes.c_int32 * max(nc, 1))(*cap)
        self.op = L.make_op(L.OP_OBJECTS, 0, n=N, h=H, w=W, cout=num_class, count=self.M, inmode=elem_bytes, aux0=form,
                            p_x1=ctypes.addressof(self.min_ratio), p_x2=ctypes.addressof(self.min_area), p_x3=ctypes.addressof(self.cap))

    def workspace_bytes(self, h) -> int:
        """rcv_op_workspace: refuses the record (RcvError with the library's message) exactly as an enqueue would."""
        return L.op_workspace(h, self.op)


class Objects:
    """The result of ``find_objects``: two int32 device tensors, ``rows`` [N, C-1, M, 8] = {x, y, w, h, area, rank, 2x+w, 2y+h} (zero
    past the emitted count) and ``counts`` [N, C-1, 4] = {components of the class, |A|, |Q|, emitted}; index 0 of the class axis is
    class 1.  The properties are views / device arithmetic; nothing here synchronises except ``to_list``."""

    def __init__(self, rows: torch.Tensor, counts: torch.Tensor):
        self.rows, self.counts = rows, counts

    @property
    def boxes(self):           # [N, C-1, M, 4] x, y, w, h (cv2.boundingRect)
        return self.rows[..., 0:4]

    @property
    def area(self):            # [N, C-1, M] pixels
        return self.rows[..., 4]

    @property
    def rank(self):            # [N, C-1, M] component number within (image, class), first-2x2-block order
        return self.rows[..., 5]

    @property
    def count(self):           # [N, C-1] emitted rows
        return self.counts[..., 3]

    @property
    def centres(self):         # [N, C-1, M, 2] float64 (x + w/2, y + h/2): test.py:59's predCent
        return self.rows[..., 6:8].to(torch.float64) / 2

    def to_list(self):
        """One host copy: per image the list of (class, x, y, w, h, area), classes ascending, each class largest first."""
        N, Cm1, M, _ = self.rows.shape
        host = torch.cat([self.rows.reshape(-1), self.counts.reshape(-1)]).cpu()
        rows = host[:N * Cm1 * M * 8].reshape(N, Cm1, M, 8).tolist()
        counts = host[N * Cm1 * M * 8:].reshape(N, Cm1, 4).tolist()
        return [[(c + 1,) + tuple(rows[n][c][k][0:5]) for c in range(Cm1) for k in range(counts[n][c][3])] for n in range(N)]


_WORKSPACES = OrderedDict()      # (device, N, H, W) -> workspace tensor, the few most recent shapes
_WORKSPACES_KEPT = 8


def _workspace(dev, shape, nbytes):
    key = (dev,) + tuple(shape)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _WORKSPACES[key] = ws
    _WORKSPACES.move_to_end(key)
    while len(_WORKSPACES) > _WORKSPACES_KEPT:
        _WORKSPACES.popitem(last=False)
    return ws


def find_objects(class_map: torch.Tensor, num_class: int = 5, min_area=0, min_ratio=0.0, max_objects=8, _form: int = 0) -> Objects:
    """The objects of every class map of a batch (RCV_OP_OBJECTS, rcv.h rcv_find_objects): class_map uint8 or int64 [N,H,W] on the HIP
    device, exactly what ``predict`` returns; a pixel is of class v when 1 <= v < num_class.  Per class c (scalars, or sequences of
    length num_class-1 for classes 1..): keep the 8-connected components with area > min_area (strict), of those the ones with
    area >= largest * min_ratio (fp64), and emit the max_objects largest (ties: lower component number first).  A per-class
    max_objects sequence gives the caps; the row count M of the result is its maximum.  Enqueued on the current stream, nothing
    synchronises; the workspace is cached per shape (calls on one shape from several streams at once must not overlap).
    ``_form`` forces a kernel form (ObjectsRecord) -- for tests."""
    if not isinstance(class_map, torch.Tensor) or class_map.dim() != 3:
        raise L.RcvError("find_objects: class_map must be a [N,H,W] tensor")
    eb = {torch.uint8: 1, torch.int64: 8}.get(class_map.dtype)
    if eb is None:
        raise L.RcvError("find_objects: dtype %s unsupported (torch.uint8 or torch.int64)" % class_map.dtype)
    N, H, W = class_map.shape
    rec = ObjectsRecord(N, H, W, num_class, min_area, min_ratio, max_objects, eb, _form)
    if class_map.device.type != "cuda":
        rec.workspace_bytes(L.planner_handle())       # bad arguments are refused with the library's message first
        raise L.RcvError("find_objects needs the class map on the HIP device (there is no CPU path)")
    dev = class_map.device
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    ws = _workspace(dev, (N, H, W), rec.workspace_bytes(h))
    class_map = class_map.contiguous()
    rows = torch.empty(N, rec.C - 1, rec.M, 8, dtype=torch.int32, device=dev)
    counts = torch.empty(N, rec.C - 1, 4, dtype=torch.int32, device=dev)
    op = rec.op
    op.p[L.RCV_P_IN], op.p[L.RCV_P_OUT], op.p[L.RCV_P_X0], op.p[L.RCV_P_PART] = class_map.data_ptr(), rows.data_ptr(), counts.data_ptr(), ws.data_ptr()
    L.OpList([op]).run(h, torch.cuda.current_stream(dev).cuda_stream)
    return Objects(rows, counts)


_MF_PLAN_SLOT = (ctypes.c_int64 * 2)()      # two distinct non-NULL addresses for records that are only planned (never read or written)


def _mf_int(name, what, x):
    try:
        return _as_int(x)
    except (TypeError, ValueError) as e:
        raise L.RcvError("%s: %s: %s" % (name, what, e)) from None


def _mf_set(name, what, classes, default):
    """A sequence of class numbers as a bit set (None: ``default``); whether a class exists is the library's refusal."""
    if classes is None:
        classes = default
    if isinstance(classes, int) and not isinstance(classes, bool):
        classes = (classes,)
    bits = 0
    try:
        for c in classes:
            c = _as_int(c)
            if not 0 <= c < 30:
                raise ValueError("class %d out of range" % c)
            bits |= 1 << c
    except (TypeError, ValueError) as e:
        raise L.RcvError("%s: %s: %s" % (name, what, e)) from None
    return bits


def _map_filter(name, class_map, num_class, window, passes, return_changed=False, plan_only=False):
    """``passes``: one (rule, set, arg0, arg1) for the single-launch rules, two for opening / closing (the first writes the uint8 bit
    map the second counts).  Plans every record first (bad arguments are refused with the library's message, on any device), then
    enqueues them in one run on the current stream."""
    if not isinstance(class_map, torch.Tensor) or class_map.dim() != 3:
        raise L.RcvError("%s: class_map must be a [N,H,W] tensor" % name)
    eb = {torch.uint8: 1, torch.int64: 8}.get(class_map.dtype)
    if eb is None:
        raise L.RcvError("%s: dtype %s unsupported (torch.uint8 or torch.int64)" % (name, class_map.dtype))
    N, H, W = class_map.shape
    C, k = _mf_int(name, "num_class", num_class), _mf_int(name, "window", window)
    ops = [L.make_op(L.OP_MAP_FILTER, 0, n=N, h=H, w=W, cout=C, count=k, inmode=eb, inmode2=1 if rule >= L.MF_OPEN_FINISH else 0,
                     aux0=rule, aux1=s, stride=a0, dil=a1) for rule, s, a0, a1 in passes]
    on_device = class_map.device.type == "cuda" and not plan_only
    h = L.planner_handle()
    if on_device:
        dev = class_map.device
        h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
        class_map = class_map.contiguous()
        out = torch.empty_like(class_map)
        changed = torch.zeros(N, dtype=torch.int32, device=dev) if return_changed else None
        src, dst, cnt = class_map.data_ptr(), out.data_ptr(), changed.data_ptr() if return_changed else None
        mid = _workspace(dev, ("map_filter bits", N, H, W), N * H * W).data_ptr() if len(ops) == 2 else None
    else:
        src, dst, mid, cnt = ctypes.addressof(_MF_PLAN_SLOT), ctypes.addressof(_MF_PLAN_SLOT) + 8, ctypes.addressof(_MF_PLAN_SLOT), None
    if len(ops) == 2:
        ops[0].p[L.RCV_P_IN], ops[0].p[L.RCV_P_OUT] = src, (mid if on_device else dst)
        ops[1].p[L.RCV_P_IN], ops[1].p[L.RCV_P_IN2], ops[1].p[L.RCV_P_OUT], ops[1].p[L.RCV_P_X0] = mid, src, dst, cnt
    else:
        ops[0].p[L.RCV_P_IN], ops[0].p[L.RCV_P_OUT], ops[0].p[L.RCV_P_X0] = src, dst, cnt
    for op in ops:
        L.op_workspace(h, op)
    if plan_only:
        return None
    if not on_device:
        raise L.RcvError("%s needs the class map on the HIP device (there is no CPU path)" % name)
    L.OpList(ops).run(h, torch.cuda.current_stream(dev).cuda_stream)
    return (out, changed) if return_changed else out


def majority_filter(class_map: torch.Tensor, num_class: int = 5, window: int = 4, min_major: int = 15, min_own: int = 7,
                    fill_void: bool = False, return_changed: bool = False, _plan_only: bool = False):
    """The windowed majority vote of labelExtraction.py:70-89 ``__filterMask`` (switched off there at :46: 480 * 640 * 16 Python
    iterations per mask) for a batch of class maps on the device (RCV_OP_MAP_FILTER, rule RCV_MF_MAJORITY; the defaults are the
    reference's).  class_map uint8 or int64 [N,H,W]; a value v is a class when 0 <= v < num_class, else void (255, -100, ...).  Per
    pixel the classes of the window x window neighbourhood (offsets -(window // 2) ... window - 1 - window // 2 on both axes, in-image
    pixels only) are counted; m = the largest count, a = the lowest class that has it.  A void pixel keeps its value unless
    ``fill_void``; otherwise the pixel becomes a when m >= min_major, or when it is a class with fewer than min_own pixels of its own
    class in the window; else it keeps its value.  Returns a new map of the same dtype; ``return_changed`` adds int32 [N], the pixels
    of each image whose value changed.  Enqueued on the current stream, nothing synchronises."""
    name = "majority_filter"
    return _map_filter(name, class_map, num_class, window,
                       [(L.MF_MAJORITY, 1 if fill_void else 0, _mf_int(name, "min_major", min_major), _mf_int(name, "min_own", min_own))],
                       return_changed, _plan_only)


def _all_classes(name, num_class):
    return range(min(max(_mf_int(name, "num_class", num_class), 0), 30))


def erode_map(class_map: torch.Tensor, num_class: int, classes=None, window: int = 3, fill: int = 0, return_changed: bool = False,
              _plan_only: bool = False, _name: str = "erode_map"):
    """Erosion of the regions of ``classes`` (None: every class): a pixel of such a class survives only where every in-image pixel
    of its window has its class (scipy's ``binary_erosion(class_map == c, ones((k, k)), border_value=1)``); the others become
    ``fill`` (0..255 for uint8 maps, any int32 for int64 maps).  Void pixels and other classes are unchanged.  One launch
    (RCV_MF_ERODE); arguments and result as ``majority_filter``."""
    return _map_filter(_name, class_map, num_class, window,
                       [(L.MF_ERODE, _mf_set(_name, "classes", classes, _all_classes(_name, num_class)), _mf_int(_name, "fill", fill), 0)],
                       return_changed, _plan_only)


def open_map(class_map: torch.Tensor, num_class: int, classes=None, window: int = 3, fill: int = 0, return_changed: bool = False,
             _plan_only: bool = False):
    """Morphological opening (erosion, then dilation; odd windows) of the regions of ``classes`` (None: every class): what of a
    region is no window wide -- speckles, thin bridges -- becomes ``fill``; everything else is unchanged.  Two launches
    (RCV_MF_ERODE_BITS into a cached uint8 bit map, RCV_MF_OPEN_FINISH)."""
    name = "open_map"
    s = _mf_set(name, "classes", classes, _all_classes(name, num_class))
    return _map_filter(name, class_map, num_class, window, [(L.MF_ERODE_BITS, s, 0, 0), (L.MF_OPEN_FINISH, s, _mf_int(name, "fill", fill), 0)],
                       return_changed, _plan_only)


def close_map(class_map: torch.Tensor, num_class: int, classes=None, window: int = 3, over=(0,), over_void: bool = True,
              return_changed: bool = False, _plan_only: bool = False):
    """Morphological closing (dilation, then erosion; odd windows) of the regions of ``classes`` (None: 1 ... num_class - 1, the
    objects) -- test.py:41's commented ``cv2.morphologyEx(imgPred, cv2.MORPH_CLOSE, np.ones((3,3)))`` per class: holes and gaps
    narrower than the window are filled.  A closing claims only pixels of the classes in ``over`` (default: background) and, with
    ``over_void``, void pixels: one object never eats another; where two closings claim a pixel the lowest class wins.  Two
    launches (RCV_MF_DILATE_BITS into a cached uint8 bit map, RCV_MF_CLOSE_FINISH)."""
    name = "close_map"
    s = _mf_set(name, "classes", classes, _all_classes(name, num_class)[1:])
    o = _mf_set(name, "over", over, ()) | (L.MF_OVER_VOID if over_void else 0)
    return _map_filter(name, class_map, num_class, window, [(L.MF_DILATE_BITS, s, 0, 0), (L.MF_CLOSE_FINISH, s, 0, o)], return_changed,
                       _plan_only)


def trim_pseudo_labels(pseudo: torch.Tensor, num_class: int, window: int = 3, return_changed: bool = False, _plan_only: bool = False):
    """``erode_map(pseudo, num_class, None, window, fill=-100)`` for the int64 pseudo-label maps of ``Segmenter(pseudo_labels=tau)``: a
    pseudo-label survives only where its whole window agrees with it, so the band along every class boundary and the rim of every
    -100 hole become -100 (ignored by the losses)."""
    if isinstance(pseudo, torch.Tensor) and pseudo.dtype != torch.int64:
        raise L.RcvError("trim_pseudo_labels: int64 pseudo-labels expected (uint8 holds no -100), got %s" % pseudo.dtype)
    return erode_map(pseudo, num_class, None, window, -100, return_changed, _plan_only, "trim_pseudo_labels")


_CLEAN_STEPS = {"majority": (majority_filter, {"num_class", "window", "min_major", "min_own", "fill_void"}),
                "erode": (erode_map, {"num_class", "classes", "window", "fill"}),
                "open": (open_map, {"num_class", "classes", "window", "fill"}),
                "close": (close_map, {"num_class", "classes", "window", "over", "over_void"}),
                "trim": (trim_pseudo_labels, {"num_class", "window"})}


def _clean_steps(clean, num_class, pseudo):
    """``Segmenter(clean=...)`` checked and planned: [(function, keywords)] for the class map and for the pseudo-label map."""
    if not isinstance(clean, (list, tuple)):
        raise L.RcvError("Segmenter: clean must be a list of (step, keywords) pairs, e.g. [('majority', {}), ('close', {'window': 3})]")
    on_labels, on_pseudo = [], []
    for step in clean:
        if not isinstance(step, (list, tuple)) or len(step) != 2 or not isinstance(step[1], dict):
            raise L.RcvError("Segmenter: clean step %r is not a (step, keywords) pair" % (step,))
        fn, allowed = _CLEAN_STEPS.get(step[0], (None, None)) if isinstance(step[0], str) else (None, None)
        if fn is None or (step[0] == "trim" and not pseudo):
            raise L.RcvError("Segmenter: clean step %r unknown (majority, erode, open, close%s)"
                             % (step[0], "; trim with pseudo_labels" if not pseudo else ", trim"))
        if not set(step[1]) <= allowed:
            raise L.RcvError("Segmenter: clean step %r takes the keywords %s (got %s)" % (step[0], sorted(allowed), sorted(step[1])))
        kw = dict(step[1])
        kw.setdefault("num_class", num_class)
        probe = torch.zeros(1, 1, 1, dtype=torch.int64 if step[0] == "trim" else torch.uint8)
        fn(probe, _plan_only=True, **kw)          # a wrong step is refused at construction, with the library's message
        (on_pseudo if step[0] == "trim" else on_labels).append((fn, kw))
    return on_labels, on_pseudo


class Segmenter:
    """``Segmenter(model)(frames)`` = ``model.predict(prepare_frames(frames, img_size, finetune), colour=True, palette=palette)``.
    ``model``: a ROBO_UNet, PB_FCN, PB_FCN_2 (segmentation mode) on the HIP device; it is put in eval mode here, once -- a caller
    that trains it afterwards calls ``.eval()`` again before the next frame.  ``objects``: a dict of ``find_objects`` keywords (e.g.
    ``DBCONVERT``); the call then returns ``(labels, colour, objects)`` with the ``Objects`` of the labels.  ``patches``: a dict of
    the ``object_patches`` keywords size / margin / return_bytes (needs ``objects``; the map size is ``img_size``); the call then
    returns ``(labels, colour, objects, patches)`` with the ``Patches`` cut out of the full-resolution frames.  ``classifier``: a
    patch classifier for ``classify_objects`` (needs ``patches``; put in eval mode here); the call then returns ``(labels, colour,
    objects, patches, classes)`` with the uint8 [N,C-1,M] class of every found object, 255 where a slot holds none.
    ``pseudo_labels``: a confidence threshold tau; the call then returns the pseudo-label map next to the class map, ``(labels,
    pseudo, colour, ...)``: int64 [B,H,W], the class where the softmax confidence is >= tau, else -100 -- ``Trainer.step`` targets
    as they are (the losses ignore labels outside [0, C)).  One forward (``model.proba``'s plan) and one colour launch.
    ``clean``: a list of ``(step, keywords)`` pairs applied in order to the class map before colour, objects and patches see it --
    ``"majority"``, ``"erode"``, ``"open"``, ``"close"`` with the keywords of ``majority_filter`` / ``erode_map`` / ``open_map`` /
    ``close_map`` (num_class defaults to the model's); the colour mask is then ``colorize`` of the cleaned map.  With
    ``pseudo_labels`` a ``("trim", {...})`` step (``trim_pseudo_labels``) applies to the pseudo-label map instead.  Without ``clean``
    nothing changes."""

    def __init__(self, model, img_size=(120, 160), finetune=False, palette=None, objects=None, patches=None, classifier=None,
                 pseudo_labels=None, clean=None):
        if not hasattr(model, "predict"):
            raise TypeError("Segmenter: model must be one of this package's networks (it has no predict)")
        if getattr(model, "classify", False):
            raise L.RcvError("Segmenter: this model is in classify mode (one class per patch, not a class map)")
        self.model = model.eval()
        self._tau = None
        if pseudo_labels is not None:
            if not hasattr(model, "proba"):
                raise TypeError("Segmenter: pseudo_labels needs a model with proba")
            self._tau = float(pseudo_labels)
            if not 0.0 <= self._tau <= 1.0:
                raise ValueError("Segmenter: pseudo_labels is a confidence threshold in [0, 1] (got %r)" % (pseudo_labels,))
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.finetune = bool(finetune)
        self._palette = palette
        self._device_palettes = {}          # device -> the palette padded to uint8 [8,3], uploaded once
        if palette is not None:
            device_palette(palette, "cpu")          # a wrong palette is refused at construction
        self._objects = None
        if objects is not None:
            if not isinstance(objects, dict) or not set(objects) <= {"num_class", "min_area", "min_ratio", "max_objects"}:
                raise L.RcvError("Segmenter: objects must be a dict of find_objects keywords (num_class, min_area, min_ratio, max_objects)")
            self._objects = dict(objects)
            ObjectsRecord(1, 1, 1, **self._objects).workspace_bytes(L.planner_handle())       # wrong rules are refused at construction
        self._patches = None
        self._classifier = None
        if patches is not None:
            if self._objects is None:
                raise L.RcvError("Segmenter: patches needs objects (the boxes to cut out)")
            self._patches = check_keywords(patches, self.img_size, "Segmenter")
        if classifier is not None:
            if self._patches is None:
                raise L.RcvError("Segmenter: classifier needs patches (a dict of object_patches keywords, {} for 32x32 patches)")
            if not isinstance(classifier, torch.nn.Module):
                raise TypeError("Segmenter: classifier must be a module (BNNL, BNNMC, PB_FCN(classify=1), PB_FCN_2(True))")
            self._classifier = classifier.eval()
        self._clean = None
        if clean is not None:
            self._clean = _clean_steps(clean, getattr(model, "numClass", 5), self._tau is not None)

    def __call__(self, frames):
        imgs = prepare_frames(frames, self.img_size, self.finetune)
        pal = None
        if self._palette is not None:
            pal = self._device_palettes.get(imgs.device)
            if pal is None:
                pal = self._device_palettes[imgs.device] = device_palette(self._palette, imgs.device)
        if self._clean is not None:
            if self._tau is None:
                labels, pseudo = self.model.predict(imgs), None
            else:
                labels, pseudo = self.model._proba_maps(imgs, self._tau)
                for fn, kw in self._clean[1]:
                    pseudo = fn(pseudo, **kw)
            for fn, kw in self._clean[0]:
                labels = fn(labels, **kw)
            head = (labels, colorize(labels, pal)) if pseudo is None else (labels, pseudo, colorize(labels, pal))
        elif self._tau is None:
            head = self.model.predict(imgs, colour=True, palette=pal)
        else:
            labels, pseudo = self.model._proba_maps(imgs, self._tau)
            head = (labels, pseudo, colorize(labels, pal))
        labels = head[0]
        if self._objects is None:
            return head
        objs = find_objects(labels, **self._objects)
        if self._patches is None:
            return head + (objs,)
        cut = object_patches(frames, objs, map_size=self.img_size, **self._patches)
        if self._classifier is None:
            return head + (objs, cut)
        return head + (objs, cut, classify_patches(cut, self._classifier))


class LabelPropagator:
    """Labels for a stream of frames: the segmenter on key frames, ``LabelProp`` on the frames between them, fed with what was said
    about the frame before -- the loop of makeLPImages.py:94-102 and the network branch of validLabelProp.py:116-135 on predictions.

        p = LabelPropagator(seg_model, lp_model, key_every=30)      # both models are put in eval mode here
        labels = p(imgs)                                             # imgs float32 [B,C,H,W], channel 0 = Y; labels uint8 [B,H,W]
        labels, colour = p(imgs, colour=True)                        # colour uint8 [B,H,W,3] = palette[labels]
        p.reset()                                                    # the next call is a key frame again

    ``imgs`` is a prepared batch (``prepare_rgb_batch(frames, train=False)``, ``prepare_frames``, ...): the driver does not choose the
    loader.  Call number n since construction or ``reset()`` is a key frame when n == 0 or ``key_every > 0 and n % key_every == 0``.

    ``soft=False``: a key frame is ``seg_model.predict(imgs)``; a propagated frame is ``lp_model.predict(labelprop_next(imgs, plane,
    labels_prev))``, the uint8 class map of the frame before as the prior.  ``soft=True``: the prior is ``2 * softmax - 1`` of the
    LOGITS of the frame before (``seg_model(imgs)`` on a key frame, ``lp_model(labelprop_next(imgs, plane, logits_prev))`` otherwise) and
    the labels are their first arg-max, ``torch.max(logits, 1)[1]``.  State -- the Y plane ``labelprop_next(keep_plane=True)`` kept
    and the previous labels or logits -- stays on the device; nothing synchronises.  A batch of another shape or on another device
    without ``reset()`` is refused: the state belongs to the stream it came from."""

    def __init__(self, seg_model, lp_model, key_every=0, soft=False, palette=None):
        for name, m in (("seg_model", seg_model), ("lp_model", lp_model)):
            if not hasattr(m, "predict"):
                raise TypeError("LabelPropagator: %s must be one of this package's networks (it has no predict)" % name)
        if getattr(seg_model, "classify", False):
            raise L.RcvError("LabelPropagator: seg_model is in classify mode (one class per patch, not a class map)")
        if isinstance(key_every, bool) or not isinstance(key_every, int) or key_every < 0:
            raise ValueError("LabelPropagator: key_every must be an integer >= 0 (0 = only the first frame is a key frame), got %r" % (key_every,))
        self.seg_model, self.lp_model = seg_model.eval(), lp_model.eval()
        self.key_every, self.soft = key_every, bool(soft)
        self._palette = palette
        self._device_palettes = {}          # device -> the palette padded to uint8 [8,3], uploaded once
        if palette is not None:
            device_palette(palette, "cpu")          # a wrong palette is refused at construction
        self.reset()

    def reset(self):
        """Forget the stream: the next call is a key frame."""
        self._n, self._key, self._plane, self._prior = 0, None, None, None

    @property
    def prior(self):
        """What the last call said about its frames and the next call reads as its prior: the uint8 class map, with ``soft`` the
        logits; None before the first call and after ``reset()``."""
        return self._prior

    @property
    def plane(self):
        """The Y plane float32 [B,H,W] kept of the last call's frames (the next call's previous frame), or None."""
        return self._plane

    def _pal(self, dev):
        pal = self._device_palettes.get(dev)
        if pal is None:
            pal = self._device_palettes[dev] = device_palette(self._palette, dev)
        return pal

    def __call__(self, imgs, colour=False):
        from .model import labelprop_next
        from .palette import colorize
        if not torch.is_tensor(imgs) or imgs.dtype != torch.float32 or imgs.dim() != 4:
            raise TypeError("LabelPropagator: imgs must be a float32 [B,C,H,W] tensor (a prepared batch, channel 0 = Y)")
        if imgs.device.type != "cuda":
            raise L.RcvError("LabelPropagator runs on the HIP device only (imgs on %s); there is no CPU path" % imgs.device)
        key = (tuple(imgs.shape), imgs.device)
        if self._key is not None and key != self._key:
            raise L.RcvError("LabelPropagator: this batch is %s on %s, the stream so far %s on %s; call reset() before another stream"
                             % (key[0], key[1], self._key[0], self._key[1]))
        key_frame = self._n == 0 or (self.key_every > 0 and self._n % self.key_every == 0)
        pal = self._pal(imgs.device) if colour else None
        col = None
        with torch.no_grad():
            if key_frame:
                plane = imgs[:, 0].clone(memory_format=torch.contiguous_format)      # (the caller's buffer is not held on to)
                x = imgs
                model = self.seg_model
            else:
                x, plane = labelprop_next(imgs, self._plane, self._prior, keep_plane=True)
                model = self.lp_model
            if self.soft:
                prior = model(x)
                labels = torch.max(prior, 1)[1].to(torch.uint8)
                if colour:
                    col = colorize(labels, pal)
            elif colour:
                labels, col = model.predict(x, colour=True, palette=pal)
                prior = labels
            else:
                prior = labels = model.predict(x)
        self._key, self._plane, self._prior = key, plane, prior
        self._n += 1
        return (labels, col) if colour else labels
