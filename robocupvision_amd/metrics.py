"""Device-side evaluation metrics: the pixel accuracy / mean class accuracy / mean IoU that
the reference's valid() builds with O(B*C^2) Python mask loops and `.item()` syncs (train.py:136-178).  One kernel
(RCV_OP_CONFUSION) counts (pred, label) pairs per image; everything else is arithmetic on B*C*C integers.

DetectionMetrics: the object-detection precision / recall of test.py (getPrecRecall, test.py:28-89, printed as its `IoU:` /
`Dist:` rows).  One op (RCV_OP_OBJECT_MATCH, csrc/objdet.hip) labels the blobs and matches them on the device; the host turns the
integer counts into the reference's float64 numbers in the reference's order.

ValidationState: the whole report of valid() -- loss, pixel accuracy over all pixels, mean class accuracy, mean IoU, the score that
picks the weights -- from a state two records keep on the device (RCV_OP_CLS_VALID, RCV_OP_VALID_FOLD).

CalibrationState: what a confidence threshold keeps -- per class and edge the kept and the correct pixels, the confusion of what
survives, accuracy against mean confidence per bin, ECE -- from one integer table RCV_OP_CLS_CALIB keeps on the device."""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L


class SegmentationMetrics:
    def __init__(self, num_class: int, device="cuda"):
        self.C = num_class
        self.device = torch.device(device)
        self.conf = torch.zeros(num_class, num_class, dtype=torch.float64, device=self.device)   # [pred][label]
        self.iou_sum = torch.zeros(num_class, dtype=torch.float64, device=self.device)
        self.n_img = 0

    def update(self, argmax_u8: torch.Tensor, targets: torch.Tensor):
        """argmax_u8: uint8 [B,H,W] (CrossEntropyLoss2d.last_argmax); targets: int64 [B,H,W]."""
        if argmax_u8.dtype != torch.uint8 or argmax_u8.device.type != "cuda":
            raise L.RcvError("SegmentationMetrics.update needs the uint8 arg-max mask on the HIP device")
        B, H, W = argmax_u8.shape
        targets = targets.to(torch.int64).contiguous()
        counts = torch.zeros(B, self.C, self.C, dtype=torch.int32, device=argmax_u8.device)
        h = L.handle(argmax_u8.device.index if argmax_u8.device.index is not None else torch.cuda.current_device())
        op = L.make_op(L.OP_CONFUSION, 0, n=B, h=H, w=W, cout=self.C, p_in=argmax_u8.contiguous().data_ptr(),
                       p_in2=targets.data_ptr(), p_out=counts.data_ptr())
        L.OpList([op]).run(h, torch.cuda.current_stream(argmax_u8.device).cuda_stream)
        c = counts.to(torch.float64)                       # [B][pred][label]
        inter = torch.diagonal(c, dim1=1, dim2=2)          # [B][C]
        union = c.sum(2) + c.sum(1) - inter                # |pred==c| + |label==c| - inter
        self.iou_sum += torch.where(union == 0, torch.ones_like(inter), inter / union.clamp(min=1)).sum(0)   # train.py:148-153
        self.conf += c.sum(0)
        self.n_img += B

    def compute(self) -> dict:
        lab_cnt = self.conf.sum(0)                         # pixels per label (train.py:142)
        total = float(self.conf.sum())
        class_acc = torch.diagonal(self.conf) / (lab_cnt / 100.0)        # conf[(j,j)] of train.py:157-163
        return {"pixel_acc": float(torch.diagonal(self.conf).sum()) / max(total, 1.0) * 100.0,
                "mean_class_acc": float(class_acc.sum()) / self.C,
                "mean_iou": float((self.iou_sum / max(self.n_img, 1)).sum()) / self.C * 100.0,
                "confusion_percent": (self.conf / (lab_cnt / 100.0)).cpu()}


def _ratio(a: float, b: float) -> float:
    """a / b in float64 with IEEE's answers where Python raises: 0 / 0 is NaN (the reference's tensors divide that way)."""
    if b == 0:
        return float("nan") if a == 0 or a != a else (float("inf") if a > 0 else float("-inf"))
    return a / b


def validation_report(state, num_class: int) -> dict:
    """The figures valid() prints (train.py:157-164) from the 76 doubles RCV_OP_VALID_FOLD keeps -- [0] sum of the batch losses,
    [1] batches, [2] images, [3] pixels, [4:12] iou_sum, [12:76] conf[pred][label] in rows of 8 -- in float64 on the host, in the
    reference's order.  A class without a label pixel in the whole pass has 0 / 0 in its column of ``confusion_percent``: NaN there, and
    so in ``mean_class_acc`` and ``score``, exactly as the reference's tensors give it."""
    s = [float(v) for v in state]
    C = num_class
    batches, images, pixels = s[1], s[2], s[3]
    conf = [[s[12 + 8 * p + l] for l in range(C)] for p in range(C)]
    lab_cnt = [sum(conf[p][l] for p in range(C)) for l in range(C)]                      # train.py:144 labCnts (integers: exact)
    percent = [[_ratio(conf[p][l], lab_cnt[l] / 100.0) for l in range(C)] for p in range(C)]      # train.py:157-159
    mean_class_acc = 0.0
    for j in range(C):                                                                     # train.py:162-163
        mean_class_acc += percent[j][j] / C
    iou = 0.0
    for c in range(C):                                                                     # train.py:161 torch.sum(IoU / imgCnt)
        iou += _ratio(s[4 + c], images)
    mean_iou = iou / C * 100
    trace = sum(conf[j][j] for j in range(C))
    return {"loss": _ratio(s[0], batches), "pixel_acc": _ratio(100.0 * trace, pixels), "mean_class_acc": mean_class_acc, "mean_iou": mean_iou,
            "score": (mean_class_acc + mean_iou) / 2, "confusion": torch.tensor(conf, dtype=torch.float64).to(torch.int64).reshape(C, C),
            "confusion_percent": torch.tensor(percent, dtype=torch.float64).reshape(C, C), "images": int(images), "batches": int(batches)}


class ValidationState:
    """The running state of one validation pass (valid(), train.py:97-178), kept on the device: 76 doubles that RCV_OP_VALID_FOLD
    updates once per batch (``model.validate``, ``Trainer.validate``, ``update_from_map``) and the per-image counts buffer
    RCV_OP_CLS_VALID accumulates into, one per batch size.  ``compute()`` is the one read-back.

    ``pixel_acc`` divides by ALL pixels, as the reference does (``running_acc += ... * outSize``), not by the pixels inside the
    confusion matrix as ``SegmentationMetrics`` does: the two differ when ``maskLabel`` or -100 leaves labels outside the classes.  A
    class with no label pixel in the whole pass makes ``mean_class_acc`` and ``score`` NaN, as the reference's 0 / 0 does.  The union
    of an image's IoU is formed from its counts (row + column - diagonal): a pixel predicted c under a label outside the classes is in
    no bin and so not in the union, where train.py:149 counts it; with every label a class the terms are the reference's."""

    def __init__(self, num_class: int, device="cuda"):
        if not isinstance(num_class, int) or not 1 <= num_class <= 8:
            raise ValueError("ValidationState counts 1..8 classes (got %r)" % (num_class,))
        self.C = num_class
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.RcvError("ValidationState lives on the HIP device (got '%s'); there is no CPU path" % self.device)
        self.buf = torch.zeros(L.VALID_STATE, dtype=torch.float64, device=self.device)
        self.device = self.buf.device
        self._counts = {}

    def reset(self):
        self.buf.zero_()
        for c in self._counts.values():
            c.zero_()

    def counts_for(self, n_images: int) -> torch.Tensor:
        """int32 [n_images][C][C], zero between batches (the fold clears what it read)."""
        c = self._counts.get(n_images)
        if c is None:
            c = self._counts[n_images] = torch.zeros(n_images, self.C, self.C, dtype=torch.int32, device=self.device)
        return c

    def update_from_map(self, pred_u8: torch.Tensor, targets: torch.Tensor, loss: torch.Tensor):
        """A batch whose class map and loss exist already (the Dice route: ``criterion.last_argmax`` and the criterion's value):
        RCV_OP_CLS_VALID's class-map form counts, RCV_OP_VALID_FOLD books ``loss`` (a device scalar) as the batch loss."""
        if not torch.is_tensor(pred_u8) or pred_u8.dtype != torch.uint8 or pred_u8.dim() != 3 or pred_u8.device != self.device:
            raise L.RcvError("ValidationState.update_from_map needs the uint8 [B,H,W] class map on %s" % self.device)
        if not torch.is_tensor(targets) or tuple(targets.shape) != tuple(pred_u8.shape):
            raise L.RcvError("ValidationState.update_from_map: targets must be [B,H,W] like the class map %s" % (tuple(pred_u8.shape),))
        if not torch.is_tensor(loss) or loss.numel() != 1 or loss.device != self.device:
            raise L.RcvError("ValidationState.update_from_map: loss must be a one-element tensor on %s (no host value: nothing synchronises)"
                             % self.device)
        B, H, W = pred_u8.shape
        pred_u8 = pred_u8.contiguous()
        targets = targets.to(self.device).to(torch.int64).contiguous()
        loss = loss.detach().to(torch.float32).reshape(1).contiguous()
        counts = self.counts_for(B)
        h = L.handle(self.device.index if self.device.index is not None else torch.cuda.current_device())
        dims = dict(n=B, h=H, w=W, cout=self.C)
        ops = [L.make_op(L.OP_CLS_VALID, 0, cin=1, inmode=L.CLS_LABEL_CLASSMAP, p_in=pred_u8.data_ptr(), p_in2=targets.data_ptr(),
                         p_x2=counts.data_ptr(), **dims),
               L.make_op(L.OP_VALID_FOLD, 0, npart=0, p_in=counts.data_ptr(), p_x0=loss.data_ptr(), p_out=self.buf.data_ptr(), **dims)]
        L.OpList(ops).run(h, torch.cuda.current_stream(self.device).cuda_stream)

    def compute(self) -> dict:
        return validation_report(self.buf.cpu().tolist(), self.C)


# the edges of a calibration pass that names none: coarse where a threshold is never chosen, fine towards 1
DEFAULT_CALIB_EDGES = (0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.85, 0.9, 0.925, 0.95, 0.97, 0.98, 0.99, 0.995, 0.999)


class CalibrationReport(dict):
    """The report of ``calibration_report``: a dict with one method."""

    def threshold(self, precision: float, cls=None):
        """The smallest edge at which the precision of the kept labelled pixels -- of class ``cls``, or of all classes -- reaches
        ``precision``; None when no edge does (a NaN precision, nothing kept, reaches nothing)."""
        row = self["all"]["precision"] if cls is None else [p[cls] for p in self["precision"]]
        for e, p in zip(self["edges"], row):
            if p >= precision:
                return e
        return None


def calibration_report(table, edges, num_class: int) -> CalibrationReport:
    """What a confidence threshold keeps, from the integers RCV_OP_CLS_CALIB counts: ``table`` int [K+1][C][C+3] (bin b holds the
    pixels whose confidence passes exactly b of the K ascending ``edges``; per predicted class: C label columns, column C = pixels
    without a label inside the classes, column C+1 / C+2 = the sum of (uint32)(confidence * 2^26) over the labelled / unlabelled ones).
    Everything is float64 arithmetic on the host; 0 / 0 is NaN (``_ratio``).
      per edge j and class c (lists [K][C]; the pixels predicted c with confidence >= edges[j] are those of the bins above j):
        ``kept`` labelled pixels, ``correct`` of them with label c, ``precision`` = correct / kept, ``coverage`` = kept / all labelled
        pixels predicted c, ``kept_unlabelled``; ``all``: the same five over all classes (lists [K])
      ``kept_confusion`` int64 [K][C][C]: [pred][label] counts of what survives edge j, as ``validation_report``'s ``confusion``
      ``bins``: per bin (lists [K+1]) ``count``, ``accuracy`` and ``mean_confidence`` (fixed-point sum / 2^26 / count) over the labelled
        pixels, ``lo`` / ``hi`` its confidence range [lo, hi), and ``per_class`` the same three as lists [K+1][C]
      ``ece`` = sum over the non-empty bins of (n_b / n) * |accuracy_b - mean_confidence_b| over the labelled pixels
      ``labelled`` / ``unlabelled``: pixels counted; ``threshold(precision, cls=None)``: see ``CalibrationReport``."""
    C = num_class
    edges = [float(e) for e in edges]
    K = len(edges)
    t = [[[int(v) for v in row] for row in plane] for plane in table]
    if len(t) != K + 1 or any(len(pl) != C or any(len(r) != C + 3 for r in pl) for pl in t):
        raise ValueError("calibration_report: the table must be [%d][%d][%d] for %d edges and %d classes" % (K + 1, C, C + 3, K, C))
    scale = float(L.CALIB_Q_SCALE)
    n_bc = [[sum(t[b][c][:C]) for c in range(C)] for b in range(K + 1)]              # labelled pixels per bin and predicted class
    ok_bc = [[t[b][c][c] for c in range(C)] for b in range(K + 1)]
    pred_c = [sum(n_bc[b][c] for b in range(K + 1)) for c in range(C)]
    n = sum(pred_c)
    out = CalibrationReport(edges=edges, num_class=C, labelled=n, unlabelled=sum(t[b][c][C] for b in range(K + 1) for c in range(C)))
    kept, correct, unl, conf = [], [], [], []
    for j in range(K):
        above = range(j + 1, K + 1)
        kept.append([sum(n_bc[b][c] for b in above) for c in range(C)])
        correct.append([sum(ok_bc[b][c] for b in above) for c in range(C)])
        unl.append([sum(t[b][c][C] for b in above) for c in range(C)])
        conf.append([[sum(t[b][p][l] for b in above) for l in range(C)] for p in range(C)])
    out["kept"], out["correct"], out["kept_unlabelled"] = kept, correct, unl
    out["precision"] = [[_ratio(float(correct[j][c]), float(kept[j][c])) for c in range(C)] for j in range(K)]
    out["coverage"] = [[_ratio(float(kept[j][c]), float(pred_c[c])) for c in range(C)] for j in range(K)]
    a_kept, a_ok = [sum(r) for r in kept], [sum(r) for r in correct]
    out["all"] = {"kept": a_kept, "correct": a_ok, "kept_unlabelled": [sum(r) for r in unl],
                  "precision": [_ratio(float(a_ok[j]), float(a_kept[j])) for j in range(K)],
                  "coverage": [_ratio(float(a_kept[j]), float(n)) for j in range(K)]}
    out["kept_confusion"] = torch.tensor(conf, dtype=torch.int64).reshape(K, C, C)
    count = [sum(r) for r in n_bc]
    acc = [_ratio(float(sum(ok_bc[b])), float(count[b])) for b in range(K + 1)]
    mean = [_ratio(sum(t[b][c][C + 1] for c in range(C)) / scale, float(count[b])) for b in range(K + 1)]
    out["bins"] = {"lo": [float("-inf")] + edges, "hi": edges + [float("inf")], "count": count, "accuracy": acc, "mean_confidence": mean,
                   "per_class": {"count": n_bc,
                                 "accuracy": [[_ratio(float(ok_bc[b][c]), float(n_bc[b][c])) for c in range(C)] for b in range(K + 1)],
                                 "mean_confidence": [[_ratio(t[b][c][C + 1] / scale, float(n_bc[b][c])) for c in range(C)]
                                                     for b in range(K + 1)]}}
    ece = float("nan") if n == 0 else 0.0
    for b in range(K + 1):
        if count[b]:
            ece += count[b] / n * abs(acc[b] - mean[b])
    out["ece"] = ece
    return out


def calibration_edges(edges):
    """The edges of a ``CalibrationState`` as a float32 tensor on the host: 1..32 finite values in [0, 1], strictly ascending once
    rounded to fp32 (the device compares in fp32).  ValueError otherwise."""
    try:
        vals = [float(e) for e in edges]
    except (TypeError, ValueError):
        raise ValueError("calibration edges must be a sequence of numbers (got %r)" % (edges,))
    if not 1 <= len(vals) <= L.CALIB_MAX_EDGES:
        raise ValueError("calibration edges: %d values (1..%d)" % (len(vals), L.CALIB_MAX_EDGES))
    if any(v != v or v in (float("inf"), float("-inf")) or not 0.0 <= v <= 1.0 for v in vals):
        raise ValueError("calibration edges must be finite and in [0, 1] (got %r)" % (vals,))
    e32 = torch.tensor(vals, dtype=torch.float32)
    if len(vals) > 1 and not bool((e32[1:] > e32[:-1]).all()):
        raise ValueError("calibration edges must be strictly ascending once rounded to float32 (got %r)" % (vals,))
    return e32


class CalibrationState:
    """The running state of one calibration pass, kept on the device: the K confidence edges (fp32) and the int64 [K+1][C][C+3] table
    RCV_OP_CLS_CALIB accumulates into (``model.calibrate``, ``Trainer.calibrate``, ``update_from_maps``).  ``compute()`` is the one
    read-back; every figure of its report (``calibration_report``) comes from integers, so a pass is reproducible bit for bit."""

    def __init__(self, num_class: int, edges, device="cuda"):
        if not isinstance(num_class, int) or not 1 <= num_class <= 8:
            raise ValueError("CalibrationState counts 1..8 classes (got %r)" % (num_class,))
        e32 = calibration_edges(edges)
        self.C = num_class
        self.K = int(e32.numel())
        self.edges = [float(v) for v in e32.tolist()]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.RcvError("CalibrationState lives on the HIP device (got '%s'); there is no CPU path" % self.device)
        self.edges_dev = e32.to(self.device)
        self.buf = torch.zeros(self.K + 1, self.C, self.C + 3, dtype=torch.int64, device=self.device)
        self.device = self.buf.device

    def reset(self):
        self.buf.zero_()

    def update_from_maps(self, class_map_u8: torch.Tensor, confidence: torch.Tensor, targets=None):
        """A batch whose class map (uint8 [B,H,W]) and confidence map (float32 [B,H,W]) exist already -- ``LabelPropagator`` output, an
        average of several networks: RCV_OP_CLS_CALIB's map form.  A class byte >= C and a NaN confidence count nowhere."""
        if not torch.is_tensor(class_map_u8) or class_map_u8.dtype != torch.uint8 or class_map_u8.dim() != 3 or class_map_u8.device != self.device:
            raise L.RcvError("CalibrationState.update_from_maps needs the uint8 [B,H,W] class map on %s" % self.device)
        if (not torch.is_tensor(confidence) or confidence.dtype != torch.float32 or tuple(confidence.shape) != tuple(class_map_u8.shape)
                or confidence.device != self.device):
            raise L.RcvError("CalibrationState.update_from_maps: confidence must be float32 %s on %s" % (list(class_map_u8.shape), self.device))
        if targets is not None and (not torch.is_tensor(targets) or tuple(targets.shape) != tuple(class_map_u8.shape)):
            raise L.RcvError("CalibrationState.update_from_maps: targets must be [B,H,W] like the class map %s" % (tuple(class_map_u8.shape),))
        B, H, W = class_map_u8.shape
        class_map_u8, confidence = class_map_u8.contiguous(), confidence.contiguous()
        if targets is not None:
            targets = targets.to(self.device).to(torch.int64).contiguous()
        h = L.handle(self.device.index if self.device.index is not None else torch.cuda.current_device())
        op = L.make_op(L.OP_CLS_CALIB, 0, n=B, h=H, w=W, cin=1, cout=self.C, inmode=L.CLS_LABEL_CLASSMAP, count=self.K,
                       p_in=class_map_u8.data_ptr(), p_x1=confidence.data_ptr(), p_in2=targets.data_ptr() if targets is not None else 0,
                       p_x0=self.edges_dev.data_ptr(), p_x2=self.buf.data_ptr())
        L.OpList([op]).run(h, torch.cuda.current_stream(self.device).cuda_stream)

    def compute(self) -> CalibrationReport:
        return calibration_report(self.buf.cpu().tolist(), self.edges, self.C)


def patch_scores(conf) -> dict:
    """The figures objDetEval.py prints from its confusion matrix ``conf[pred, label]`` (integers): ``acc`` = the validation accuracy
    of objDetEval.py:156,164 (100 * #(pred == label) / #patches), and the three of objDetEval.py:171-179 over the object classes 1..3:
    ``obj_acc`` = totAcc / total * 100 with total = sum(conf[:, 1:4]) (patches whose LABEL is an object) and totAcc = the diagonal
    1..3, ``false_neg`` = 100 - obj_acc, ``false_pos`` = (sum(conf[1:4, :]) - totAcc) / total * 100.  Float64 on the host."""
    c = torch.as_tensor(conf).to(torch.int64).cpu()
    n = int(c.sum())
    total = int(c[:, 1:4].sum())
    tot_acc = int(c[1, 1] + c[2, 2] + c[3, 3])
    fp = int(c[1:4, :].sum()) - tot_acc
    nan = float("nan")
    obj = tot_acc / total * 100 if total else nan
    return {"acc": int(torch.diagonal(c).sum()) * 100 / n if n else nan, "obj_acc": obj, "false_neg": 100 - obj,
            "false_pos": fp / total * 100 if total else nan, "confusion": c}


class PatchMetrics:
    """The confusion matrix of the patch classifiers' validation loop (objDetEval.py:155-159: ``conf[(predClass[j], labels[j])] += 1``
    per sample, each a device read) accumulated on the device by RCV_OP_CONFUSION with one 1x1 "image" per patch; nothing is read
    back before ``compute``."""

    def __init__(self, num_class: int = 4, device="cuda"):
        if num_class < 4 or num_class > 8:
            raise ValueError("PatchMetrics reports the object classes 1..3: 4 <= num_class <= 8 (got %d)" % num_class)
        self.C = num_class
        self.device = torch.device(device)
        self.conf = None

    def reset(self):
        self.conf = None

    def update(self, pred_u8: torch.Tensor, labels: torch.Tensor):
        """pred_u8: uint8 [B] or [B,1,1] (``BNNL.predict`` / ``BNNMC.predict`` of 32x32 patches) on the HIP device; labels: int64 [B]."""
        if pred_u8.dtype != torch.uint8 or pred_u8.device.type != "cuda":
            raise L.RcvError("PatchMetrics.update needs the uint8 class of every patch on the HIP device")
        B = pred_u8.shape[0]
        if pred_u8.numel() != B or labels.numel() != B:
            raise ValueError("PatchMetrics.update takes one class and one label per patch: pred %s, labels %s" % (tuple(pred_u8.shape), tuple(labels.shape)))
        labels = labels.to(pred_u8.device).to(torch.int64).contiguous()
        counts = torch.zeros(B, self.C, self.C, dtype=torch.int32, device=pred_u8.device)
        h = L.handle(pred_u8.device.index if pred_u8.device.index is not None else torch.cuda.current_device())
        op = L.make_op(L.OP_CONFUSION, 0, n=B, h=1, w=1, cout=self.C, p_in=pred_u8.contiguous().data_ptr(), p_in2=labels.data_ptr(),
                       p_out=counts.data_ptr())
        L.OpList([op]).run(h, torch.cuda.current_stream(pred_u8.device).cuda_stream)
        s = counts.sum(0, dtype=torch.int64)
        self.conf = s if self.conf is None else self.conf + s

    def compute(self) -> dict:
        if self.conf is None:
            return patch_scores(torch.zeros(self.C, self.C, dtype=torch.int64))
        return patch_scores(self.conf)


DEFAULT_IOU_THRESHOLDS = (0.75, 0.5, 0.25, 0.1, 0.05)     # test.py:258
DEFAULT_DIST_THRESHOLDS = (1.25, 2.5, 5, 10, 20)          # test.py:259; test.py:261-262 doubles them for --noScale


def _elem_bytes(t: torch.Tensor, what: str, allowed) -> int:
    nbytes = {torch.uint8: 1, torch.int64: 8}.get(t.dtype)
    if nbytes is None or t.dtype not in allowed:
        raise L.RcvError("%s: dtype %s unsupported (%s)" % (what, t.dtype, " or ".join(str(a) for a in allowed)))
    return nbytes


class ObjectMatchRecord:
    """One RCV_OP_OBJECT_MATCH record and the host double[K] threshold arrays it points to (kept alive with it)."""

    def __init__(self, N: int, H: int, W: int, num_class: int, iou_thresholds, dist_thresholds, pred_bytes: int = 1,
                 target_bytes: int = 8):
        iou = [float(t) for t in iou_thresholds]
        dist = [float(d) for d in dist_thresholds]
        if len(iou) != len(dist):
            raise L.RcvError("object_match: %d IoU thresholds but %d distance thresholds" % (len(iou), len(dist)))
        self.K = len(iou)
        self.iou = (ctypes.c_double * max(self.K, 1))(*iou)
        self.dist = (ctypes.c_double * max(self.K, 1))(*dist)
        self.op = L.make_op(L.OP_OBJECT_MATCH, 0, n=N, h=H, w=W, cout=num_class, count=self.K, inmode=pred_bytes,
                            inmode2=target_bytes, p_x0=ctypes.addressof(self.iou), p_x1=ctypes.addressof(self.dist))

    def workspace_bytes(self, h) -> int:
        """rcv_op_workspace: refuses the record (RcvError with the library's message) exactly as an enqueue would."""
        return L.op_workspace(h, self.op)


def object_match_counts(pred: torch.Tensor, target: torch.Tensor, num_class: int, iou_thresholds=DEFAULT_IOU_THRESHOLDS,
                        dist_thresholds=DEFAULT_DIST_THRESHOLDS, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """The raw counts of RCV_OP_OBJECT_MATCH: int32 [N][C-1][2+2K] = {nPred, nTrue, nCorrIoU[K], nCorrDist[K]} per image and class
    1..C-1 (rcv.h rcv_object_match).  pred: uint8 (CrossEntropyLoss2d.last_argmax) or int64 (torch.max(pred,1)[1]) [N,H,W];
    target: int64 or uint8 [N,H,W]; both on the HIP device.  Enqueued on the current stream; nothing synchronises."""
    if pred.device.type != "cuda" or target.device.type != "cuda" or pred.device != target.device:
        raise L.RcvError("object_match_counts needs pred and target on one HIP device (there is no CPU path)")
    if pred.dim() != 3 or pred.shape != target.shape:
        raise L.RcvError("object_match_counts: pred %s and target %s must both be [N,H,W]" % (tuple(pred.shape), tuple(target.shape)))
    pb = _elem_bytes(pred, "object_match_counts pred", (torch.uint8, torch.int64))
    tb = _elem_bytes(target, "object_match_counts target", (torch.int64, torch.uint8))
    N, H, W = pred.shape
    pred, target = pred.contiguous(), target.contiguous()
    rec = ObjectMatchRecord(N, H, W, num_class, iou_thresholds, dist_thresholds, pb, tb)
    dev = pred.device
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    nbytes = rec.workspace_bytes(h)
    if workspace is None or workspace.numel() < nbytes or workspace.device != dev:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(N, num_class - 1, 2 + 2 * rec.K, dtype=torch.int32, device=dev)
    op = rec.op
    op.p[L.RCV_P_IN], op.p[L.RCV_P_IN2] = pred.data_ptr(), target.data_ptr()
    op.p[L.RCV_P_OUT], op.p[L.RCV_P_PART] = counts.data_ptr(), workspace.data_ptr()
    L.OpList([op]).run(h, torch.cuda.current_stream(dev).cuda_stream)
    return counts


def detection_scores(batches, num_class: int, K: int):
    """test.py's numbers from the counts of each update() (a list of int arrays [B][C-1][2+2K]): per batch and threshold pair,
    prec / recall summed over c (outer) and b (inner) in Python float64, batch value (prec/(C-1) + recall/(C-1))/2, summed over the
    batches (test.py:28-89,258-262).  Returns the two lists of sums [K] (IoU, distance); divide by the image count (test.py:183)."""
    sums = [[0.0] * K, [0.0] * K]
    for cnt in batches:
        rows = cnt.tolist()
        B = len(rows)
        for crit in range(2):
            for k in range(K):
                j = 2 + crit * K + k
                prec = 0.0
                rec = 0.0
                for c in range(num_class - 1):
                    for b in range(B):
                        n_pred, n_true, n_corr = rows[b][c][0], rows[b][c][1], rows[b][c][j]
                        prec += n_corr / n_pred if n_pred != 0 else 1
                        rec += n_corr / n_true if n_true != 0 else 1
                sums[crit][k] += (prec / (num_class - 1) + rec / (num_class - 1)) / 2
    return sums


class DetectionMetrics:
    """The `IoU:` / `Dist:` rows of test.py's validation.  update() enqueues one op per batch (the counts stay on the device);
    compute() synchronises once and returns {"iou": [K], "dist": [K], "images": n} with test.py's float64 values."""

    def __init__(self, num_class: int, iou_thresholds=DEFAULT_IOU_THRESHOLDS, dist_thresholds=DEFAULT_DIST_THRESHOLDS, device="cuda"):
        self.C = num_class
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.dist_thresholds = tuple(float(d) for d in dist_thresholds)
        self.K = len(self.iou_thresholds)
        self.device = torch.device(device)
        # the arguments are refused here, with the library's message, rather than at the first update
        ObjectMatchRecord(1, 1, 1, num_class, self.iou_thresholds, self.dist_thresholds).workspace_bytes(L.planner_handle())
        self._ws = None
        self.reset()

    def reset(self):
        self._counts = []
        self.n_img = 0

    def update(self, pred_class: torch.Tensor, targets: torch.Tensor):
        """pred_class: uint8 or int64 [B,H,W] class map on the HIP device; targets: int64 or uint8 [B,H,W]."""
        if pred_class.device.type != "cuda":
            raise L.RcvError("DetectionMetrics.update needs the class map on the HIP device (there is no CPU path)")
        if targets.device != pred_class.device:
            targets = targets.to(pred_class.device, non_blocking=True)
        B, H, W = pred_class.shape
        rec = ObjectMatchRecord(B, H, W, self.C, self.iou_thresholds, self.dist_thresholds)
        h = L.handle(pred_class.device.index if pred_class.device.index is not None else torch.cuda.current_device())
        need = rec.workspace_bytes(h)
        if self._ws is None or self._ws.numel() < need or self._ws.device != pred_class.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=pred_class.device)
        self._counts.append(object_match_counts(pred_class, targets, self.C, self.iou_thresholds, self.dist_thresholds, self._ws))
        self.n_img += B

    def compute(self) -> dict:
        if not self._counts:
            return {"iou": [0.0] * self.K, "dist": [0.0] * self.K, "images": 0}
        sizes = [c.shape[0] for c in self._counts]
        host = torch.cat(self._counts).cpu().numpy()        # the one synchronisation
        batches, at = [], 0
        for b in sizes:
            batches.append(host[at:at + b])
            at += b
        iou, dist = detection_scores(batches, self.C, self.K)
        return {"iou": [v / self.n_img for v in iou], "dist": [v / self.n_img for v in dist], "images": self.n_img}
