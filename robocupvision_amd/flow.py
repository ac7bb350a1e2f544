"""Label propagation by dense optical flow on the device (test.py:135-140 ``--lProp``; validLabelProp.py:108-114 ``--optFlow``).

    from robocupvision_amd.flow import propagate_labels, rgb_to_gray
    lp = propagate_labels(pred, rgb_to_gray(frames))      # pred [T,H,W] class maps of a sequence, frames uint8 [T,H,W,3]

``farneback_flow`` (RCV_OP_FARNEBACK) stands where transform.py:185-187 ``optFlow`` calls cv2.calcOpticalFlowFarneback, ``update_labels``
(RCV_OP_REMAP_LABELS) where transform.py:189-198 ``updateLabels`` calls cv2.remap; ``optFlow`` / ``updateLabels`` are the reference's
names with the reference's shapes.  The algorithm is the project's own statement of Farnebäck's method with OpenCV's parameter meanings
(tests/farneback_restatement.py): agreement with cv2 bit for bit is not claimed.  Everything runs on the HIP device, on the
current stream, without host synchronisation; there is no CPU path."""
from __future__ import annotations

import torch

from . import _lib as L
from .infer import _workspace

__all__ = ["farneback_flow", "update_labels", "propagate_labels", "rgb_to_gray", "optFlow", "updateLabels", "FlowRecord"]


class FlowRecord:
    """The RCV_OP_FARNEBACK record of B pairs of H x W frames with `channels` bytes per pixel; the library checks it (and sizes the
    workspace) in ``workspace_bytes``, which refuses everything outside the contract with the library's message."""

    def __init__(self, B, H, W, channels=1, pyr_scale=0.5, levels=2, winsize=15, iterations=2, poly_n=7, poly_sigma=1.5, flags=0):
        try:
            self.op = L.make_op(L.OP_FARNEBACK, n=B, h=H, w=W, cin=channels, count=levels, aux0=winsize, aux1=iterations, stride=poly_n,
                                dil=flags, f0=pyr_scale, f1=poly_sigma)
        except (TypeError, ValueError, OverflowError) as e:
            raise L.RcvError("farneback_flow: %s" % e) from None

    def workspace_bytes(self, h) -> int:
        return L.op_workspace(h, self.op)


def _device_index(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def farneback_flow(prev: torch.Tensor, next: torch.Tensor, pyr_scale=.5, levels=2, winsize=15, iterations=2, poly_n=7, poly_sigma=1.5,
                   flags=0) -> torch.Tensor:
    """Dense flow from ``prev`` to ``next``: uint8 [B,H,W] gray or [B,H,W,3] RGB (gray is formed on load) -> float32 [B,2,H,W], channel
    0 = dx (columns), 1 = dy (rows); [H,W] inputs give [2,H,W].  next(x) = prev(x - d) gives +d.  Enqueued on the current stream, nothing
    synchronises; the workspace is cached per shape (calls on one shape from several streams at once must not overlap).  Parameters
    outside the contract are refused with the library's message before anything is launched."""
    if not (isinstance(prev, torch.Tensor) and isinstance(next, torch.Tensor)) or prev.shape != next.shape:
        raise L.RcvError("farneback_flow: prev and next must be tensors of one shape")
    if prev.dtype != torch.uint8 or next.dtype != torch.uint8:
        raise L.RcvError("farneback_flow: uint8 frames expected, got %s / %s" % (prev.dtype, next.dtype))
    single = prev.dim() == 2
    if single:
        prev, next = prev[None], next[None]
    if prev.dim() == 4 and prev.shape[-1] == 3:
        ch = 3
    elif prev.dim() == 3:
        ch = 1
    else:
        raise L.RcvError("farneback_flow: frames must be [B,H,W] gray, [B,H,W,3] RGB or one [H,W] plane, got %s" % (tuple(prev.shape),))
    B, H, W = prev.shape[:3]
    rec = FlowRecord(B, H, W, ch, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    if prev.device.type != "cuda" or next.device != prev.device:
        rec.workspace_bytes(L.planner_handle())       # bad arguments are refused with the library's message first
        raise L.RcvError("farneback_flow needs both frames on one HIP device (there is no CPU path)")
    dev = prev.device
    h = L.handle(_device_index(prev))
    ws = _workspace(dev, ("flow", B, H, W, levels), rec.workspace_bytes(h))
    prev, next = prev.contiguous(), next.contiguous()
    flow = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
    op = rec.op
    op.p[L.RCV_P_IN], op.p[L.RCV_P_IN2], op.p[L.RCV_P_OUT], op.p[L.RCV_P_PART] = prev.data_ptr(), next.data_ptr(), flow.data_ptr(), ws.data_ptr()
    L.OpList([op]).run(h, torch.cuda.current_stream(dev).cuda_stream)
    return flow[0] if single else flow


def update_labels(labels: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """labels uint8 or int64 [N,H,W] (or [H,W]) moved through flow float32 [N,2,H,W] (or [2,H,W]): out[y,x] = labels[rint(y + flow[1]),
    rint(x + flow[0])] inside the plane, 0 outside.  A new tensor of the labels' dtype."""
    if not (isinstance(labels, torch.Tensor) and isinstance(flow, torch.Tensor)):
        raise L.RcvError("update_labels: tensors expected")
    single = labels.dim() == 2
    if single:
        labels, flow = labels[None], flow[None] if flow.dim() == 3 else flow
    if labels.dim() != 3 or flow.dim() != 4 or flow.shape != (labels.shape[0], 2) + tuple(labels.shape[1:]):
        raise L.RcvError("update_labels: labels [N,H,W] and flow [N,2,H,W] expected, got %s and %s" % (tuple(labels.shape), tuple(flow.shape)))
    if flow.dtype != torch.float32:
        raise L.RcvError("update_labels: float32 flow expected, got %s" % flow.dtype)
    eb = {torch.uint8: 1, torch.int64: 8}.get(labels.dtype)
    if eb is None:
        raise L.RcvError("update_labels: dtype %s unsupported (torch.uint8 or torch.int64)" % labels.dtype)
    N, H, W = labels.shape
    op = L.make_op(L.OP_REMAP_LABELS, n=N, h=H, w=W, inmode=eb)
    if labels.device.type != "cuda" or flow.device != labels.device:
        L.op_workspace(L.planner_handle(), op)
        raise L.RcvError("update_labels needs labels and flow on one HIP device (there is no CPU path)")
    dev = labels.device
    labels, flow = labels.contiguous(), flow.contiguous()
    out = torch.empty_like(labels)
    op.p[L.RCV_P_IN], op.p[L.RCV_P_IN2], op.p[L.RCV_P_OUT] = labels.data_ptr(), flow.data_ptr(), out.data_ptr()
    L.OpList([op]).run(L.handle(_device_index(labels)), torch.cuda.current_stream(dev).cuda_stream)
    return out[0] if single else out


def rgb_to_gray(rgb: torch.Tensor) -> torch.Tensor:
    """cv2.COLOR_RGB2GRAY on uint8 [...,3] (dataset.py:265): (4899 R + 9617 G + 1868 B + 8192) >> 14.  Integer torch ops on the tensor's
    device; ``farneback_flow`` forms the same bytes itself when it is given RGB frames."""
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() < 1 or rgb.shape[-1] != 3:
        raise L.RcvError("rgb_to_gray: a uint8 [...,3] tensor expected")
    c = rgb.to(torch.int32)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).to(torch.uint8)


def propagate_labels(pred: torch.Tensor, gray: torch.Tensor, **params) -> torch.Tensor:
    """test.py:135-140 for a sequence [T,H,W] or a batch of sequences [S,T,H,W], T >= 2: out[0] = update_labels(pred[1], flow(g0 -> g1)),
    out[i] = update_labels(out[i-1], flow(g_i -> g_{i-1})).  ``gray``: uint8 frames of pred's shape (or with a trailing RGB axis).  All
    S*T flows are one batched call; the T remaps are chained, each over the S sequences at once.  ``params``: farneback_flow's."""
    if not (isinstance(pred, torch.Tensor) and isinstance(gray, torch.Tensor)):
        raise L.RcvError("propagate_labels: tensors expected")
    single = pred.dim() == 3
    if single:
        pred, gray = pred[None], gray[None]
    if pred.dim() != 4 or pred.shape[1] < 2 or tuple(gray.shape[:4]) != tuple(pred.shape) or gray.dim() not in (4, 5):
        raise L.RcvError("propagate_labels: pred [T,H,W] or [S,T,H,W] with T >= 2 and frames of the same shape expected, got %s and %s"
                         % (tuple(pred.shape), tuple(gray.shape)))
    S, T, H, W = pred.shape
    dst = torch.cat([gray[:, 1:2], gray[:, :-1]], 1)                    # flow i runs from frame i to frame 1 (i = 0) or frame i - 1
    tail = tuple(gray.shape[4:])
    flow = farneback_flow(gray.reshape((S * T, H, W) + tail), dst.reshape((S * T, H, W) + tail), **params).view(S, T, 2, H, W)
    out = torch.empty_like(pred)
    cur = pred[:, 1]
    for i in range(T):
        cur = update_labels(cur, flow[:, i])
        out[:, i] = cur
    return out[0] if single else out


def optFlow(imgp: torch.Tensor, imgn: torch.Tensor) -> torch.Tensor:
    """transform.py:185-187: two gray uint8 [H,W] frames -> flow [2,H,W] with the reference's parameters."""
    return farneback_flow(imgp, imgn, pyr_scale=0.5, levels=2, winsize=15, iterations=2, poly_n=7, poly_sigma=1.5, flags=0)


def updateLabels(oldLab: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """transform.py:189-198: a class map [H,W] and a flow [2,H,W] -> the moved class map as int64 [H,W]."""
    return update_labels(oldLab, flow).long()
