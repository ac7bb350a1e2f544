"""Drop-in counterpart of the reference's ``model`` module for the ROBO-UNet / U-Net hot path.

Same public names, constructor arguments, sub-module names, ``state_dict`` keys and parameter
order as the reference (model.py:76-124, 166-199, 379-414, 461-567), so a caller written against
``from model import *`` (train.py:3,13; test.py:14; detect.py:13) keeps working -- but ``forward``
and ``backward`` run as hand-written HIP kernels on gfx950 through librcv.so (see engine.py).

The ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.ConvTranspose2d`` children exist only as parameter
containers (identical construction order => identical random init for a given seed, identical
state_dict); their own ``forward`` is never used.  There is no CPU path: calling a module on a
CPU tensor raises.
"""
from __future__ import annotations

from typing import List, Optional

import os

import torch
import torch.nn as nn

from . import _lib as L
from .engine import Engine
from .bnn import BNNL, BNNMC      # the reference's model.py:569-619 (kernels: csrc/bnn.hip)

__all__ = ["ROBO_UNet", "CrossEntropyLoss2d", "DiceLoss", "PB_FCN", "PB_FCN_2", "LabelProp", "Conv", "Pool", "LevelDown",
           "labelprop_batch", "labelprop_next", "upSampleTransposeConv", "UltClassifier", "ConvPoolSimple", "ConvPool", "DownSampler", "Classifier", "pruneModelNew",
           "count_zero_weights", "getParamSize", "BNNL", "BNNMC", "pruneModel", "pruneModel2",
           "View", "ConvPoolDouble", "DownSamplerThick", "FCN", "ConvSep", "trConvSep"]


# ------------------------------------------------------------------------------------------
# autograd glue: one node for the whole network
# ------------------------------------------------------------------------------------------
class _EngineFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine: Engine, training: bool, n_inputs: int, *tensors):
        inputs = [t.detach() for t in tensors[:n_inputs]]
        out = engine.forward(inputs, training, fresh_out=not training and not ALIAS_OUTPUTS)
        ctx.engine = engine
        ctx.generation = engine._generation
        ctx.n_inputs = n_inputs
        ctx.n_params = len(tensors) - n_inputs
        return out

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        fl = eng.flat
        # a parameter whose .grad already aliases the engine's gradient buffer is about to be
        # overwritten: detach it first so autograd's accumulation keeps its meaning
        base, end = fl.grad.data_ptr(), fl.grad.data_ptr() + 4 * fl.numel
        for p in fl.params:
            if p.grad is not None and base <= p.grad.data_ptr() < end:
                p.grad = p.grad.clone()
        plan = eng.backward(grad_out, ctx.generation)
        in_grads = []
        for k in range(ctx.n_inputs):
            g = plan.input_grads[k] if ctx.needs_input_grad[3 + k] else None
            in_grads.append(g)
        # parameters the graph never reads (PB_FCN's pooled classification head) keep grad None, as under the reference's autograd
        p_grads = [fl.grad_view(k) if eng.param_used[k] else None for k in range(ctx.n_params)]
        return (None, None, None, *in_grads, *p_grads)


# The engine writes its result into a buffer it owns and overwrites at the next forward of the same shape.  The reference's modules
# return a fresh tensor every call (a caller may keep predictions across iterations), so by default the module surface hands out a
# copy (one extra pass over the logits: 0.08 ms at 32 x 5 x 480 x 640).  ALIAS_OUTPUTS = True (or RCV_ALIAS_OUTPUTS=1) returns the
# engine's buffer itself: valid until the next forward of the same shape.  (Trainer.step's fused path never goes through here.)
ALIAS_OUTPUTS = bool(os.environ.get("RCV_ALIAS_OUTPUTS"))


def _run_engine(engine: Engine, training: bool, inputs: List[torch.Tensor]) -> torch.Tensor:
    out = _EngineFunction.apply(engine, training, len(inputs), *inputs, *engine.param_list)
    # (an inference pass wrote its result into a fresh tensor already: Engine.forward(fresh_out=True))
    return out if (ALIAS_OUTPUTS or not training) else out.clone()


def _bn_modules(m: nn.Module):
    return [x for x in m.modules() if isinstance(x, nn.BatchNorm2d)]


def _graph_mode(m: nn.Module) -> bool:
    """What the engine's graph depends on beyond the module tree: PB_FCN / PB_FCN_2 read ``classify`` at every forward
    (model.py:294, 450), so a change of it after construction must reach the next forward."""
    return bool(getattr(m, "classify", False))


class _EngineOwner:
    """Mixed into every module that can own an Engine.  The engine caches, per eval plan, everything that depends on the parameters
    only (packed filters, BatchNorm constants) and re-derives it when it can SEE a change: its own kernels wrote parameters
    (``params_dirty``) or a torch in-place op bumped a tensor's version counter.  Writes through ``.data`` (``p.data.mul_()``, the
    reference's ``pruneModel``: ``param = param.data; param[...] = 0``, model.py:626-640) bump no counter, so the cache is ALSO dropped
    at every ``.train()`` / ``.eval()`` call and after ``load_state_dict`` -- the reference's scripts call ``model.eval()`` at the top
    of every validation pass (train.py:104, trainer.py:162-171).  A caller that edits ``.data`` BETWEEN two eval-mode forwards without
    calling ``.eval()`` again must call ``invalidate()`` itself."""

    def invalidate(self):
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.invalidate()

    def train(self, mode: bool = True):
        self.invalidate()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate()
        return out

    def predict(self, x, colour=False, palette=None):
        """The class of every pixel, on the device, without the logits (detect.py:131-133: ``model(x)``, ``torch.max(pred, 1)``,
        ``Colorize``).  ``x`` as for ``forward``.  Returns a fresh uint8 [N,H,W] tensor -- what ``SegmentationMetrics.update`` and
        ``DetectionMetrics.update`` take -- or, with ``colour=True``, ``(labels, colour)`` with ``colour`` uint8 [N,H,W,3] =
        ``palette[labels]``.  ``palette``: uint8 [k,3], k <= 8 (missing rows are black); default: the reference's five rows
        (``labelcolormap``).  The class is the FIRST maximum of the logits ``self(x)`` writes in eval mode, bit for bit (RCV_OP_CLS_LABEL:
        the same kernels' arithmetic with another tail).  Runs under ``torch.no_grad()``; eval mode only."""
        from .palette import device_palette
        if self.training:
            raise L.RcvError("predict is an inference call and this module is in training mode: call `.eval()` first")
        if _graph_mode(self):
            raise L.RcvError("predict: this model is in classify mode (the pooled patch-classification head gives one class per patch, "
                             "not a class map); build it with classify off")
        if not hasattr(self, "_get_engine"):
            raise L.RcvError("predict: %s has no per-pixel classifier (ROBO_UNet, PB_FCN, PB_FCN_2 and LabelProp have)" % type(self).__name__)
        if not torch.is_tensor(x):
            raise TypeError("predict: x must be a tensor")
        if x.device.type != "cuda":
            raise L.RcvError("predict runs on the HIP device only (input on %s); there is no CPU path" % x.device)
        with torch.no_grad():
            inputs = self._engine_inputs(x)
            pal = device_palette(palette, x.device) if colour else None
            return self._get_engine().predict(inputs, bool(colour), pal)

    def validate(self, x, targets, state, weight=None, labels=False):
        """One batch of valid() (train.py:114-153) on the device: the forward, ``CrossEntropyLoss2d(weight)(self(x), targets)``,
        ``torch.max(pred, 1)`` and the per-image (pred, label) counts in one pass whose classifier tail keeps the logits in registers
        (RCV_OP_CLS_VALID), folded into ``state`` (``metrics.ValidationState``) by RCV_OP_VALID_FOLD.  ``x`` as for ``forward``;
        ``targets`` int64 [N,H,W]; ``weight`` float32 [C] or None.  Returns None, or with ``labels=True`` the class map as a fresh uint8
        [N,H,W] tensor -- ``predict``'s, bit for bit, what ``DetectionMetrics.update`` takes.  The batch loss booked in the state is bit
        for bit ``float(CrossEntropyLoss2d(weight)(self(x), targets))`` for every network but LabelProp (four lanes share a pixel of its
        16-channel tail: equal to rounding).  Nothing synchronises before ``state.compute()``.  Eval mode only, as ``predict``."""
        if self.training:
            raise L.RcvError("validate is an inference call and this module is in training mode: call `.eval()` first")
        if _graph_mode(self):
            raise L.RcvError("validate: this model is in classify mode (the pooled patch-classification head gives one class per patch, "
                             "not a class map); build it with classify off")
        if not hasattr(self, "_get_engine"):
            raise L.RcvError("validate: %s has no per-pixel classifier (ROBO_UNet, PB_FCN, PB_FCN_2 and LabelProp have)" % type(self).__name__)
        if not torch.is_tensor(x) or not torch.is_tensor(targets):
            raise TypeError("validate: x and targets must be tensors")
        if x.device.type != "cuda" or targets.device.type != "cuda":
            raise L.RcvError("validate runs on the HIP device only (input on %s, targets on %s); there is no CPU path" % (x.device, targets.device))
        if not hasattr(state, "counts_for") or not hasattr(state, "buf"):
            raise TypeError("validate: state must be a metrics.ValidationState")
        with torch.no_grad():
            inputs = self._engine_inputs(x)
            if weight is not None:
                weight = torch.as_tensor(weight, dtype=torch.float32, device=x.device).contiguous()
            return self._get_engine().validate(inputs, targets.to(torch.int64).contiguous(), weight, state, bool(labels))

    def proba(self, x, labels=False, confidence=False, min_confidence=None):
        """The class probabilities of every pixel, on the device, without the logits: what the robot's engine outputs (every exported
        ``net.cfg`` ends in ``[softmax]``).  ``x`` as for ``forward``.  Returns a fresh float32 [N,C,H,W] tensor, softmax over the
        classes of the logits ``self(x)`` writes in eval mode with the arithmetic fixed (RCV_OP_CLS_PROBA: first maximum m,
        ``expf(z - m)``, sum in class order, IEEE division) -- or a tuple of it and, in this order, what is asked for: ``labels=True``
        the class map uint8 [N,H,W] (``predict``'s, bit for bit), ``confidence=True`` float32 [N,H,W], the probability of that class,
        ``min_confidence=tau`` the pseudo-label int64 [N,H,W]: the class where confidence >= tau, else -100, usable as the targets
        of ``Trainer.step`` (the losses ignore labels outside [0, C)).  Nothing synchronises.  Eval mode only, refusals as ``predict``."""
        return self._proba_call(x, bool(labels), bool(confidence), None if min_confidence is None else float(min_confidence), True)

    def _proba_maps(self, x, min_confidence):
        """(class map, pseudo-label) of ``proba`` without the probabilities (``infer.Segmenter(pseudo_labels=tau)``)."""
        return self._proba_call(x, True, False, float(min_confidence), False)

    def _proba_call(self, x, labels, confidence, min_confidence, probabilities):
        if self.training:
            raise L.RcvError("proba is an inference call and this module is in training mode: call `.eval()` first")
        if _graph_mode(self):
            raise L.RcvError("proba: this model is in classify mode (the pooled patch-classification head gives one class per patch, "
                             "not a class map); build it with classify off")
        if not hasattr(self, "_get_engine"):
            raise L.RcvError("proba: %s has no per-pixel classifier (ROBO_UNet, PB_FCN, PB_FCN_2 and LabelProp have)" % type(self).__name__)
        if not torch.is_tensor(x):
            raise TypeError("proba: x must be a tensor")
        if x.device.type != "cuda":
            raise L.RcvError("proba runs on the HIP device only (input on %s); there is no CPU path" % x.device)
        with torch.no_grad():
            return self._get_engine().proba(self._engine_inputs(x), labels, confidence, min_confidence, probabilities)

    def calibrate(self, x, state, targets=None):
        """One batch of a confidence calibration pass on the device: the forward, then the class and the softmax confidence of every
        pixel -- ``proba``'s, bit for bit -- counted into ``state`` (``metrics.CalibrationState``) by predicted class, label and
        confidence bin (RCV_OP_CLS_CALIB as the classifier's tail).  ``x`` as for ``forward``; ``targets`` int64 [N,H,W], or None for
        frames without labels (every pixel counts as unlabelled, as a target outside [0, C) does).  For every edge tau of the state the
        labelled pixels counted above it are exactly those ``proba(min_confidence=tau)`` keeps.  Nothing per pixel is stored and nothing
        synchronises before ``state.compute()``.  Returns None.  Eval mode only, refusals as ``predict``."""
        if self.training:
            raise L.RcvError("calibrate is an inference call and this module is in training mode: call `.eval()` first")
        if _graph_mode(self):
            raise L.RcvError("calibrate: this model is in classify mode (the pooled patch-classification head gives one class per patch, "
                             "not a class map); build it with classify off")
        if not hasattr(self, "_get_engine"):
            raise L.RcvError("calibrate: %s has no per-pixel classifier (ROBO_UNet, PB_FCN, PB_FCN_2 and LabelProp have)" % type(self).__name__)
        if not torch.is_tensor(x) or not (targets is None or torch.is_tensor(targets)):
            raise TypeError("calibrate: x and targets must be tensors (targets may be None)")
        if x.device.type != "cuda" or (targets is not None and targets.device.type != "cuda"):
            raise L.RcvError("calibrate runs on the HIP device only (input on %s%s); there is no CPU path"
                             % (x.device, "" if targets is None else ", targets on %s" % targets.device))
        if not hasattr(state, "edges_dev") or not hasattr(state, "buf"):
            raise TypeError("calibrate: state must be a metrics.CalibrationState")
        with torch.no_grad():
            if targets is not None:
                targets = targets.to(torch.int64).contiguous()
            self._get_engine().calibrate(self._engine_inputs(x), state, targets)


class _BlockMixin(_EngineOwner):
    """Standalone call of a single block (NCHW in, NCHW out like the reference's blocks): the block
    becomes a one-node graph with an NHWC input and a materialised output."""

    def _block_graph(self):
        raise NotImplementedError

    def _block_forward(self, *xs: torch.Tensor) -> torch.Tensor:
        eng = self.__dict__.get("_engine")
        if eng is None:
            graph = self._block_graph()
            eng = Engine(graph, list(self.parameters()), _bn_modules(self))
            self.__dict__["_engine"] = eng
        ins = [x.permute(0, 2, 3, 1).contiguous() for x in xs]
        y = _run_engine(eng, self.training, ins)
        return y.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------
# building blocks (reference: model.py:92-124, 166-199, 379-414)
# ------------------------------------------------------------------------------------------
class Pool(_BlockMixin, nn.Module):
    """MaxPool2d(2,2) (model.py:92-103).  Parameter-free; inside a network it is fused with the
    producer's BatchNorm apply; called on its own (NCHW in, NCHW out, like the reference's module) it is a one-node graph."""

    def __init__(self, ch, stride=2):
        super().__init__()
        if stride != 2:
            raise NotImplementedError("only the 2x2/2 max-pool of the reference networks is built")
        self.ch = ch
        self.stride = stride
        self.pool = nn.MaxPool2d(stride, stride)     # container for repr/state parity only

    def _block_graph(self):
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}], "nodes": [{"op": "pool", "src": ("in", 0)}]}

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] % 4 or x.shape[2] % 2 or x.shape[3] % 2:
            raise ValueError("Pool expects float32 [B,C,H,W] with C a multiple of 4 and even H, W (got %s)" % (tuple(x.shape),))
        return self._block_forward(x.to(torch.float32))

    def getComp(self, W, H, pruned):
        return W * H * self.ch, W // self.stride, H // self.stride


class Conv(_BlockMixin, nn.Module):
    """bn(relu(conv3x3(x))) -- ReLU before BatchNorm (model.py:105-124)."""

    def __init__(self, inplanes, planes, size, stride=1):
        super().__init__()
        if size != 3:
            raise NotImplementedError("only 3x3 Conv blocks are built (reference networks use size=3)")
        self.stride = stride
        self.size = size
        self.inch = inplanes
        self.ch = planes
        self.conv = nn.Conv2d(inplanes, planes, kernel_size=size, padding=size // 2, stride=stride)
        self.bn = nn.BatchNorm2d(planes)

    def _node(self, src):
        return {"op": "conv", "src": src, "weight": self.conv.weight, "bias": self.conv.bias, "bn": self.bn,
                "stride": self.stride, "dil": 1, "order": "relu_bn"}

    def _block_graph(self):
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}],
                "nodes": [self._node(("in", 0)), {"op": "mat", "src": ("node", 0)}]}

    def forward(self, x):
        return self._block_forward(x)

    def getComp(self, W, H, pruned):
        W = W // self.stride
        H = H // self.stride
        ratio = float(self.conv.weight.nonzero().size(0)) / float(self.conv.weight.numel()) if pruned else 1
        return self.size * self.size * W * H * self.inch * self.ch * 2 * ratio + W * H * self.ch * 4, W, H


class ConvPoolSimple(_BlockMixin, nn.Module):
    """relu(bn(conv(x))) with dilation (model.py:166-176): LabelProp inference and the PB_FCN encoder."""

    def __init__(self, inplanes, planes, size, stride, padding, dilation, bias, *_ignored):
        super().__init__()
        if size != 3 or padding != dilation:
            raise NotImplementedError("ConvPoolSimple is built for 3x3 kernels with padding == dilation")
        self.stride, self.dilation = stride, dilation
        self.conv = nn.Conv2d(inplanes, planes, size, stride=stride, padding=padding, dilation=dilation, bias=bias)
        self.bn = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU()

    def _node(self, src):
        return {"op": "conv", "src": src, "weight": self.conv.weight, "bias": self.conv.bias, "bn": self.bn,
                "stride": self.stride, "dil": self.dilation, "order": "bn_relu"}

    def _block_graph(self):
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}],
                "nodes": [self._node(("in", 0)), {"op": "mat", "src": ("node", 0)}]}

    def forward(self, x):
        return self._block_forward(x)


class ConvPool(_BlockMixin, nn.Module):
    """relu(bn(pool(relu(conv1(x))))): a dilated 3x3 conv, then a stride-2 3x3 conv as the 'pool' (model.py:126-142)."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.relu = nn.ReLU()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, dilation=2, padding=2, bias=False)
        self.pool = nn.Conv2d(planes, planes, kernel_size=3, padding=1, stride=2, bias=False)
        self.bn = nn.BatchNorm2d(planes)

    def _nodes(self, nodes: list, src):
        nodes.append({"op": "conv", "src": src, "weight": self.conv1.weight, "bias": None, "bn": None, "stride": 1, "dil": 2,
                      "order": "relu"})
        nodes.append({"op": "conv", "src": ("node", len(nodes) - 1), "weight": self.pool.weight, "bias": None, "bn": self.bn,
                      "stride": 2, "dil": 1, "order": "bn_relu"})
        return ("node", len(nodes) - 1)

    def _block_graph(self):
        nodes: list = []
        out = self._nodes(nodes, ("in", 0))
        nodes.append({"op": "mat", "src": out})
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}], "nodes": nodes}

    def forward(self, x):
        return self._block_forward(x)


class upSampleTransposeConv(_BlockMixin, nn.Module):
    """relu(bn(ConvTranspose2d(k3,s2,p1,op1)(x))) (model.py:178-199)."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.stride = 2
        self.size = 3
        self.inch = inplanes
        self.ch = planes
        self.relu = nn.ReLU()
        self.conv = nn.ConvTranspose2d(inplanes, planes, kernel_size=3, padding=1, stride=2, output_padding=1, bias=True)
        self.bn = nn.BatchNorm2d(planes)

    def _node(self, src, skip, concat=False):
        return {"op": "up", "src": src, "skip": skip, "concat": concat, "weight": self.conv.weight, "bias": self.conv.bias,
                "bn": self.bn}

    def _block_graph(self):
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}],
                "nodes": [self._node(("in", 0), None), {"op": "mat", "src": ("node", 0)}]}

    def forward(self, x):
        return self._block_forward(x)

    def getComp(self, W, H, pruned):
        ratio = float(self.conv.weight.nonzero().size(0)) / float(self.conv.weight.numel()) if pruned else 1
        return self.size * self.size * W * H * self.inch * self.ch * 2 * ratio + W * H * self.ch * 4, W * self.stride, H * self.stride


class LevelDown(nn.Module):
    """One encoder level (model.py:379-401): [Pool], Conv0 (stride 2 when downsampling without
    pooling), Conv1.. ; children are named exactly like the reference (state_dict keys)."""

    def __init__(self, inplanes, planes, levels, doPool, pool=False):
        super().__init__()
        self.layers = nn.Sequential()
        first_stride = 1
        if pool:
            if doPool:
                self.layers.add_module("Pool", Pool(inplanes, 2))
                levels -= 1
        elif doPool:
            first_stride = 2
        self.layers.add_module("Conv0", Conv(inplanes, planes, 3, stride=first_stride))
        for i in range(levels - 1):
            self.layers.add_module("Conv%d" % (i + 1), Conv(planes, planes, 3))

    def _nodes(self, nodes: list, src):
        """Append this level's nodes; returns the reference of its output."""
        for m in self.layers:
            if isinstance(m, Pool):
                nodes.append({"op": "pool", "src": src})
            else:
                nodes.append(m._node(src))
            src = ("node", len(nodes) - 1)
        return src

    def forward(self, x):
        for m in self.layers:
            x = m(x)
        return x


POOLED_5X5 = ("the pooled patch-classification heads are built for a 1x1 classifier; a 5x5 classifier behind the pool is not built "
              "(classTrainer.py uses kernel size 1)")


class UltClassifier(nn.Module):
    """1x1 (or, for the v2 net, 3x3) classifier (model.py:403-414).  The pooled variant (AdaptiveAvgPool2d(1), Dropout2d, 1x1
    classifier: PB_FCN_2.classifier) is the patch-classification head of classTrainer.py, run as PB_FCN_2(classify=True)'s graph."""

    def __init__(self, inplanes, nClass, pool, dropout=0.5, size=1):
        super().__init__()
        if size not in (1, 3, 5):
            raise NotImplementedError("classifier kernel sizes 1, 3 and 5 are built (got %d)" % size)
        if pool and size == 5:
            raise NotImplementedError(POOLED_5X5)
        self.pooled = bool(pool)
        self.layers = nn.Sequential()
        if pool:        # patch-classification head (PB_FCN_2.classifier): the containers hold the parameters and the dropout rate
            self.layers.add_module("Pool", nn.AdaptiveAvgPool2d(1))
            self.layers.add_module("DO", nn.Dropout2d(dropout))
        self.layers.add_module("Class", nn.Conv2d(inplanes, nClass, size, padding=size // 2))

    def _node(self, src):
        if self.pooled:
            raise L.RcvError("the pooled classification head (classify=True) is outside the segmentation path")
        c = self.layers.Class
        return {"op": "cls", "src": src, "weight": c.weight, "bias": c.bias}

    def _head_node(self, src):
        """The pooled head as the graph's last node (model.py:444-453): plane mean, Dropout2d(DO.p), 1x1 classifier."""
        if not self.pooled:
            raise L.RcvError("this UltClassifier has no pooled head")
        c = self.layers.Class
        return {"op": "pool_cls", "src": src, "pool": ("avg",), "weight": c.weight, "bias": c.bias, "dropout": float(self.layers.DO.p)}

    def forward(self, x):
        raise L.RcvError("UltClassifier is executed as part of its network graph; standalone use is not built")


# ------------------------------------------------------------------------------------------
# ROBO_UNet (model.py:461-536)
# ------------------------------------------------------------------------------------------
class ROBO_UNet(_EngineOwner, nn.Module):
    def __init__(self, noScale=False, planes=8, nClass=5, depth=4, levels=2, bellySize=5, bellyPlanes=128, pool=False, v2=False,
                 classSize=1):
        super().__init__()
        self.numClass = nClass
        self.planes = planes
        self.v2 = v2
        self.img_shape = (240, 320) if noScale else (120, 160)
        if noScale:
            depth += 1
        maxDepth = planes * pow(2, depth - 1)

        self.downPart = nn.ModuleList()
        self.downPart.add_module("Level0", LevelDown(3, planes, levels - 1, False, pool))
        for i in range(depth - 1):
            nCh = planes * pow(2, i)
            self.downPart.add_module("Level%d" % (i + 1), LevelDown(nCh, nCh * 2, levels, True, pool))

        self.PB = nn.Sequential()
        if bellySize > 0:
            self.PB.add_module("PB_1", LevelDown(maxDepth, bellyPlanes, bellySize - 1, False))
            self.PB.add_module("PB_2", LevelDown(bellyPlanes, maxDepth, 1, False))

        self.upPart = nn.ModuleList()
        for i in range(depth - 1):
            nCh = planes * pow(2, depth - 1 - i)
            oCh = nCh // 2
            if i > 0 and v2:      # v2: the previous level's output is concatenated with its skip tensor (model.py:487-488,507)
                nCh *= 2
            self.upPart.add_module("Up%d" % i, upSampleTransposeConv(nCh, oCh))

        self.segmenter = UltClassifier(planes * 2 if v2 else planes, nClass, False, size=classSize)

    # graph of model.py:495-511
    def _graph(self):
        nodes: list = []
        downs = [("in", 0)]
        for level in self.downPart:
            downs.append(level._nodes(nodes, downs[-1]))
        for level in self.PB:
            downs[-1] = level._nodes(nodes, downs[-1])
        up = downs[-1]
        for i, layer in enumerate(self.upPart):
            nodes.append(layer._node(up, downs[-(i + 2)], concat=self.v2))
            up = ("node", len(nodes) - 1)
        nodes.append(self.segmenter._node(up))
        return {"inputs": [{"layout": "nchw"}], "nodes": nodes}

    def _get_engine(self) -> Engine:
        eng = self.__dict__.get("_engine")
        mode = _graph_mode(self)
        if eng is None or self.__dict__.get("_engine_mode") != mode:
            eng = Engine(self._graph(), list(self.parameters()), _bn_modules(self))
            self.__dict__["_engine"] = eng
            self.__dict__["_engine_mode"] = mode
        return eng

    def _engine_inputs(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("ROBO_UNet expects float32 [B,3,H,W], got %s" % (tuple(x.shape),))
        down = 2 ** (len(self.downPart) - 1)
        if x.shape[2] % down or x.shape[3] % down:
            raise ValueError("H and W must be multiples of %d (got %dx%d)" % (down, x.shape[2], x.shape[3]))
        return [x.to(torch.float32).contiguous()]

    def forward(self, x):
        return _run_engine(self._get_engine(), self.training, self._engine_inputs(x))

    def get_computations(self, pruned=False):
        """Analytic per-layer operation counts (model.py:513-536); host arithmetic only."""
        H, W = self.img_shape
        computations = []
        for part in self.downPart:
            for module in part.layers:
                comp, W, H = module.getComp(W, H, pruned)
                computations.append(comp)
        for part in self.PB:
            for module in part.layers:
                comp, W, H = module.getComp(W, H, pruned)
                computations.append(comp)
        for module in self.upPart:
            comp, W, H = module.getComp(W, H, pruned)
            computations.append(comp)
        computations.append(self.img_shape[0] * self.img_shape[1] * self.numClass * self.planes * 2)
        return computations


# ------------------------------------------------------------------------------------------
# CrossEntropyLoss2d (model.py:76-82) + fused arg-max / accuracy (train.py:70-71)
# ------------------------------------------------------------------------------------------
class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, weight, module):
        if logits.device.type != "cuda":
            raise L.RcvError("CrossEntropyLoss2d runs on the HIP device only (got %s)" % logits.device)
        h = L.handle(logits.device.index if logits.device.index is not None else torch.cuda.current_device())
        logits_c = logits.detach().to(torch.float32).contiguous()
        targets_c = targets.detach().to(torch.int64).contiguous()
        N, Cc, H, W = logits_c.shape
        if targets_c.shape != (N, H, W):
            raise ValueError("targets must be [B,H,W] matching logits %s, got %s" % (tuple(logits_c.shape), tuple(targets_c.shape)))
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        argmax = torch.empty(N, H, W, dtype=torch.uint8, device=logits.device)
        op = L.make_op(L.OP_CE_FWD, L.F_ARGMAX, n=N, h=H, w=W, cout=Cc, p_in=logits_c.data_ptr(), p_in2=targets_c.data_ptr(),
                       p_w=(weight.data_ptr() if weight is not None else 0), p_out=out.data_ptr(), p_x0=argmax.data_ptr())
        nbytes = L.op_workspace(h, op)
        part = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=logits.device)
        op.p[L.RCV_P_PART] = part.data_ptr()
        L.OpList([op]).run(h, torch.cuda.current_stream(logits.device).cuda_stream)
        ctx.save_for_backward(logits_c, targets_c, out)
        ctx.weight = weight
        ctx.handle = h
        module.last_argmax = argmax
        module.last_stats = out          # [loss, sum_w, #correct, sum_w*nll]
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        logits, targets, out = ctx.saved_tensors
        N, Cc, H, W = logits.shape
        go = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        dl = torch.empty_like(logits)
        w = ctx.weight
        op = L.make_op(L.OP_CE_BWD, 0, n=N, h=H, w=W, cout=Cc, p_in=logits.data_ptr(), p_in2=targets.data_ptr(),
                       p_w=(w.data_ptr() if w is not None else 0), p_x0=out.data_ptr(), p_x1=go.data_ptr(), p_out=dl.data_ptr())
        L.OpList([op]).run(ctx.handle, torch.cuda.current_stream(logits.device).cuda_stream)
        return dl, None, None, None


class CrossEntropyLoss2d(nn.Module):
    """NLLLoss(weight, mean)(log_softmax(inputs, 1), targets) (model.py:76-82).  After a call,
    ``last_argmax`` (uint8 [B,H,W], first maximum on ties) and ``last_stats[2]`` (#pixels whose
    arg-max equals the target) hold what train.py:70-71 computes with torch.max."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).clone())
        self.last_argmax: Optional[torch.Tensor] = None
        self.last_stats: Optional[torch.Tensor] = None

    def forward(self, inputs, targets):
        w = self.weight
        if w is not None and w.device != inputs.device:
            w = w.to(inputs.device)
            self.weight = w
        return _CEFunction.apply(inputs, targets, w, self)


# ------------------------------------------------------------------------------------------
# DiceLoss (model.py:5-43; train.py:315 --useDice) + the same fused arg-max / accuracy
# ------------------------------------------------------------------------------------------
class _DiceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, weight, eps, module):
        if logits.device.type != "cuda":
            raise L.RcvError("DiceLoss runs on the HIP device only (got %s)" % logits.device)
        h = L.handle(logits.device.index if logits.device.index is not None else torch.cuda.current_device())
        logits_c = logits.detach().to(torch.float32).contiguous()
        N, Cc, H, W = logits_c.shape
        targets_c = targets.detach().to(torch.int64).reshape(N, H, W).contiguous()     # [B,H,W] or [B,1,H,W] (model.py:36)
        out = torch.empty(4 + 16, dtype=torch.float32, device=logits.device)
        argmax = torch.empty(N, H, W, dtype=torch.uint8, device=logits.device)
        op = L.make_op(L.OP_DICE_FWD, L.F_ARGMAX, n=N, h=H, w=W, cout=Cc, f1=eps, p_in=logits_c.data_ptr(), p_in2=targets_c.data_ptr(),
                       p_w=weight.data_ptr(), p_out=out.data_ptr(), p_x0=argmax.data_ptr())
        nbytes = L.op_workspace(h, op)
        part = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=logits.device)
        op.p[L.RCV_P_PART] = part.data_ptr()
        L.OpList([op]).run(h, torch.cuda.current_stream(logits.device).cuda_stream)
        ctx.save_for_backward(logits_c, targets_c, out)
        ctx.handle = h
        module.last_argmax = argmax
        module.last_stats = out          # [loss, -, #correct, -, backward coefficients...]
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        logits, targets, out = ctx.saved_tensors
        N, Cc, H, W = logits.shape
        go = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        dl = torch.empty_like(logits)
        op = L.make_op(L.OP_DICE_BWD, 0, n=N, h=H, w=W, cout=Cc, p_in=logits.data_ptr(), p_in2=targets.data_ptr(),
                       p_x0=out.data_ptr(), p_x1=go.data_ptr(), p_out=dl.data_ptr())
        L.OpList([op]).run(ctx.handle, torch.cuda.current_stream(logits.device).cuda_stream)
        return dl, None, None, None, None


class DiceLoss(nn.Module):
    """1 - mean_c(2 w_c I_c / (S_c + N_c + eps)) over softmax probabilities (model.py:5-43); the class weights are rescaled to
    mean 1 exactly as model.py:8.  ``last_argmax`` / ``last_stats[2]`` as CrossEntropyLoss2d.  The single-class branch (model.py:25-33: one
    logit channel z, probabilities (sigmoid z, 1 - sigmoid z) against the classes (t == 1, t == 0)) runs on the same kernels: those
    probabilities are the softmax of (z, 0), so the logits are widened by a zero channel and the target is flipped."""

    def __init__(self, weights, eps=1e-7):
        super().__init__()
        weights = torch.as_tensor(weights, dtype=torch.float32)
        self.register_buffer("weights", (weights / weights.sum().item() * weights.shape[0]).clone())
        self.eps = eps
        self.last_argmax: Optional[torch.Tensor] = None
        self.last_stats: Optional[torch.Tensor] = None

    def forward(self, logits, true):
        if logits.shape[1] == 1:
            if self.weights.numel() not in (1, 2):
                raise ValueError("single-class DiceLoss takes 1 or 2 class weights (got %d)" % self.weights.numel())
            if true.dim() == 4:
                true = true[:, 0]
            logits = torch.cat([logits, torch.zeros_like(logits)], dim=1)        # softmax((z, 0)) = (sigmoid z, 1 - sigmoid z)
            true = 1 - true.long()                                               # class 0 <-> target == 1 (model.py:28-30)
            if self.weights.numel() == 1:
                self.weights = self.weights.expand(2).clone()
        if logits.shape[1] != self.weights.shape[0]:
            raise ValueError("DiceLoss has %d class weights but the logits have %d channels" % (self.weights.shape[0], logits.shape[1]))
        w = self.weights
        if w.device != logits.device:
            w = w.to(logits.device)
            self.weights = w
        return _DiceFunction.apply(logits, true, w, float(self.eps), self)


# ------------------------------------------------------------------------------------------
# LabelProp (model.py:538-567) and the batch assembly of its training script (labelPropTrain.py:162-193)
# ------------------------------------------------------------------------------------------
class LabelProp(_EngineOwner, nn.Module):
    def __init__(self, numClass, numPlanes, dropout=0.0):
        super().__init__()
        self.pre = ConvPoolSimple(8, numPlanes // 4, 3, 1, 1, 1, False, dropout)
        self.down1 = ConvPoolSimple(numPlanes // 4, numPlanes // 2, 3, 2, 1, 1, False, dropout)
        self.down2 = ConvPoolSimple(numPlanes // 2, numPlanes // 2, 3, 2, 1, 1, False, dropout)
        self.down3 = ConvPoolSimple(numPlanes // 2, numPlanes, 3, 2, 1, 1, False, dropout)
        self.conv1 = ConvPoolSimple(numPlanes, numPlanes * 2, 3, 1, 2, 2, False, dropout)
        self.conv2 = ConvPoolSimple(numPlanes * 2, numPlanes * 2, 3, 1, 2, 2, False, dropout)
        self.conv3 = ConvPoolSimple(numPlanes * 2, numPlanes, 3, 1, 2, 2, False, dropout)
        self.upConv1 = upSampleTransposeConv(numPlanes, numPlanes // 2)
        self.upConv2 = upSampleTransposeConv(numPlanes // 2, numPlanes // 2)
        self.upConv3 = upSampleTransposeConv(numPlanes // 2, numPlanes // 2)
        self.classifier = nn.Conv2d(numPlanes // 2, numClass, 1, padding=0)

    # graph of model.py:556-567
    def _graph(self):
        nodes = []

        def add(node):
            nodes.append(node)
            return ("node", len(nodes) - 1)

        top = add(self.pre._node(("in", 0)))
        middle = add(self.down1._node(top))
        bottom = add(self.down2._node(middle))
        x = add(self.down3._node(bottom))
        x = add(self.conv1._node(x))
        x = add(self.conv2._node(x))
        x = add(self.conv3._node(x))
        x = add(self.upConv1._node(x, bottom))          # bottom + upConv1(x)
        x = add(self.upConv2._node(x, middle))          # middle + upConv2(x)
        x = add(self.upConv3._node(x, None))
        x = add({"op": "add_slice", "src": x, "add": top})      # x[:, 0:8] += top
        add({"op": "cls", "src": x, "weight": self.classifier.weight, "bias": self.classifier.bias})
        return {"inputs": [{"layout": "nhwc", "requires_grad": False}], "nodes": nodes}

    def _get_engine(self) -> Engine:
        eng = self.__dict__.get("_engine")
        mode = _graph_mode(self)
        if eng is None or self.__dict__.get("_engine_mode") != mode:
            eng = Engine(self._graph(), list(self.parameters()), _bn_modules(self))
            self.__dict__["_engine"] = eng
            self.__dict__["_engine_mode"] = mode
        return eng

    def _engine_inputs(self, x):
        """The engine reads the 8-channel input NHWC.  For a tensor whose memory already is NHWC (``labelprop_batch``, or
        ``x.contiguous(memory_format=torch.channels_last)``) the permutation is a view and nothing is copied.  A TRAINING forward takes
        only such a tensor: the first conv's filter gradient reads the input again in backward, so a re-laid-out copy would be a hidden
        full-resolution pass per step plus a tensor the engine would have to keep alive behind the caller's back -- the step's input
        is ``labelprop_batch``'s output, which has the layout already.  Inference re-lays a plain NCHW tensor out itself, as it always did."""
        if x.dim() != 4 or x.shape[1] != 8 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError("LabelProp expects float32 [B,8,H,W] with H,W multiples of 8, got %s" % (tuple(x.shape),))
        if x.requires_grad and self.training:
            raise L.RcvError("LabelProp does not produce a gradient for its input (labelPropTrain.py assembles it from frames and "
                             "labels); pass a tensor with requires_grad=False")
        nhwc = x.detach().to(torch.float32).permute(0, 2, 3, 1)
        if self.training and not nhwc.is_contiguous():
            raise L.RcvError("LabelProp in training mode reads its input as NHWC memory and makes no hidden copy of it: pass what "
                             "labelprop_batch(images, labels) returns, or x.contiguous(memory_format=torch.channels_last) "
                             "(got strides %s for shape %s); eval mode takes any layout" % (tuple(x.stride()), tuple(x.shape)))
        return [nhwc.contiguous()]

    def forward(self, x):
        """x float32 [B,8,H,W] -> logits [B,numClass,H,W] (model.py:556-567).  In training mode the tail is the out-of-place form of
        ``x[:,0:8] = x[:,0:8] + top``: upConv3's ReLU mask is taken from its own output, before the skip is added; the input must then be
        NHWC in memory (``labelprop_batch``'s output, or ``memory_format=torch.channels_last``), see ``_engine_inputs``."""
        return _run_engine(self._get_engine(), self.training, self._engine_inputs(x))


def _lp_input(cur, prev, prev_c, prior, pair, B, C, H, W, keep_plane, what):
    """One RCV_OP_LP_INPUT launch on the current stream (operands checked and contiguous): the NHWC inputs, logically [B,8,H,W], and
    the kept Y plane or None."""
    dev = cur.device
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    inputs = torch.empty(B, H, W, 8, dtype=torch.float32, device=dev)
    plane = torch.empty(B, H, W, dtype=torch.float32, device=dev) if keep_plane else None
    mode = {torch.uint8: L.LP_PRIOR_U8, torch.int64: L.LP_PRIOR_I64, torch.float32: L.LP_PRIOR_LOGITS}[prior.dtype]
    L.check(L.load().rcv_lp_input(h, cur.data_ptr(), prev.data_ptr() if prev is not None else None, prev_c, prior.data_ptr(), mode,
                                  1 if pair else 0, B, C, H, W, 5, inputs.data_ptr(), plane.data_ptr() if keep_plane else None,
                                  torch.cuda.current_stream(dev).cuda_stream), what)
    return inputs.permute(0, 3, 1, 2), plane


def _frame_planes(t, name, what):
    """(B, C, H, W) of a float32 frame tensor [B,C,H,W] or plane tensor [B,H,W] (C = 1)."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor" % (what, name))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32 (got %s)" % (what, name, t.dtype))
    if t.dim() not in (3, 4) or min(t.shape) < 1:
        raise ValueError("%s: %s must be [B,C,H,W] or a [B,H,W] plane (got %s)" % (what, name, tuple(t.shape)))
    return (t.shape[0], 1, t.shape[1], t.shape[2]) if t.dim() == 3 else tuple(t.shape)


def labelprop_next(cur, prev, prior, keep_plane=False):
    """LabelProp's input for the frames ``cur`` from a PREDICTION of the frames before them, one launch (RCV_OP_LP_INPUT): the loop body of
    makeLPImages.py:98-100 and the network branch of validLabelProp.py:116-130 on what a network said, not on ground truth.

    ``cur`` and ``prev`` float32 [B,C,H,W] (only channel 0, Y, is read) or [B,H,W] planes; ``prior`` is what was predicted for ``prev``:
    a class map uint8 or int64 [B,H,W] (``predict``'s output) -> labelToPred (transform.py:172-183), +1 at the class and -1 elsewhere,
    a value outside [0, 5) giving -1 in all five channels; or float32 logits [B,5,H,W] (``model(x)`` in eval mode) -> the prior the
    reference leaves commented at labelPropTrain.py:179, ``softmax * 2 - 1`` with m = max z, e = expf(z - m), S = (((e0 + e1) + e2) + e3)
    + e4, 2 * (e / S) - 1.  Returns ``inputs`` of logical shape [B,8,H,W] whose MEMORY is NHWC (``LabelProp`` reads it without a copy, in
    training mode too) = [Ycur, Yprev, Ycur - Yprev, prior]; with ``keep_plane=True`` ``(inputs, plane)``, ``plane`` a fresh float32
    [B,H,W] copy of Ycur written by the same launch (the next call's ``prev``)."""
    what = "labelprop_next"
    B, C, H, W = _frame_planes(cur, "cur", what)
    Bp, Cp, Hp, Wp = _frame_planes(prev, "prev", what)
    if not torch.is_tensor(prior):
        raise TypeError("%s: prior must be a tensor" % what)
    if prior.dtype not in (torch.uint8, torch.int64, torch.float32):
        raise TypeError("%s: prior must be a uint8 / int64 class map or float32 logits (got %s)" % (what, prior.dtype))
    if (Bp, Hp, Wp) != (B, H, W):
        raise ValueError("%s: prev %s does not match cur %s" % (what, tuple(prev.shape), tuple(cur.shape)))
    want = (B, 5, H, W) if prior.dtype == torch.float32 else (B, H, W)
    if tuple(prior.shape) != want:
        raise ValueError("%s: a %s prior must be %s for these frames (got %s)" % (what, prior.dtype, list(want), tuple(prior.shape)))
    if cur.device.type != "cuda" or prev.device != cur.device or prior.device != cur.device:
        raise L.RcvError("%s runs on the HIP device only (cur on %s, prev on %s, prior on %s)" % (what, cur.device, prev.device, prior.device))
    inputs, plane = _lp_input(cur.contiguous(), prev.contiguous(), Cp, prior.contiguous(), False, B, C, H, W, bool(keep_plane), "rcv_lp_input")
    return (inputs, plane) if keep_plane else inputs


def labelprop_batch(images, labels, num_class=5, prior_logits=None):
    """The batch assembly of labelPropTrain.py:162-193 in one launch (RCV_OP_LP_BATCH).

    ``images`` float32 [B,2,C,H,W] (frame pairs; only channel 0 of each frame is read, as the script does) and ``labels`` int64
    [B,2,H,W] -> ``(inputs, targets)``: ``inputs`` of logical shape [2B,8,H,W] whose MEMORY is NHWC (``LabelProp`` reads it without a
    copy), ``targets`` int64 [2B,H,W].  ``inputs[2b] = [Ya, Yb, Ya - Yb, labelToPred(label_b)]``, ``targets[2b] = label_a``, and the
    swapped sample at ``2b + 1``; labelToPred (transform.py:172-183) is -1 everywhere and +1 at the label's class.  A label outside
    [0, 5) cannot be refused without a host synchronisation (torch's ``scatter_`` would raise): such a pixel gets -1 in all five class
    channels and the label is never used as an index.  Exact: copies, +-1 and one fp32 subtraction.

    ``prior_logits`` float32 [B,2,5,H,W] (e.g. ``modelSeg(images.view(2B,3,H,W)).view(B,2,5,H,W)``): the class channels are the soft
    prior the script leaves commented at labelPropTrain.py:179, ``softmax(prior_logits) * 2 - 1`` of the OTHER frame of the pair, in
    place of ``labelToPred(labels)`` (the pair form of RCV_OP_LP_INPUT, arithmetic as ``labelprop_next``); ``targets`` is then
    ``labels.view(2B,H,W)``, a view without a copy.  Without the keyword nothing changes."""
    if prior_logits is not None:
        return _labelprop_batch_soft(images, labels, num_class, prior_logits)
    if num_class != 5:
        raise ValueError("labelprop_batch: num_class must be 5 (LabelProp's first conv reads 3 + 5 channels), got %r" % (num_class,))
    if not (torch.is_tensor(images) and torch.is_tensor(labels)):
        raise TypeError("labelprop_batch: images and labels must be tensors")
    if images.dtype != torch.float32 or labels.dtype != torch.int64:
        raise TypeError("labelprop_batch: images must be float32 and labels int64 (got %s, %s)" % (images.dtype, labels.dtype))
    if images.dim() != 5 or images.shape[1] != 2 or images.shape[2] < 1 or labels.dim() != 4:
        raise ValueError("labelprop_batch: images must be [B,2,C,H,W] and labels [B,2,H,W] (got %s, %s)"
                         % (tuple(images.shape), tuple(labels.shape)))
    B, _, Cc, H, W = images.shape
    if tuple(labels.shape) != (B, 2, H, W) or B < 1 or H < 1 or W < 1:
        raise ValueError("labelprop_batch: labels %s do not match images %s" % (tuple(labels.shape), tuple(images.shape)))
    if images.device.type != "cuda" or labels.device != images.device:
        raise L.RcvError("labelprop_batch runs on the HIP device only (images on %s, labels on %s)" % (images.device, labels.device))
    images, labels = images.contiguous(), labels.contiguous()
    dev = images.device
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    inputs = torch.empty(2 * B, H, W, 8, dtype=torch.float32, device=dev)
    targets = torch.empty(2 * B, H, W, dtype=torch.int64, device=dev)
    L.check(L.load().rcv_labelprop_batch(h, images.data_ptr(), labels.data_ptr(), B, Cc, H, W, num_class, inputs.data_ptr(),
                                         targets.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rcv_labelprop_batch")
    return inputs.permute(0, 3, 1, 2), targets


def _labelprop_batch_soft(images, labels, num_class, prior_logits):
    """``labelprop_batch(images, labels, prior_logits=...)``: the same argument checks, then the pair form of RCV_OP_LP_INPUT."""
    if num_class != 5:
        raise ValueError("labelprop_batch: num_class must be 5 (LabelProp's first conv reads 3 + 5 channels), got %r" % (num_class,))
    if not (torch.is_tensor(images) and torch.is_tensor(labels) and torch.is_tensor(prior_logits)):
        raise TypeError("labelprop_batch: images, labels and prior_logits must be tensors")
    if images.dtype != torch.float32 or labels.dtype != torch.int64 or prior_logits.dtype != torch.float32:
        raise TypeError("labelprop_batch: images and prior_logits must be float32 and labels int64 (got %s, %s, %s)"
                        % (images.dtype, prior_logits.dtype, labels.dtype))
    if images.dim() != 5 or images.shape[1] != 2 or images.shape[2] < 1 or labels.dim() != 4:
        raise ValueError("labelprop_batch: images must be [B,2,C,H,W] and labels [B,2,H,W] (got %s, %s)"
                         % (tuple(images.shape), tuple(labels.shape)))
    B, _, Cc, H, W = images.shape
    if tuple(labels.shape) != (B, 2, H, W) or B < 1 or H < 1 or W < 1:
        raise ValueError("labelprop_batch: labels %s do not match images %s" % (tuple(labels.shape), tuple(images.shape)))
    if tuple(prior_logits.shape) != (B, 2, 5, H, W):
        raise ValueError("labelprop_batch: prior_logits must be %s for these images (got %s)" % ([B, 2, 5, H, W], tuple(prior_logits.shape)))
    if images.device.type != "cuda" or labels.device != images.device or prior_logits.device != images.device:
        raise L.RcvError("labelprop_batch runs on the HIP device only (images on %s, labels on %s, prior_logits on %s)"
                         % (images.device, labels.device, prior_logits.device))
    inputs, _ = _lp_input(images.contiguous(), None, 0, prior_logits.contiguous(), True, 2 * B, Cc, H, W, False, "rcv_lp_input")
    return inputs, labels.contiguous().view(2 * B, H, W)


# ------------------------------------------------------------------------------------------
# host-side helpers of the module surface (model.py:45-74) -- scalar bookkeeping, not hot path
# ------------------------------------------------------------------------------------------
class PruneError(L.RcvError, ZeroDivisionError):
    """A tensor the prune rules cannot handle.  The reference dies with a ZeroDivisionError on a tensor without a non-zero weight
    (model.py:52, 629): callers that catch that keep working."""


def _prune_on_device(big, rule, ratio=0.0, lower=0.0, upper=0.0, amounts=None):
    """RCV_OP_PRUNE over the weight tensors ``big`` (device, fp32, contiguous): one launch, one workgroup per tensor, and ONE
    device-to-host copy of the job table at the end -- the only synchronisation of the call.  Returns (masks, rows): the masks are
    views of one uint8 buffer.  When the tensors are views of one flat buffer (the engine's layout) that buffer mirrors it element
    for element, so the optimizers take it as their flat prune mask as it is (optim._adopt_flat_mask)."""
    import ctypes as C
    dev = big[0].device
    datas = []
    for k, p in enumerate(big):
        d = p.data
        if d.device != dev or d.dtype != torch.float32 or not d.is_contiguous():
            raise L.RcvError("prune: parameter %d must be a contiguous fp32 tensor on %s (got %s, %s)" % (k, dev, d.dtype, d.device))
        datas.append(d)
    base = datas[0].untyped_storage().data_ptr()
    flat = all(d.untyped_storage().data_ptr() == base for d in datas)
    if flat:
        total = datas[0].untyped_storage().nbytes() // 4
        offs = [(d.data_ptr() - base) // 4 for d in datas]
    else:
        offs, total = [], 0
        for d in datas:
            offs.append(total)
            total += d.numel()
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    table = (L.RcvPruneJob * len(big))()
    for k, d in enumerate(datas):
        j = table[k]
        j.w, j.mask, j.n = d.data_ptr(), buf.data_ptr() + offs[k], d.numel()
        j.amount = 0 if amounts is None else amounts[k]
        j.lower, j.upper, j.ratio = float(lower), float(upper), float(ratio)
    lib = L.load()
    if lib.rcv_prune_check(table, len(big), rule) != 0:
        raise L.RcvError("librcv rcv_prune refused (parameter index = job index): %s" % lib.rcv_last_error().decode("utf-8", "replace"))
    h = L.handle(dev.index if dev.index is not None else torch.cuda.current_device())
    jobs = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    with torch.cuda.device(dev):
        L.check(lib.rcv_prune(h, jobs.data_ptr(), len(big), rule, torch.cuda.current_stream(dev).cuda_stream), "rcv_prune")
    rows = (L.RcvPruneJob * len(big)).from_buffer_copy(jobs.cpu().numpy().tobytes())
    _prune_check_rows(rows, rule)
    masks = [buf[o:o + d.numel()].view(d.shape).view(torch.bool) for o, d in zip(offs, datas)]
    return masks, rows


def _prune_check_rows(rows, rule):
    """The per-tensor refusals only the data can decide (rcv_prune_job.result[3])."""
    for k, r in enumerate(rows):
        st = int(r.result[3])
        if st == L.PRUNE_ST_NO_END:
            raise L.RcvError("pruneModel: parameter %d: the threshold search did not settle in %d steps (the window [lower, upper] is "
                             "narrower than one 2.5 %% step of the threshold moves the pruned share); the tensor is untouched"
                             % (k, L.PRUNE_MAX_ITER))
        if st == L.PRUNE_ST_ALL_ZERO or (rule != L.PRUNE_SMALLEST_K and st == L.PRUNE_ST_OK and int(r.result[1]) == 0):
            raise PruneError("prune: parameter %d has no non-zero weight (float division by zero in the reference)" % k)
        if st != L.PRUNE_ST_OK:
            raise L.RcvError("prune: parameter %d: the job was refused on the device (status %d)" % (k, st))


def pruneModelNew(params, ratio=0.01):
    """Magnitude pruning masks (model.py:45-57): zero weights below ratio*max|w|, return the masks.  Parameters on the HIP device
    are handled by one RCV_OP_PRUNE launch (rule 0) and one copy back, instead of three host syncs per tensor."""
    big = [p for p in params if p.dim() > 1]
    if big and big[0].device.type == "cuda":
        masks, rows = _prune_on_device(big, L.PRUNE_MAX_RATIO, ratio=ratio)
        for r in rows:
            print("Pruned %f%% of the weights" % (float(r.result[0]) / float(r.result[1]) * 100))
        return masks
    indices = []
    for param in big:
        with torch.no_grad():
            thresh = torch.max(torch.abs(param)) * ratio
            mask = torch.abs(param) < thresh
            print("Pruned %f%% of the weights" % (float(torch.sum(mask)) / float(torch.sum(param != 0)) * 100))
            param[mask] = 0
            indices.append(torch.abs(param) < thresh)
    return indices


def pruneModel(params, lower=73, upper=77):
    """model.py:621-642: per weight tensor, a threshold that starts at the tensor's standard deviation and is stepped by 2.5 % until
    between ``lower`` and ``upper`` per cent of the non-zero weights lie below it; those are zeroed.  Returns the masks.

    Fixed here where the reference leaves it open: the standard deviation is the fp32 rounding of the float64 two-pass value; the
    search is cut off after 4096 steps (the reference's loop need not end) with an RcvError that names the parameter; a tensor
    with fewer than two elements, or without a non-zero weight, is refused (PruneError, a ZeroDivisionError as in the reference)."""
    big = [p for p in params if p.dim() > 1]
    if big and big[0].device.type == "cuda":
        masks, rows = _prune_on_device(big, L.PRUNE_STD_SEARCH, lower=lower, upper=upper)
        for r in rows:
            print("Pruned %f%% of the weights" % (float(r.result[0]) / float(r.result[1]) * 100))
        return masks
    indices = []
    for k, param in enumerate(big):
        param = param.data
        if param.numel() < 2:
            raise L.RcvError("pruneModel: parameter %d has %d element: its standard deviation is NaN" % (k, param.numel()))
        d = param.double()
        thresh = torch.sqrt(((d - d.mean()) ** 2).sum() / (param.numel() - 1)).float()
        nonzero = float(torch.sum(param != 0))
        if nonzero == 0:
            raise PruneError("prune: parameter %d has no non-zero weight (float division by zero in the reference)" % k)
        for _ in range(L.PRUNE_MAX_ITER):
            num = float(torch.sum(torch.abs(param) < thresh)) / nonzero * 100
            if num < lower:
                thresh *= 1.025
            elif num > upper:
                thresh *= 0.975
            else:
                break
        else:
            raise L.RcvError("pruneModel: parameter %d: the threshold search did not settle in %d steps; the tensor is untouched"
                             % (k, L.PRUNE_MAX_ITER))
        print("Pruned %f%% of the weights" % (float(torch.sum(torch.abs(param) < thresh)) / nonzero * 100))
        param[torch.abs(param) < thresh] = 0
        indices.append(torch.abs(param) < thresh)
    return indices


def pruneModel2(params, ratio, lT, hT):
    """model.py:644-672 (pruner.py:158-209): zero the ``int(n * r)`` smallest-magnitude weights of every weight tensor, r = 0 below
    100 elements, 0.8 * ratio below ``lT``, 1.05 * ratio above ``hT``; the mask is ``param == 0`` afterwards, so weights pruned in
    earlier rounds are in it.  Among equal magnitudes at the boundary the LOWEST flat indices go (torch.topk leaves that open)."""
    big = [p for p in params if p.dim() > 1]
    rs, amounts = [], []
    for k, param in enumerate(big):
        r = ratio
        if getParamSize(param) < 100:
            r = 0
        elif getParamSize(param) < lT:
            r = ratio * 0.8
        if getParamSize(param) > hT:
            r = ratio * 1.05
        amount = int(param.numel() * r)
        if amount > param.numel() or amount < 0:
            raise L.RcvError("pruneModel2: parameter %d: amount %d out of range for %d elements (torch.topk: k not in range)"
                             % (k, amount, param.numel()))
        rs.append(r)
        amounts.append(amount)
    if big and big[0].device.type == "cuda":
        masks, _ = _prune_on_device(big, L.PRUNE_SMALLEST_K, amounts=amounts)
    else:
        masks = []
        for param, amount in zip(big, amounts):
            flat = param.data.reshape(-1)
            if not param.data.is_contiguous():
                raise L.RcvError("pruneModel2: parameters must be contiguous")
            if amount > 0:
                idx = torch.sort(torch.abs(flat), stable=True)[1][:amount]
                flat[idx] = 0.0
            masks.append(param.data == 0.0)
    for param, amount, r in zip(big, amounts, rs):
        print("Pruned %d of %d weights (%.3f%%)" % (amount, param.numel(), r))
    return masks


def count_zero_weights(model):
    """Fraction of weights below 1% of their tensor's maximum (model.py:59-66)."""
    small = 0.0
    total = 0
    for param in model.parameters():
        mx = torch.max(torch.abs(param))
        small += float((torch.abs(param) < mx * 0.01).sum())
        total += param.numel()
    return float(small / total)


def getParamSize(x):
    n = 1
    for s in x.size():
        n *= s
    return n


class DownSampler(nn.Module):
    """PB_FCN encoder (model.py:201-237): children and construction order as the reference (state_dict / init parity)."""

    def __init__(self, planes, noScale):
        super().__init__()
        self.noScale = noScale
        outPlanes = planes // 4
        self.conv0 = ConvPoolSimple(3, outPlanes, 3, 1, 2, 2, False)
        self.conv1 = ConvPoolSimple(outPlanes, planes // 2, 3, 2, 1, 1, False)
        self.conv2 = ConvPool(planes // 2, planes)
        self.conv_ext = ConvPool(planes, planes) if noScale else None
        self.conv3 = ConvPool(planes, planes * 2)
        self.conv4 = ConvPoolSimple(planes * 2, planes * 4, 3, 1, 2, 2, False)
        self.conv5 = ConvPoolSimple(planes * 4, planes * 4, 3, 1, 2, 2, False)
        self.conv6 = ConvPoolSimple(planes * 4, planes * 4, 3, 1, 2, 2, False)
        self.conv7 = ConvPoolSimple(planes * 4, planes * 4, 3, 1, 2, 2, False)
        self.conv8 = ConvPoolSimple(planes * 4, planes * 2, 3, 1, 2, 2, False)

    def _nodes(self, nodes: list, src):
        """model.py:221-229; returns the references of (x4, x3, x2, x1, x0) (x4 is None without noScale)."""
        def add(node):
            nodes.append(node)
            return ("node", len(nodes) - 1)

        def belly(x):
            x = self.conv3._nodes(nodes, x)
            for m in (self.conv4, self.conv5, self.conv6, self.conv7, self.conv8):
                x = add(m._node(x))
            return x

        x0 = add(self.conv0._node(src))
        x1 = add(self.conv1._node(x0))
        x2 = self.conv2._nodes(nodes, x1)
        if self.noScale:
            x3 = self.conv_ext._nodes(nodes, x2)
            return belly(x3), x3, x2, x1, x0
        return None, belly(x2), x2, x1, x0

    def forward(self, x):
        raise L.RcvError("DownSampler is executed as part of PB_FCN's graph; standalone use is not built")


class Classifier(nn.Module):
    """1x1 (kernelSize) classifier conv, optionally behind a max-pool (model.py:255-266).  The un-pooled one is PB_FCN's segmenter;
    the pooled one (poolSize > 1) is the patch-classification head, run as PB_FCN(classify=1)'s graph."""

    def __init__(self, inplanes, num_classes, poolSize=0, kernelSize=1):
        super().__init__()
        self.classifier = nn.Conv2d(inplanes, num_classes, kernel_size=kernelSize, padding=kernelSize // 2)
        self.pool = None
        if poolSize > 1:
            self.pool = nn.MaxPool2d(poolSize)

    def _node(self, src):
        if self.pool is not None:
            raise L.RcvError("the pooled classification head of PB_FCN (classify=1) is outside the segmentation path")
        return {"op": "cls", "src": src, "weight": self.classifier.weight, "bias": self.classifier.bias}

    def _head_node(self, src):
        """The pooled head as the graph's last node (model.py:262-265): MaxPool2d(poolSize) (floor), then the classifier."""
        if self.pool is None:
            raise L.RcvError("this Classifier has no pooled head")
        if tuple(self.classifier.kernel_size) == (5, 5):
            raise NotImplementedError(POOLED_5X5)
        k = self.pool.kernel_size
        return {"op": "pool_cls", "src": src, "pool": ("max", k if isinstance(k, int) else k[0]), "weight": self.classifier.weight,
                "bias": self.classifier.bias, "dropout": 0.0}

    def forward(self, x):
        raise L.RcvError("Classifier is executed as part of PB_FCN's graph; standalone use is not built")


class PB_FCN(_EngineOwner, nn.Module):
    """The older PB-FCN segmentation net of trainer.py (model.py:269-309): dilated conv->BN->ReLU encoder, three (four with
    noScale) transposed-conv decoder blocks with skip adds, 1x1 segmenter.  classify=1 (classTrainer.py:83, the pretraining
    stage) runs the encoder and the pooled head instead: MaxPool2d(4) of f3 (MaxPool2d(2) of f4 with noScale), 1x1 classifier;
    the decoder and the segmenter then keep grad None, as under the reference's autograd."""

    def __init__(self, planes, num_classes, kernelSize, noScale, classify):
        super().__init__()
        self.noScale = noScale
        self.classify = classify
        self.img_shape = (240, 320) if self.noScale else (120, 160)
        muliplier = 2 if noScale else 1
        outPlanes = planes // 4
        self.FCN = DownSampler(planes, noScale)
        self.up1 = upSampleTransposeConv(planes * 2, planes)
        self.up2 = upSampleTransposeConv(planes, planes // 2 * muliplier)
        self.up3 = upSampleTransposeConv(planes // 2 * muliplier, outPlanes * muliplier)
        self.up4 = upSampleTransposeConv(planes // 2, outPlanes) if noScale else None
        self.classifier = Classifier(planes * 2, num_classes, poolSize=(2 if noScale else 4), kernelSize=kernelSize)
        self.segmenter = Classifier(outPlanes, num_classes, kernelSize=kernelSize)

    # graph of model.py:291-309
    def _graph(self):
        nodes: list = []
        f4, f3, f2, f1, f0 = self.FCN._nodes(nodes, ("in", 0))
        if self.classify:           # model.py:294-298
            nodes.append(self.classifier._head_node(f4 if self.noScale else f3))
            return {"inputs": [{"layout": "nchw"}], "nodes": nodes}

        def up(layer, x, skip):
            nodes.append(layer._node(x, skip))
            return ("node", len(nodes) - 1)

        if self.noScale:
            x = up(self.up1, f4, f3)
            x = up(self.up2, x, f2)
            x = up(self.up3, x, f1)
            x = up(self.up4, x, f0)
        else:
            x = up(self.up1, f3, f2)
            x = up(self.up2, x, f1)
            x = up(self.up3, x, f0)
        nodes.append(self.segmenter._node(x))
        return {"inputs": [{"layout": "nchw"}], "nodes": nodes}

    def _get_engine(self) -> Engine:
        eng = self.__dict__.get("_engine")
        mode = _graph_mode(self)
        if eng is None or self.__dict__.get("_engine_mode") != mode:
            eng = Engine(self._graph(), list(self.parameters()), _bn_modules(self))
            self.__dict__["_engine"] = eng
            self.__dict__["_engine_mode"] = mode
        return eng

    def _engine_inputs(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("PB_FCN expects float32 [B,3,H,W], got %s" % (tuple(x.shape),))
        down = 16 if self.noScale else 8
        if x.shape[2] % down or x.shape[3] % down:
            raise ValueError("H and W must be multiples of %d (got %dx%d)" % (down, x.shape[2], x.shape[3]))
        return [x.to(torch.float32).contiguous()]

    def forward(self, x):
        return _run_engine(self._get_engine(), self.training, self._engine_inputs(x))


class View(nn.Module):
    """x.view(-1, numFeat) (model.py:84-90): a reshape, no kernel; works on any device like the reference's."""

    def __init__(self, numFeat):
        super().__init__()
        self.numFeat = numFeat

    def forward(self, x):
        return x.view(-1, self.numFeat)


class ConvPoolDouble(_BlockMixin, nn.Module):
    """relu(bn(pool(relu(conv2(relu(conv1(x))))))): two dilated 3x3 convs, then a stride-2 3x3 conv as the 'pool' (model.py:144-164)."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.relu = nn.ReLU()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, dilation=2, padding=2, bias=False)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, dilation=2, padding=2, bias=False)
        self.pool = nn.Conv2d(planes, planes, kernel_size=3, padding=1, stride=2, bias=False)
        self.bn = nn.BatchNorm2d(planes)

    def _nodes(self, nodes: list, src):
        for conv in (self.conv1, self.conv2):
            nodes.append({"op": "conv", "src": src, "weight": conv.weight, "bias": None, "bn": None, "stride": 1, "dil": 2,
                          "order": "relu"})
            src = ("node", len(nodes) - 1)
        nodes.append({"op": "conv", "src": src, "weight": self.pool.weight, "bias": None, "bn": self.bn,
                      "stride": 2, "dil": 1, "order": "bn_relu"})
        return ("node", len(nodes) - 1)

    def _block_graph(self):
        nodes: list = []
        out = self._nodes(nodes, ("in", 0))
        nodes.append({"op": "mat", "src": out})
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}], "nodes": nodes}

    def forward(self, x):
        return self._block_forward(x)


class DownSamplerThick(nn.Module):
    """FCN's encoder (model.py:235-254): children and construction order as the reference (state_dict / init parity)."""

    def __init__(self, planes):
        super().__init__()
        outPlanes = planes // 2
        self.conv0 = ConvPoolSimple(3, outPlanes, 3, 1, 2, 2, False)
        self.conv0_1 = ConvPoolSimple(outPlanes, outPlanes, 3, 1, 2, 2, False)
        self.conv1 = ConvPoolSimple(outPlanes, outPlanes, 3, 2, 1, 1, False)
        self.conv2 = ConvPoolDouble(outPlanes, planes)
        self.conv3 = ConvPoolDouble(planes, planes * 2)
        self.conv4 = ConvPoolSimple(planes * 2, planes * 4, 3, 1, 2, 2, False)
        self.conv5 = ConvPoolSimple(planes * 4, planes * 2, 3, 1, 2, 2, False)

    def _nodes(self, nodes: list, src):
        """model.py:248-254; returns the references of (x3, x2, x1, x0)."""
        def add(node):
            nodes.append(node)
            return ("node", len(nodes) - 1)

        x0 = add(self.conv0_1._node(add(self.conv0._node(src))))
        x1 = add(self.conv1._node(x0))
        x2 = self.conv2._nodes(nodes, x1)
        x3 = self.conv3._nodes(nodes, x2)
        x3 = add(self.conv5._node(add(self.conv4._node(x3))))
        return x3, x2, x1, x0

    def forward(self, x):
        raise L.RcvError("DownSamplerThick is executed as part of FCN's graph; standalone use is not built")


class FCN(_EngineOwner, nn.Module):
    """The oldest segmentation net (model.py:311-330), the one the trained checkpoints shipped with the reference
    (pth/bestModelSeg1*.pth) load into: DownSamplerThick(32), three transposed-conv decoder blocks with skip adds and a 1x1
    classifier on 16 channels, five classes.  Training, eval, ``predict`` and ``validate`` as PB_FCN."""

    def __init__(self):
        super().__init__()
        planes = 32
        self.FCN = DownSamplerThick(32)
        self.up1 = upSampleTransposeConv(planes * 2, planes)
        self.up2 = upSampleTransposeConv(planes, planes // 2)
        self.up3 = upSampleTransposeConv(planes // 2, planes // 2)
        self.classifier = Classifier(planes // 2, 5, 1)

    # graph of model.py:325-330
    def _graph(self):
        nodes: list = []
        f3, f2, f1, f0 = self.FCN._nodes(nodes, ("in", 0))
        x = f3
        for layer, skip in ((self.up1, f2), (self.up2, f1), (self.up3, f0)):
            nodes.append(layer._node(x, skip))
            x = ("node", len(nodes) - 1)
        nodes.append(self.classifier._node(x))
        return {"inputs": [{"layout": "nchw"}], "nodes": nodes}

    def _get_engine(self) -> Engine:
        eng = self.__dict__.get("_engine")
        if eng is None:
            eng = Engine(self._graph(), list(self.parameters()), _bn_modules(self))
            self.__dict__["_engine"] = eng
        return eng

    def _engine_inputs(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("FCN expects float32 [B,3,H,W], got %s" % (tuple(x.shape),))
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError("H and W must be multiples of 8 (got %dx%d)" % (x.shape[2], x.shape[3]))
        return [x.to(torch.float32).contiguous()]

    def forward(self, x):
        return _run_engine(self._get_engine(), self.training, self._engine_inputs(x))


class ConvSep(_BlockMixin, nn.Module):
    """relu(bn2(conv_1x1(relu(bn1(cat(conv_nx1(x), conv_1xn(x))))))) (model.py:333-361): the separable stand-in for Conv.  The 1-D
    pair runs as ONE 3x3 record whose filter is the cross of the two (first half of the channels: centre column, second half: centre
    row; same stride, dilation and padding); the 1x1 conv is the pointwise family (csrc/conv_pw.hip)."""

    def __init__(self, inplanes, planes, size, stride=1):
        super().__init__()
        if size != 3:
            raise NotImplementedError("only ConvSep(size=3) is built: the 1-D pair is lowered to the 3x3 records (got size=%r)" % (size,))
        if planes % 2:
            raise NotImplementedError("ConvSep is built for an even number of planes: each 1-D conv gives planes // 2 of the channels "
                                      "the 1x1 conv and its BatchNorm expect (got planes=%r)" % (planes,))
        self.stride = stride
        self.size = size
        self.inch = inplanes
        self.ch = planes
        dilation = 1 if stride > 1 else 2
        padding = size // 2 + dilation - 1
        self.conv_nx1 = nn.Conv2d(inplanes, planes // 2, dilation=dilation, kernel_size=(size, 1), padding=(padding, 0), stride=stride,
                                  bias=False)
        self.conv_1xn = nn.Conv2d(inplanes, planes // 2, dilation=dilation, kernel_size=(1, size), padding=(0, padding), stride=stride,
                                  bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv_1x1 = nn.Conv2d(planes, planes, kernel_size=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)

    def _nodes(self, nodes: list, src):
        nodes.append({"op": "conv", "src": src, "cross": (self.conv_nx1.weight, self.conv_1xn.weight, 0), "bias": None, "bn": self.bn1,
                      "stride": self.stride, "dil": 1 if self.stride > 1 else 2, "order": "bn_relu"})
        nodes.append({"op": "pw", "src": ("node", len(nodes) - 1), "weight": self.conv_1x1.weight, "bn": self.bn2, "order": "bn_relu"})
        return ("node", len(nodes) - 1)

    def _block_graph(self):
        nodes: list = []
        out = self._nodes(nodes, ("in", 0))
        nodes.append({"op": "mat", "src": out})
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}], "nodes": nodes}

    def forward(self, x):
        return self._block_forward(x)

    def getComp(self, W, H, pruned):
        W = W // self.stride
        H = H // self.stride
        ratio_nx1 = float(self.conv_nx1.weight.nonzero().size(0)) / float(self.conv_nx1.weight.numel()) if pruned else 1
        ratio_1xn = float(self.conv_1xn.weight.nonzero().size(0)) / float(self.conv_1xn.weight.numel()) if pruned else 1
        ratio_1x1 = float(self.conv_1x1.weight.nonzero().size(0)) / float(self.conv_1x1.weight.numel()) if pruned else 1
        return self.size * W * H * self.inch * self.ch * 2 * (ratio_1xn + ratio_nx1) + W * H * self.ch * self.ch * 2 * ratio_1x1 \
            + W * H * self.ch * 8, W, H


class trConvSep(_BlockMixin, nn.Module):
    """relu(bn2(trconv1x3(y) + trconv3x1(y))), y = relu(bn1(conv(x))) (model.py:363-377): the separable stand-in for
    upSampleTransposeConv.  The 1x1 conv is the pointwise family; the pair of 1-D transposed convs runs as ONE 3x3 stride-2 transposed
    record whose filter is the cross of the two, the centre tap their sum."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.trconv1x3 = nn.ConvTranspose2d(planes, planes, kernel_size=(1, 3), padding=(0, 1), stride=2, output_padding=1, bias=False)
        self.trconv3x1 = nn.ConvTranspose2d(planes, planes, kernel_size=(3, 1), padding=(1, 0), stride=2, output_padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.bn2 = nn.BatchNorm2d(planes)

    def _nodes(self, nodes: list, src):
        nodes.append({"op": "pw", "src": src, "weight": self.conv.weight, "bn": self.bn1, "order": "bn_relu"})
        nodes.append({"op": "up", "src": ("node", len(nodes) - 1), "skip": None, "concat": False,
                      "cross": (self.trconv1x3.weight, self.trconv3x1.weight, 1), "bias": None, "bn": self.bn2})
        return ("node", len(nodes) - 1)

    def _block_graph(self):
        nodes: list = []
        out = self._nodes(nodes, ("in", 0))
        nodes.append({"op": "mat", "src": out})
        return {"inputs": [{"layout": "nhwc", "requires_grad": True}], "nodes": nodes}

    def forward(self, x):
        return self._block_forward(x)


class PB_FCN_2(ROBO_UNet):
    """trainer.py's v2 net (model.py:416-458, built at trainer.py:126-127): the ROBO-UNet graph with a one-conv Level0 plus a
    pooled patch-classification head whose parameters stay outside the segmentation graph (grad None).  classify=True
    (classTrainer.py:83 --v2) runs downPart -> PB -> plane mean -> Dropout2d -> 1x1 classifier instead (model.py:444-453); the
    decoder and the segmenter then keep grad None."""

    def __init__(self, classify, nClass=5, planes=8, depth=4, levels=2, bellySize=5, bellyPlanes=128):
        nn.Module.__init__(self)
        self.classify = classify
        self.numClass = nClass
        self.planes = planes
        self.v2 = False
        self.img_shape = (120, 160)
        maxDepth = planes * pow(2, depth - 1)
        self.downPart = nn.ModuleList()
        self.downPart.add_module("Level0", LevelDown(3, planes, 1, False))
        for i in range(depth - 1):
            nCh = planes * pow(2, i)
            self.downPart.add_module("Level%d" % (i + 1), LevelDown(nCh, nCh * 2, levels, True))
        self.PB = nn.Sequential()
        self.PB.add_module("PB_1", LevelDown(maxDepth, bellyPlanes, bellySize - 1, False))
        self.PB.add_module("PB_2", LevelDown(bellyPlanes, maxDepth, 1, False))
        self.upPart = nn.ModuleList()
        for i in range(depth - 1):
            nCh = planes * pow(2, depth - 1 - i)
            self.upPart.add_module("Up%d" % i, upSampleTransposeConv(nCh, nCh // 2))
        self.classifier = UltClassifier(maxDepth, nClass, True)
        self.segmenter = UltClassifier(planes, nClass, False)

    def _graph(self):
        if not self.classify:
            return ROBO_UNet._graph(self)
        nodes: list = []
        x = ("in", 0)
        for level in self.downPart:
            x = level._nodes(nodes, x)
        for level in self.PB:
            x = level._nodes(nodes, x)
        nodes.append(self.classifier._head_node(x))
        return {"inputs": [{"layout": "nchw"}], "nodes": nodes}
