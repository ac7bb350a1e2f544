"""Robot-side export of a trained network: the flat float64 weight file of paramSave.py and the
darknet-style layer list of weights/net.cfg that the on-robot inference engine reads next to it -- written for every network the
engine's section vocabulary can spell (``net_cfg``, ``save_export``), and read back (``loadParams``, ``load_export``) into a module
that runs on the engine's existing graph nodes.  Host-side I/O, no kernels."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .engine import Engine
from .model import _EngineOwner, _run_engine

__all__ = ["flat_params", "saveParams", "loadParams", "net_cfg", "save_export", "load_export", "ExportedNet"]


def flat_params(model, skipClassifier: bool = False) -> np.ndarray:
    """Every state_dict entry (parameters AND buffers, num_batches_tracked included) flattened and concatenated in
    state_dict order as float64 (paramSave.py:9-18); entries whose name contains 'classifier' are dropped on request."""
    chunks = []
    for name, v in model.state_dict().items():
        if "classifier" in name and skipClassifier:
            continue
        chunks.append(v.detach().cpu().numpy().reshape(-1).astype(np.float64))
    return np.concatenate(chunks) if chunks else np.empty(0)


def saveParams(path, model, fName="weights.dat", skipClassifier=False):
    """paramSave.py:5-18: raw float64 dump to path/fName."""
    if not os.path.exists(path):
        os.makedirs(path)
    flat_params(model, skipClassifier).tofile(os.path.join(path, fName))


def _fill(tensors, flat: np.ndarray, what: str):
    """Copies ``flat`` into ``tensors`` in order.  ``tensors``: [(tensor, is num_batches_tracked)].  The file may carry the
    num_batches_tracked scalars or not; which, is decided by its element count."""
    full = sum(t.numel() for t, _ in tensors)
    bare = sum(t.numel() for t, nbt in tensors if not nbt)
    if flat.size not in (full, bare):
        raise ValueError("%s holds %d values; the network takes %d (%d with the num_batches_tracked scalars)" % (what, flat.size, bare, full))
    with_nbt = flat.size == full and full != bare
    off = 0
    with torch.no_grad():
        for t, nbt in tensors:
            if nbt and not with_nbt:
                continue
            n = t.numel()
            t.copy_(torch.from_numpy(flat[off:off + n].reshape(tuple(t.shape))).to(t.dtype))
            off += n
    return with_nbt


def loadParams(path, model, fName="weights.dat"):
    """The inverse of ``saveParams(path, model, fName)``: the float64 file's values into ``model``'s state_dict entries, in state_dict
    order.  A file without the num_batches_tracked scalars (the exports the reference ships) loads as well; those buffers then keep
    their values.  Raises ValueError with both counts when the file fits neither way."""
    flat = np.fromfile(os.path.join(path, fName), dtype=np.float64)
    _fill([(v, k.endswith("num_batches_tracked")) for k, v in model.state_dict().items()], flat, os.path.join(path, fName))
    if hasattr(model, "invalidate"):
        model.invalidate()
    return model


# ------------------------------------------------------------------------------------------
# writers: graph -> sections
# ------------------------------------------------------------------------------------------
_BN_RELU = ["[batchnorm]", "activation = relu"]
_BN_LINEAR = ["[batchnorm]", "activation = linear"]


def _conv_lines(w, stride, dil, activation, has_bias=None):
    k = w.shape[2]
    lines = ["[convolutional]", "filters=%d" % w.shape[0], "size=%d" % k, "stride=%d" % stride, "pad=%d" % (dil * (k // 2))]
    if has_bias is not None:
        lines.append("dilation=%d" % dil)
    lines.append("activation=%s" % activation)
    if has_bias is not None:
        lines.append("hasBias=%d" % has_bias)
    return lines


def _export_graph(model):
    if getattr(model, "v2", False):
        raise TypeError("net_cfg: a v2 network concatenates its skip tensors, and the reference ships no section spelling for a concatenation")
    if getattr(model, "classify", False):
        raise TypeError("net_cfg: a network in classify mode ends in the pooled patch head; the layer list describes the segmentation path")
    if not hasattr(model, "_graph"):
        raise TypeError("net_cfg describes the segmentation networks (PB_FCN, PB_FCN_2, ROBO_UNet, FCN, LabelProp), not %s" % type(model).__name__)
    return model._graph()


def _sections(graph):
    """The sections of a graph and, per section, the tensors it owns in file order: [(lines, [(tensor, is nbt)])]."""
    out = []
    close = {}            # node index -> layer index (0-based, [net] not counted) of the node's closing section
    ch = {}               # node index -> channels of its output

    def bn_tensors(bn):
        return [(bn.weight, False), (bn.bias, False), (bn.running_mean, False), (bn.running_var, False)] + \
            ([(bn.num_batches_tracked, True)] if bn.num_batches_tracked is not None else [])

    def wb(d):
        return [(d["weight"], False)] + ([(d["bias"], False)] if d.get("bias") is not None else [])

    def skip_from(ref, idx):
        if ref[0] != "node":
            raise TypeError("net_cfg: node %d adds the network input; [shortcut] refers to layers" % idx)
        return ["[shortcut]", "activation=linear", "from=%d" % close[ref[1]]]

    for idx, d in enumerate(graph["nodes"]):
        op = d["op"]
        last = idx == len(graph["nodes"]) - 1
        if d.get("cross") is not None:
            raise TypeError("net_cfg: node %d is a separable (1-D pair) block; the reference ships no section spelling for it" % idx)
        if op == "conv":
            order, bn, has_bias = d.get("order", "bn_relu"), d.get("bn"), int(d.get("bias") is not None)
            if order == "relu" and bn is None:
                out.append((_conv_lines(d["weight"], d["stride"], d["dil"], "relu", has_bias), wb(d)))
            elif order == "bn_relu" and bn is not None:
                out.append((_conv_lines(d["weight"], d["stride"], d["dil"], "linear", has_bias), wb(d)))
                out.append((_BN_RELU, bn_tensors(bn)))
            elif order == "relu_bn" and bn is not None:
                out.append((_conv_lines(d["weight"], d["stride"], d["dil"], "relu", has_bias), wb(d)))
                out.append((_BN_LINEAR, bn_tensors(bn)))
            else:
                raise TypeError("net_cfg: conv node %d (order %s, %s BatchNorm) has no section spelling" % (idx, order, "with" if bn is not None else "no"))
            ch[idx] = d["weight"].shape[0]
        elif op == "up":
            if d.get("concat"):
                raise TypeError("net_cfg: node %d concatenates its skip tensor (v2); the reference ships no section spelling for it" % idx)
            c = d["weight"]
            if d.get("bias") is None:
                raise TypeError("net_cfg: transposed conv node %d has no bias; [transposedconv] always carries one" % idx)
            out.append((["[transposedconv]", "filters=%d" % c.shape[1], "size=%d" % c.shape[2], "stride=2", "pad=1", "outpad=1", "activation=linear"], wb(d)))
            out.append((_BN_RELU, bn_tensors(d["bn"])))
            if d.get("skip") is not None:
                out.append((skip_from(d["skip"], idx), []))
            ch[idx] = c.shape[1]
        elif op == "add_slice":
            # x[:, 0:Ca] += add: a shortcut from a narrower layer adds into the leading channels (the shipped weightsLP/net.cfg)
            out.append((skip_from(d["add"], idx), []))
            ch[idx] = ch[d["src"][1]]
        elif op == "cls" and last:
            out.append((_conv_lines(d["weight"], 1, 1, "linear"), wb(d)))
            out.append((["[softmax]"], []))
        elif op == "pool":
            raise TypeError("net_cfg: node %d is a max-pool (pool=True); the reference ships no section spelling for it" % idx)
        else:
            raise TypeError("net_cfg: node %d ('%s') has no section spelling" % (idx, op))
        close[idx] = len(out) - 1
    return out


def _net_lines(model, graph, img_shape):
    H, W = img_shape if img_shape is not None else getattr(model, "img_shape", (120, 160))
    first = graph["nodes"][0]
    channels = 3 if graph["inputs"][0]["layout"] == "nchw" else first["weight"].shape[1]
    # downscale: carried verbatim from the shipped files; its consumer is not in the reference
    return ["[net]", "height=%d" % H, "width=%d" % W, "channels=%d" % channels, "downscale=4"]


def net_cfg(model, img_shape=None) -> str:
    """The layer list of weights/net.cfg for a segmentation network (PB_FCN, PB_FCN_2(classify=False), ROBO_UNet without v2 / pool,
    FCN, LabelProp): one [convolutional] / [transposedconv] section per conv, a [batchnorm] section where one follows (its activation
    says on which side of it the ReLU sits), [shortcut] sections for the skip adds (``from`` = index of the skipped block's closing
    layer; from a narrower layer: into the leading channels), [softmax] last.  ``img_shape`` = (H, W) overrides [net] height / width.
    Raises TypeError, saying why, for what the shipped section vocabulary cannot spell."""
    graph = _export_graph(model)
    sec = [_net_lines(model, graph, img_shape)] + [lines for lines, _ in _sections(graph)]
    return "\n\n".join("\n".join(lines) for lines in sec) + "\n"


def save_export(path, model, img_shape=None):
    """Writes path/net.cfg and path/weights.dat: the float64 file holds exactly the tensors the cfg lists, in cfg order (per
    [convolutional] / [transposedconv]: weight, bias; per [batchnorm]: weight, bias, running mean, running var, num_batches_tracked).
    For LabelProp, FCN and ROBO_UNet that is bit for bit ``saveParams``' file; for PB_FCN and PB_FCN_2 it is that file without the
    pooled patch head (``classifier.*``), which the layer list does not contain."""
    graph = _export_graph(model)
    secs = _sections(graph)
    text = "\n\n".join("\n".join(lines) for lines in [_net_lines(model, graph, img_shape)] + [lines for lines, _ in secs]) + "\n"
    if not os.path.exists(path):
        os.makedirs(path)
    with open(os.path.join(path, "net.cfg"), "w") as f:
        f.write(text)
    chunks = [t.detach().cpu().numpy().reshape(-1).astype(np.float64) for _, ts in secs for t, _ in ts]
    np.concatenate(chunks).tofile(os.path.join(path, "weights.dat"))


# ------------------------------------------------------------------------------------------
# reader: sections -> graph
# ------------------------------------------------------------------------------------------
_KEYS = {"net": {"height", "width", "channels", "downscale"},
         "convolutional": {"filters", "size", "stride", "pad", "dilation", "activation", "hasBias"},
         "batchnorm": {"activation"}, "transposedconv": {"filters", "size", "stride", "pad", "outpad", "activation"},
         "shortcut": {"activation", "from"}, "softmax": set()}


def _parse_cfg(text: str):
    """[(name, {key: value})]; the first section must be [net].  Layer indices are 0-based and do not count [net]."""
    secs = []
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        if line.startswith("[") and line.endswith("]"):
            name = line[1:-1].strip()
            if name not in _KEYS:
                raise ValueError("net.cfg: section %d is [%s]; the engine runs %s" % (len(secs) - 1, name, ", ".join("[%s]" % k for k in _KEYS)))
            secs.append((name, {}))
            continue
        if not secs or "=" not in line:
            raise ValueError("net.cfg: line '%s' belongs to no section" % line)
        k, v = (s.strip() for s in line.split("=", 1))
        if k not in _KEYS[secs[-1][0]]:
            raise ValueError("net.cfg: section %d [%s] has no key '%s'" % (len(secs) - 2, secs[-1][0], k))
        secs[-1][1][k] = v
    if not secs or secs[0][0] != "net":
        raise ValueError("net.cfg: the first section must be [net]")
    return secs


class ExportedNet(_EngineOwner, nn.Module):
    """A network read back from its robot-side export (``load_export``).  ``layers`` holds one module per section that owns tensors
    (nn.Conv2d, nn.ConvTranspose2d, nn.BatchNorm2d), in cfg order, so ``state_dict()`` lists the file's values in file order; ``net``
    holds the [net] keys.  Inference only: ``forward`` (logits), ``predict``, ``validate`` and ``proba`` run the graph the sections
    lower to -- for a network ``net_cfg`` can write, the graph of that network's own module, so the results are bit for bit its."""

    def __init__(self, cfg_text: str):
        super().__init__()
        secs = _parse_cfg(cfg_text)
        net = {k: int(v) for k, v in secs[0][1].items()}
        for k in ("height", "width", "channels"):
            if k not in net:
                raise ValueError("net.cfg: [net] lacks '%s'" % k)
        self.net = net
        cin = net["channels"]
        if cin != 3 and (cin < 4 or cin % 4):
            raise ValueError("net.cfg: [net] channels=%d: 3 (an NCHW image) or a multiple of 4 (an NHWC tensor)" % cin)
        self.layers = nn.ModuleList()
        self._file_tensors = []       # [(tensor, is nbt)] in file order
        self._bns = []
        layers = secs[1:]
        nodes: list = []
        close = {}                    # layer index -> (node index, channels) for the closing layer of every node
        src, ch, i = ("in", 0), cin, 0

        def bad(k, why):
            return ValueError("net.cfg: section %d [%s]: %s" % (k, layers[k][0] if k < len(layers) else "end of file", why))

        def geti(k, key, default=None):
            v = layers[k][1].get(key, default)
            if v is None:
                raise bad(k, "'%s' is missing" % key)
            return int(v)

        def name(k):
            return layers[k][0] if k < len(layers) else None

        def act(k):
            return layers[k][1].get("activation", "linear").strip()

        def add_bn(k, channels):
            bn = nn.BatchNorm2d(channels)
            self.layers.append(bn)
            self._bns.append(bn)
            self._file_tensors += [(bn.weight, False), (bn.bias, False), (bn.running_mean, False), (bn.running_var, False),
                                   (bn.num_batches_tracked, True)]
            return bn

        def skip_of(k, want):
            """The node a [shortcut] at layer k refers to; want = channels of the tensor it adds into."""
            f = geti(k, "from")
            if f not in close:
                raise bad(k, "from=%d is not the closing layer of an earlier block (closing layers: %s)" % (f, sorted(close)))
            node, c = close[f]
            if c > want:
                raise bad(k, "from=%d has %d channels, more than the %d it is added into" % (f, c, want))
            return node, c

        while i < len(layers):
            kind = name(i)
            if kind == "convolutional":
                filters, size, stride, pad = geti(i, "filters"), geti(i, "size"), geti(i, "stride"), geti(i, "pad")
                dil, has_bias, a = geti(i, "dilation", 1), geti(i, "hasBias", 1), act(i)
                nxt = name(i + 1)
                if a == "linear" and nxt in ("softmax", None):
                    if name(i + 1 + (nxt == "softmax")) is not None:
                        raise bad(i + 1 + (nxt == "softmax"), "nothing may follow the classifier%s" % (" and its [softmax]" if nxt == "softmax" else ""))
                    if size not in (1, 3, 5) or stride != 1 or dil != 1 or pad != size // 2 or not has_bias:
                        raise bad(i, "the classifier is a 1x1, 3x3 or 5x5 conv with stride 1, pad size/2, no dilation and a bias")
                    conv = nn.Conv2d(ch, filters, size, padding=pad)
                    self.layers.append(conv)
                    self._file_tensors += [(conv.weight, False), (conv.bias, False)]
                    nodes.append({"op": "cls", "src": src, "weight": conv.weight, "bias": conv.bias})
                    self.num_classes = filters
                    i = len(layers)
                    break
                if size != 3 or pad != dil or stride not in (1, 2):
                    raise bad(i, "feature convs are 3x3 with pad == dilation and stride 1 or 2 (size=%d pad=%d dilation=%d stride=%d)" % (size, pad, dil, stride))
                conv = nn.Conv2d(ch, filters, 3, stride=stride, padding=pad, dilation=dil, bias=bool(has_bias))
                self.layers.append(conv)
                self._file_tensors += [(conv.weight, False)] + ([(conv.bias, False)] if has_bias else [])
                node = {"op": "conv", "src": src, "weight": conv.weight, "bias": conv.bias, "bn": None, "stride": stride, "dil": dil}
                if nxt == "batchnorm":
                    b = act(i + 1)
                    if (a, b) == ("linear", "relu"):
                        node["order"] = "bn_relu"
                    elif (a, b) == ("relu", "linear"):
                        node["order"] = "relu_bn"
                    else:
                        raise bad(i + 1, "conv activation=%s followed by batchnorm activation = %s: exactly one of the two is relu" % (a, b))
                    node["bn"] = add_bn(i + 1, filters)
                    i += 2
                elif a == "relu":
                    node["order"] = "relu"
                    i += 1
                else:
                    raise bad(i, "a conv with activation=%s and no [batchnorm] behind it is neither a feature conv nor the last layer" % a)
                nodes.append(node)
                src, ch = ("node", len(nodes) - 1), filters
                close[i - 1] = (len(nodes) - 1, ch)
            elif kind == "transposedconv":
                filters = geti(i, "filters")
                if (geti(i, "size"), geti(i, "stride"), geti(i, "pad"), geti(i, "outpad"), act(i)) != (3, 2, 1, 1, "linear"):
                    raise bad(i, "transposed convs are size=3 stride=2 pad=1 outpad=1 activation=linear")
                if name(i + 1) != "batchnorm" or act(i + 1) != "relu":
                    raise bad(i + 1, "a [transposedconv] is followed by [batchnorm] activation = relu")
                conv = nn.ConvTranspose2d(ch, filters, 3, padding=1, stride=2, output_padding=1, bias=True)
                self.layers.append(conv)
                self._file_tensors += [(conv.weight, False), (conv.bias, False)]
                bn = add_bn(i + 1, filters)
                node = {"op": "up", "src": src, "skip": None, "concat": False, "weight": conv.weight, "bias": conv.bias, "bn": bn}
                i += 2
                narrow = None
                if name(i) == "shortcut":
                    sk, c = skip_of(i, filters)
                    if c == filters:
                        node["skip"] = ("node", sk)
                    else:
                        narrow = sk
                    i += 1
                nodes.append(node)
                src, ch = ("node", len(nodes) - 1), filters
                if narrow is not None:      # a shortcut from a narrower layer adds into the leading channels
                    nodes.append({"op": "add_slice", "src": src, "add": ("node", narrow)})
                    src = ("node", len(nodes) - 1)
                close[i - 1] = (len(nodes) - 1, ch)
            elif kind == "shortcut":
                sk, c = skip_of(i, ch)
                if c == ch or src[0] != "node":
                    raise bad(i, "a [shortcut] stands behind a [transposedconv] + [batchnorm]; on its own it adds a narrower layer into the leading channels")
                nodes.append({"op": "add_slice", "src": src, "add": ("node", sk)})
                src = ("node", len(nodes) - 1)
                i += 1
                close[i - 1] = (len(nodes) - 1, ch)
            else:
                raise bad(i, "a [%s] cannot stand here" % kind)
        if not nodes or nodes[-1]["op"] != "cls":
            raise ValueError("net.cfg: section %d: the layer list ends without a classifier (a last [convolutional] activation=linear)" % (len(layers) - 1))
        strides, worst = 1, 1          # the deepest downscale: H and W must be multiples of it
        for d in nodes:
            if d["op"] == "conv":
                strides *= d["stride"]
            elif d["op"] == "up":
                strides = max(strides // 2, 1)
            worst = max(worst, strides)
        self._down = worst
        if strides != 1:
            raise ValueError("net.cfg: the classifier runs at 1/%d of the input resolution; the decoder must return to full resolution" % strides)
        self._graph_dict = {"inputs": [{"layout": "nchw"} if cin == 3 else {"layout": "nhwc", "requires_grad": False}], "nodes": nodes}
        for p in self.parameters():
            p.requires_grad_(False)
        nn.Module.train(self, False)

    def _graph(self):
        return self._graph_dict

    def _get_engine(self) -> Engine:
        eng = self.__dict__.get("_engine")
        if eng is None:
            eng = Engine(self._graph(), list(self.parameters()), self._bns)
            self.__dict__["_engine"] = eng
        return eng

    def _engine_inputs(self, x):
        c = self.net["channels"]
        if x.dim() != 4 or x.shape[1] != c:
            raise ValueError("this export expects float32 [B,%d,H,W], got %s" % (c, tuple(x.shape)))
        if x.shape[2] % self._down or x.shape[3] % self._down:
            raise ValueError("H and W must be multiples of %d (got %dx%d)" % (self._down, x.shape[2], x.shape[3]))
        if c == 3:
            return [x.to(torch.float32).contiguous()]
        return [x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()]

    def train(self, mode: bool = True):
        if mode:
            raise L.RcvError("an exported network is an inference network: training runs on the module it was exported from")
        return super().train(False)

    def forward(self, x):
        """x float32 [B,channels,H,W] -> logits [B,classes,H,W] (what stands in front of the cfg's [softmax]; ``proba`` applies it)."""
        return _run_engine(self._get_engine(), False, self._engine_inputs(x))


def load_export(cfg_path, dat_path) -> ExportedNet:
    """Reads a robot-side export: parses the layer list, lowers it to the engine's graph nodes (conv in its three orders, up with its
    skip, add_slice, cls) and fills the tensors from the float64 file, section by section (files with and without the
    num_batches_tracked scalars both load).  Refuses any other section or pattern with the section's index, and a file of the wrong
    length with both counts."""
    with open(cfg_path) as f:
        net = ExportedNet(f.read())
    flat = np.fromfile(dat_path, dtype=np.float64)
    with_nbt = _fill(net._file_tensors, flat, str(dat_path))
    if not with_nbt:          # the file lists no num_batches_tracked: neither does the module's state_dict
        for bn in net._bns:
            bn.num_batches_tracked = None
    del net._file_tensors
    return net
