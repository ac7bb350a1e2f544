"""BNN-L and BNN-M-C, the patch classifiers the reference trains as its comparison baselines (model.py:569-619; objDetEval.py,
classVal.py --hessL / --hessMC), on the HIP path.

Same constructors, child names, ``state_dict`` keys and construction order as the reference.  The ``nn.Conv2d`` / ``nn.MaxPool2d`` /
``nn.Dropout*`` children are parameter and setting containers only; ``forward`` and ``backward`` run the records of csrc/bnn.hip: one
launch per stage (conv -> Dropout2d -> MaxPool2d -> ReLU) and direction, one for BNN-L's head (fc -> Dropout -> ReLU -> classifier),
and one fixed-order reduction per filter gradient.  The modules drive the library through a small plan of their own (a handful of
records per batch shape, cached); there is no CPU path.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L

__all__ = ["BNNL", "BNNMC"]


class _Plan:
    """Buffers and the two record lists of one (batch shape, dropout, backward) combination.  Built in three parts: the forward
    records with the stage buffers, the dropout keep-scale buffers, the backward records.  Pointers that change from call to call
    (parameters, input, logits, logits gradient, parameter gradients) are not written here: each part notes their (record, slot)
    pairs in a slot table and the caller patches them in."""

    def __init__(self, net: "_BNNBase", N: int, C: int, H: int, W: int, dropout: bool, backward: bool, handle, device):
        self.N, self.dropout, self.backward, self.handle, self.device = N, dropout, backward, handle, device
        self.generation = 0
        self.x = None
        self._bufs = []                # every device buffer the records point at lives as long as the plan
        self.param_slots = []          # (list, op index, pointer slot, parameter index)
        self.x_slots, self.out_slots, self.gout_slots = [], [], []      # (list, op index, pointer slot)
        self.grad_slots = []           # (backward op index, pointer slot, parameter index)
        self.keep_shapes = []          # (shape, p) of every keep-scale buffer, in forward order
        self._pidx = {id(p): k for k, p in enumerate(net.parameters())}
        self.grad_offsets, o = [], 0
        for p in net.parameters():
            self.grad_offsets.append(o)
            o += p.numel()
        self.grad_numel = o
        fwd, stage_info, head_info = self._forward_records(net, N, C, H, W)
        self._dropout_buffers(fwd, stage_info, head_info)
        bwd = self._backward_records(net, stage_info, head_info) if backward else []
        self.fwd, self.bwd = L.OpList(fwd), L.OpList(bwd)

    def _buf(self, shape, dtype=torch.float32):
        if self.device is None:        # planning only
            return None
        self._bufs.append(torch.empty(shape, dtype=dtype, device=self.device))
        return self._bufs[-1]

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def _forward_records(self, net, N, C, H, W):
        """The forward list.  Returns it with one dict per stage (and one for the head) holding what the other two parts need: the
        forward op index, the buffers, the keep-scale index and, when a backward is planned, the validated backward record."""
        pidx, fwd, stage_info, head_info = self._pidx, [], [], None
        stages = net._stages()
        cin, hh, ww, prev_out = C, H, W, None
        for si, (conv, pool, do, relu) in enumerate(stages):
            last = si == len(stages) - 1 and not net._has_head
            K, P, cout = int(conv.kernel_size[0]), int(conv.padding[0]), int(conv.out_channels)
            k = int(pool.kernel_size) if pool is not None else 0
            if pool is not None and int(pool.stride) != 2:
                raise L.RcvError("%s: the pooled stages run MaxPool2d(k, 2) only (stride %s given)" % (type(net).__name__, pool.stride))
            hc, wc = hh + 2 * P - K + 1, ww + 2 * P - K + 1
            ho, wo = ((hc - k) // 2 + 1, (wc - k) // 2 + 1) if k else (hc, wc)
            flags = (L.F_RELU if relu else 0) | (L.F_OUT_NCHW if last else 0)
            common = dict(n=N, h=hh, w=ww, cin=cin, cout=cout, ho=ho, wo=wo, aux0=K, aux1=k, count=P,
                          inmode=L.LOAD_NCHW if si == 0 else L.LOAD_PLAIN)
            f = L.make_op(L.OP_BNN_STAGE_FWD, flags, **common)
            L.op_workspace(self.handle, f)                 # refuses what the launch would refuse (plane too small, channel counts)
            info = dict(fi=len(fwd), conv=conv, first=si == 0, last=last, x=prev_out, keep=None, bwd=None,
                        out=None if last else self._buf((N, ho, wo, cout)),
                        arg=self._buf((N, ho, wo, cout), torch.uint8) if (self.backward and k) else None)
            if self.dropout and do is not None:
                self.keep_shapes.append(((N, cout), float(do.p)))
                info["keep"] = len(self.keep_shapes) - 1
            f.p[L.RCV_P_IN] = self._ptr(prev_out)
            f.p[L.RCV_P_OUT] = self._ptr(info["out"])
            f.p[L.RCV_P_X1] = self._ptr(info["arg"])
            fwd.append(f)
            self.param_slots += [("fwd", info["fi"], L.RCV_P_W, pidx[id(conv.weight)]), ("fwd", info["fi"], L.RCV_P_BIAS, pidx[id(conv.bias)])]
            if si == 0:
                self.x_slots.append(("fwd", info["fi"], L.RCV_P_IN))
            if last:
                self.out_slots.append(("fwd", info["fi"], L.RCV_P_OUT))
            if self.backward:
                b = L.make_op(L.OP_BNN_STAGE_BWD, flags, **common)
                nbytes = L.op_workspace(self.handle, b)
                info.update(bwd=b, ws=self._buf(max(nbytes // 4, 1)), dx=self._buf((N, hh, ww, cin)) if si > 0 else None)
            stage_info.append(info)
            prev_out, cin, hh, ww = info["out"], cout, ho, wo
        self.head_shape = (N, hh, ww)
        self.out_shape = (N, net._num_classes(), hh, ww)
        if net._has_head:
            nC, hid = int(net.classifier.out_channels), int(net.fc.out_channels)
            common = dict(n=N, h=hh, w=ww, cin=cin, cout=nC, count=hid)
            f = L.make_op(L.OP_BNN_HEAD_FWD, 0, **common)
            L.op_workspace(self.handle, f)
            head_info = dict(fi=len(fwd), x=prev_out, keep=None, bwd=None)
            if self.dropout:
                self.keep_shapes.append(((N, hh, ww, hid), float(net.dof.p)))
                head_info["keep"] = len(self.keep_shapes) - 1
            f.p[L.RCV_P_IN] = self._ptr(prev_out)
            fwd.append(f)
            fi = head_info["fi"]
            self.param_slots += [("fwd", fi, L.RCV_P_W, pidx[id(net.fc.weight)]), ("fwd", fi, L.RCV_P_BIAS, pidx[id(net.fc.bias)]),
                                 ("fwd", fi, L.RCV_P_X1, pidx[id(net.classifier.weight)]), ("fwd", fi, L.RCV_P_X2, pidx[id(net.classifier.bias)])]
            self.out_slots.append(("fwd", fi, L.RCV_P_OUT))
            if self.backward:
                b = L.make_op(L.OP_BNN_HEAD_BWD, 0, **common)
                nbytes = L.op_workspace(self.handle, b)
                head_info.update(bwd=b, ws=self._buf(max(nbytes // 4, 1)), dx=self._buf((N, hh, ww, cin)))
        return fwd, stage_info, head_info

    def _dropout_buffers(self, fwd, stage_info, head_info):
        """The keep-scales: one flat buffer viewed per layer, drawn by ONE bernoulli over per-element probabilities and one multiply
        by the per-element scale.  Points the forward AND the planned backward records of every dropping layer at its view."""
        self.keep_flat = self.keep_views = self.keep_prob = self.keep_scale = None
        if not self.keep_shapes or self.device is None:
            return
        sizes = [int(torch.Size(s).numel()) for s, _ in self.keep_shapes]
        self.keep_flat = torch.zeros(sum(sizes), dtype=torch.float32, device=self.device)
        self.keep_prob = torch.cat([torch.full((n,), 1.0 - p) for n, (_, p) in zip(sizes, self.keep_shapes)]).to(self.device)
        # 1 / (1 - p) in fp32, as torch's dropout scales its noise
        self.keep_scale = torch.cat([torch.full((n,), 1.0) / torch.full((n,), 1.0 - p) if p < 1.0 else torch.zeros(n)
                                     for n, (_, p) in zip(sizes, self.keep_shapes)]).to(self.device)
        self.keep_views, o = [], 0
        for n, (s, _) in zip(sizes, self.keep_shapes):
            self.keep_views.append(self.keep_flat[o:o + n].view(s))
            o += n
        for info in stage_info + ([head_info] if head_info is not None else []):
            if info["keep"] is not None:
                view = self.keep_views[info["keep"]]
                fwd[info["fi"]].p[L.RCV_P_X0] = view.data_ptr()
                if info["bwd"] is not None:
                    info["bwd"].p[L.RCV_P_X0] = view.data_ptr()

    def _backward_records(self, net, stage_info, head_info):
        """The backward list: the head, then the stages from the last to the first; each record's input gradient is the dx buffer of
        the record before it (the first one reads the caller's logits gradient)."""
        pidx, bwd = self._pidx, []
        dnext = None                   # gradient of the output of the layer in hand
        if head_info is not None:
            b, bi = head_info["bwd"], len(bwd)
            b.p[L.RCV_P_EPI_AUX] = self._ptr(head_info["x"])
            b.p[L.RCV_P_OUT] = self._ptr(head_info["dx"])
            b.p[L.RCV_P_PART] = self._ptr(head_info["ws"])
            bwd.append(b)
            self.gout_slots.append(("bwd", bi, L.RCV_P_IN))
            self.param_slots += [("bwd", bi, L.RCV_P_W, pidx[id(net.fc.weight)]), ("bwd", bi, L.RCV_P_BIAS, pidx[id(net.fc.bias)]),
                                 ("bwd", bi, L.RCV_P_X1, pidx[id(net.classifier.weight)])]
            self.grad_slots += [(bi, L.RCV_P_X2, pidx[id(net.fc.weight)]), (bi, L.RCV_P_X3, pidx[id(net.fc.bias)]),
                                (bi, L.RCV_P_X4, pidx[id(net.classifier.weight)]), (bi, L.RCV_P_X5, pidx[id(net.classifier.bias)])]
            dnext = head_info["dx"]
        for st in reversed(stage_info):
            b, bi = st["bwd"], len(bwd)
            if st["last"]:
                self.gout_slots.append(("bwd", bi, L.RCV_P_IN))
            else:
                b.p[L.RCV_P_IN] = self._ptr(dnext)
                b.p[L.RCV_P_IN_AUX] = self._ptr(st["out"])
            b.p[L.RCV_P_X1] = self._ptr(st["arg"])
            if st["first"]:
                self.x_slots.append(("bwd", bi, L.RCV_P_EPI_AUX))
            else:
                b.p[L.RCV_P_EPI_AUX] = self._ptr(st["x"])
            b.p[L.RCV_P_OUT] = self._ptr(st["dx"])
            b.p[L.RCV_P_PART] = self._ptr(st["ws"])
            bwd.append(b)
            self.param_slots.append(("bwd", bi, L.RCV_P_W, pidx[id(st["conv"].weight)]))
            self.grad_slots += [(bi, L.RCV_P_X2, pidx[id(st["conv"].weight)]), (bi, L.RCV_P_X3, pidx[id(st["conv"].bias)])]
            dnext = st["dx"]
        return bwd

    def launches(self):
        """Library launches of (forward, backward): a backward record is its kernel plus the row reduction."""
        return self.fwd.n, 2 * self.bwd.n

    def set_params(self, params):
        for which, oi, slot, pi in self.param_slots:
            (self.fwd if which == "fwd" else self.bwd).arr[oi].p[slot] = params[pi].data_ptr()

    def set_slots(self, slots, tensor):
        for which, oi, slot in slots:
            (self.fwd if which == "fwd" else self.bwd).arr[oi].p[slot] = tensor.data_ptr()


class _BNNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, plan, x, *params):
        plan.set_params(params)
        plan.set_slots(plan.x_slots, x)
        out = torch.empty(plan.out_shape, dtype=torch.float32, device=x.device)
        plan.set_slots(plan.out_slots, out)
        net._fill_dropout(plan)
        plan.fwd.run(plan.handle, torch.cuda.current_stream(x.device).cuda_stream)
        plan.x = x
        plan.generation += 1
        ctx.plan, ctx.generation = plan, plan.generation
        return out

    @staticmethod
    def backward(ctx, grad_out):
        plan = ctx.plan
        if not plan.backward:
            raise L.RcvError("this forward ran without gradients enabled; it kept nothing for a backward")
        if plan.generation != ctx.generation:
            raise L.RcvError("backward of a forward whose buffers a later forward of the same shape has overwritten")
        g = grad_out.detach().to(torch.float32).contiguous()
        flat = torch.empty(plan.grad_numel, dtype=torch.float32, device=g.device)
        base = flat.data_ptr()
        for oi, slot, pi in plan.grad_slots:
            plan.bwd.arr[oi].p[slot] = base + 4 * plan.grad_offsets[pi]
        plan.set_slots(plan.gout_slots, g)
        plan.bwd.run(plan.handle, torch.cuda.current_stream(g.device).cuda_stream)
        offs = plan.grad_offsets
        grads = []
        for k, need in enumerate(ctx.needs_input_grad[3:]):
            n = (offs[k + 1] if k + 1 < len(offs) else plan.grad_numel) - offs[k]
            grads.append(flat[offs[k]:offs[k] + n].view(plan.param_shapes[k]) if need else None)
        return (None, None, None, *grads)


class _BNNBase(nn.Module):
    _has_head = False

    def _stages(self):
        raise NotImplementedError

    def _num_classes(self) -> int:
        return int(self.classifier.out_channels)

    def _plan_for(self, N, C, H, W, dropout, backward, handle, device) -> _Plan:
        plans = self.__dict__.setdefault("_plans", {})
        key = (N, C, H, W, dropout, backward, None if device is None else str(device))
        plan = plans.get(key)
        if plan is None:
            if len(plans) >= 8:
                plans.clear()
            plan = _Plan(self, N, C, H, W, dropout, backward, handle, device)
            plan.param_shapes = [tuple(p.shape) for p in self.parameters()]
            plans[key] = plan
        return plan

    def _plan_records(self, N, C, H, W, handle=None, training=True):
        """(tests, tools) The validated records of one batch shape without a device: ``(forward, backward)`` lists of RcvOp.  Raises what
        the library's workspace query refuses."""
        plan = _Plan(self, N, C, H, W, training, training, handle if handle is not None else L.planner_handle(256), None)
        return [plan.fwd.arr[k] for k in range(plan.fwd.n)], [plan.bwd.arr[k] for k in range(plan.bwd.n)]

    def __getstate__(self):                      # copy.deepcopy / pickling: the plans (device buffers, ctypes records) stay behind
        d = self.__dict__.copy()
        d.pop("_plans", None)
        d.pop("_last_plan", None)
        return d

    def _apply(self, fn, *args, **kwargs):      # .to() / .cuda() / .float(): the plans hold device buffers
        self.__dict__.pop("_plans", None)
        self.__dict__.pop("_last_plan", None)
        return super()._apply(fn, *args, **kwargs)

    # ---- dropout hooks (the names of Engine's) ----
    def _impose_dropout(self, scales: Optional[List[torch.Tensor]]):
        """(tests) Use these keep-scales, in forward order (do1, do2, do3 as float [N][C] holding 0 or 1/(1-p); BNN-L's dof as
        [N][h][w][512] holding 0 or 2), instead of drawing them in every following training forward; None draws again.  A list that
        does not fit the batch shape is refused at the forward."""
        if scales is not None:
            want = [int(conv.out_channels) for conv, pool, do, relu in self._stages() if do is not None]
            scales = [s.detach().to(torch.float32).contiguous() for s in scales]
            ok = len(scales) == len(want) + (1 if self._has_head else 0)
            ok = ok and all(s.dim() == 2 and s.shape[1] == c and s.shape[0] == scales[0].shape[0] for s, c in zip(scales, want))
            if ok and self._has_head:
                s = scales[-1]
                ok = s.dim() == 4 and s.shape[3] == int(self.fc.out_channels) and s.shape[0] == scales[0].shape[0]
            if not ok:
                raise L.RcvError("%s takes the keep-scales %s%s of one batch, got %s" % (
                    type(self).__name__, ", ".join("[N][%d]" % c for c in want),
                    " and [N][h][w][%d]" % int(self.fc.out_channels) if self._has_head else "", [tuple(s.shape) for s in scales]))
        self.__dict__["_imposed"] = scales

    def _last_dropout_scales(self) -> Optional[List[torch.Tensor]]:
        """(tests) The keep-scales the last training forward used, in forward order, or None."""
        plan = self.__dict__.get("_last_plan")
        if plan is None or plan.keep_views is None:
            return None
        return [v.clone() for v in plan.keep_views]

    def _fill_dropout(self, plan: _Plan):
        self.__dict__["_last_plan"] = plan
        if plan.keep_views is None:
            return
        imposed = self.__dict__.get("_imposed")
        if imposed is not None:
            if len(imposed) != len(plan.keep_views) or any(tuple(s.shape) != tuple(v.shape) for s, v in zip(imposed, plan.keep_views)):
                raise L.RcvError("the imposed dropout keep-scales %s do not fit this batch: %s expected (impose one list per batch shape, "
                                 "or None to draw again)" % ([tuple(s.shape) for s in imposed], [tuple(v.shape) for v in plan.keep_views]))
            for s, v in zip(imposed, plan.keep_views):
                v.copy_(s)
        else:
            torch.bernoulli(plan.keep_prob, out=plan.keep_flat)
            plan.keep_flat.mul_(plan.keep_scale)

    # ---- the module surface ----
    def _checked_input(self, x, what):
        if not torch.is_tensor(x):
            raise TypeError("%s: x must be a tensor" % what)
        if x.device.type != "cuda":
            raise L.RcvError("%s runs on the HIP device only (input on %s); there is no CPU path" % (what, x.device))
        if x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("%s expects float32 [B,3,H,W], got %s %s" % (what, x.dtype, tuple(x.shape)))
        for p in self.parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise L.RcvError("%s: parameter on %s (%s) but the input on %s; move the module with .to()" % (what, p.device, p.dtype, x.device))
        return x.detach().contiguous()

    def forward(self, x):
        """x float32 [B,3,H,W] on the HIP device -> float32 logits [B,4,h,w] (a 32x32 patch gives [B,4,1,1])."""
        name = type(self).__name__
        xc = self._checked_input(x, name)
        if x.requires_grad and self.training:
            raise L.RcvError("%s does not produce a gradient for its input (the first stage computes none); pass a tensor with "
                             "requires_grad=False" % name)
        backward = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        N, C, H, W = xc.shape
        idx = xc.device.index if xc.device.index is not None else torch.cuda.current_device()
        plan = self._plan_for(N, C, H, W, bool(self.training), backward, L.handle(idx), xc.device)
        return _BNNFunction.apply(self, plan, xc, *self.parameters())

    def predict(self, x):
        """The class of every patch (pixel of the logit plane) on the device: uint8 [B,h,w], the FIRST maximum of the logits ``self(x)``
        writes in eval mode, bit for bit -- written by the last launch itself, no logits are stored.  Eval mode only."""
        name = type(self).__name__
        if self.training:
            raise L.RcvError("predict is an inference call and this module is in training mode: call `.eval()` first")
        xc = self._checked_input(x, name + ".predict")
        with torch.no_grad():
            N, C, H, W = xc.shape
            idx = xc.device.index if xc.device.index is not None else torch.cuda.current_device()
            plan = self._plan_for(N, C, H, W, False, False, L.handle(idx), xc.device)
            plan.set_params(list(self.parameters()))
            plan.set_slots(plan.x_slots, xc)
            labels = torch.empty(plan.head_shape, dtype=torch.uint8, device=xc.device)
            last = plan.fwd.arr[plan.fwd.n - 1]
            slot = L.RCV_P_X3 if self._has_head else L.RCV_P_X2
            last.p[L.RCV_P_OUT] = None
            last.p[slot] = labels.data_ptr()
            try:
                plan.fwd.run(plan.handle, torch.cuda.current_stream(xc.device).cuda_stream)
            finally:
                last.p[slot] = None
            plan.generation += 1
            return labels


class BNNL(_BNNBase):
    """BNN-L (model.py:569-594): three 8x8 conv stages with MaxPool2d(4,2), then fc 16->512, Dropout, ReLU, classifier 512->4."""
    _has_head = True

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 8, padding=4)
        self.conv2 = nn.Conv2d(8, 16, 8, padding=3)
        self.conv3 = nn.Conv2d(16, 16, 8, padding=3)
        self.fc = nn.Conv2d(16, 512, 1)
        self.classifier = nn.Conv2d(512, 4, 1)

        self.relu = nn.ReLU()

        self.pool1 = nn.MaxPool2d(4, 2)
        self.pool2 = nn.MaxPool2d(4, 2)
        self.pool3 = nn.MaxPool2d(4, 2)

        self.do1 = nn.Dropout2d(0.25)
        self.do2 = nn.Dropout2d(0.25)
        self.do3 = nn.Dropout2d(0.25)
        self.dof = nn.Dropout(0.5)

    def _stages(self):
        return [(self.conv1, self.pool1, self.do1, True), (self.conv2, self.pool2, self.do2, True), (self.conv3, self.pool3, self.do3, True)]


class BNNMC(_BNNBase):
    """BNN-M-C (model.py:596-619): 5x5 / 3x3 / 3x3 conv stages with MaxPool2d(4,2), (4,2), (2,2), then a 3x3 classifier without padding."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 5, padding=1)
        self.conv2 = nn.Conv2d(8, 16, 3, padding=1)
        self.conv3 = nn.Conv2d(16, 16, 3, padding=1)
        self.classifier = nn.Conv2d(16, 4, 3)

        self.relu = nn.ReLU()

        self.pool1 = nn.MaxPool2d(4, 2)
        self.pool2 = nn.MaxPool2d(4, 2)
        self.pool3 = nn.MaxPool2d(2, 2)

        self.do1 = nn.Dropout2d(0.25)
        self.do2 = nn.Dropout2d(0.25)
        self.do3 = nn.Dropout2d(0.25)

    def _stages(self):
        return [(self.conv1, self.pool1, self.do1, True), (self.conv2, self.pool2, self.do2, True), (self.conv3, self.pool3, self.do3, True),
                (self.classifier, None, None, False)]
