"""GPU: the masked SGD step.  rcv_sgd_step_pruned against rcv_sgd_step on a gradient zeroed by hand (what ``param.grad[indices] = 0``
between backward and ``optimizer.step()`` leaves, trainer.py:220-226), bit for bit; and the prune phase of trainer.py /
labelPropTrain.py as a whole: Trainer + optim.SGD + Trainer.prune against the autograd path with the literal loop."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import cpu_reference as O
import labelprop_restatement as LR
from robocupvision_amd import _lib as L
import robocupvision_amd.model as M
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PB_W = [1, 6, 1.5, 3, 3]          # trainer.py:135


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _step(pruned, p, g, buf, lre, mask, n, lr, mom, wd, step, gs):
    lib, h, s = L.load(), L.handle(0), torch.cuda.current_stream().cuda_stream
    lre_ptr = lre.data_ptr() if lre is not None else None
    if pruned:
        rc = lib.rcv_sgd_step_pruned(h, p.data_ptr(), g.data_ptr(), buf.data_ptr(), lre_ptr, mask.data_ptr() if mask is not None else None,
                                     n, lr, mom, wd, step, gs, s)
    else:
        rc = lib.rcv_sgd_step(h, p.data_ptr(), g.data_ptr(), buf.data_ptr(), lre_ptr, n, lr, mom, wd, step, gs, s)
    L.check(rc, "rcv_sgd_step")


@pytest.mark.parametrize("mom", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_masked_step_equals_step_on_zeroed_gradient(n, mom):
    rng = np.random.default_rng(1000 + n)
    lr, wd, gs = 0.2, 1e-3, 0.25
    p0 = rng.standard_normal(n).astype(np.float32)
    mask = rng.random(n) < 0.4
    mask[0] = True
    lre = np.full(n, lr, np.float32)
    for lo in range(5, n, 97):                              # stretches of lr_elem == 0: parameters outside the graph
        lre[lo:lo + 13] = 0.0
    mask_d = _dev(mask.astype(np.uint8))
    for with_lre in (False, True):
        lre_d = _dev(lre) if with_lre else None
        # a: the masked launch; b: the plain launch on a gradient zeroed by hand; c / d: the masked entry with a null mask and the plain one
        pa, pb, pc, pd = (_dev(p0) for _ in range(4))
        ba, bb, bc, bd = (torch.full((n,), 123.0, device=DEV) for _ in range(4))        # ignored at step 1
        for step in (1, 2, 3):
            g = rng.standard_normal(n).astype(np.float32)
            g0 = g.copy()
            g0[mask] = 0.0
            _step(True, pa, _dev(g), ba, lre_d, mask_d, n, lr, mom, wd, step, gs)
            _step(False, pb, _dev(g0), bb, lre_d, None, n, lr, mom, wd, step, gs)
            _step(True, pc, _dev(g), bc, lre_d, None, n, lr, mom, wd, step, gs)
            _step(False, pd, _dev(g), bd, lre_d, None, n, lr, mom, wd, step, gs)
            assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(_bits(ba), _bits(bb)), (n, mom, with_lre, step)
            assert np.array_equal(_bits(pc), _bits(pd)) and np.array_equal(_bits(bc), _bits(bd)), (n, mom, with_lre, step)
        if with_lre:
            dead = lre == 0
            assert np.array_equal(_bits(pa)[dead], p0.view(np.uint32)[dead]) and bool((ba.cpu().numpy()[dead] == 123.0).all())
        if n > 1:
            assert not np.array_equal(_bits(pa), _bits(pd))             # the mask does something


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _prune_phase(make_model, x, t, weights, sgd_kw, rule, kw):
    """Run A: Trainer + fused SGD + Trainer.prune.  Run B: the autograd path, a second fused SGD without a mask, and the literal
    ``param.grad[indices] = 0`` loop before ``opt.step()``.  Parameters must agree bit for bit after each of three steps."""
    torch.manual_seed(12345678)
    ma = make_model().to(DEV)
    torch.manual_seed(12345678)
    mb = make_model().to(DEV)
    tr = Trainer(ma, class_weights=weights, optimizer=SGD(ma, **sgd_kw))
    masks_a = _quiet(tr.prune, rule, **kw)
    masks_b = _quiet(getattr(M, rule), mb.parameters(), **kw)
    assert len(masks_a) == len(masks_b) > 0 and all(torch.equal(a, b) for a, b in zip(masks_a, masks_b))
    assert sum(int(m.sum()) for m in masks_a) > 100
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
    opt_b = SGD(mb, **sgd_kw)
    crit = M.CrossEntropyLoss2d(torch.tensor(weights, dtype=torch.float32)).to(DEV)
    for step in range(3):
        tr.step(x, t)
        mb.train()
        opt_b.zero_grad()
        loss = crit(mb(x), t)
        loss.backward()
        k = 0
        for p in mb.parameters():
            if p.dim() > 1:
                if p.grad is not None:
                    p.grad[masks_b[k]] = 0
                k += 1
        opt_b.step()
        for (name, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            assert np.array_equal(_bits(pa.detach()), _bits(pb.detach())), "step %d: %s differs" % (step + 1, name)
    big = [p for p in ma.parameters() if p.dim() > 1]
    for p, m in zip(big, masks_a):
        assert float(p.detach()[m].abs().sum()) == 0.0            # fresh optimizer: wd * 0 + 0 keeps a pruned weight at exactly 0
    return tr, masks_a


def test_pb_fcn_prune_phase_matches_the_literal_loop():
    x, t = O.synthetic_batch(2, 32, 32, seed=5)
    tr, masks = _prune_phase(lambda: M.PB_FCN(32, 5, 1, False, 0), x.to(DEV), t.to(DEV), PB_W,
                             dict(lr=1e-1, momentum=0.1, weight_decay=1e-3), "pruneModel2", dict(ratio=0.3, lT=1000, hT=50000))
    assert tr.optimizer._prune_flat is not None and tr.prune_indices is not None


def test_labelprop_prune_phase_matches_the_literal_loop():
    im, lab = LR.synthetic_pairs(2, 24, 32, 13)
    x, t = M.labelprop_batch(im.to(DEV), lab.to(DEV))
    _prune_phase(lambda: M.LabelProp(5, 32, 0.0), x, t, list(LR.LP_WEIGHTS), dict(lr=1e-1, momentum=0.1, weight_decay=1e-3),
                 "pruneModel", dict(lower=73, upper=77))


def test_masks_built_on_the_flat_layout_are_used_as_they_are():
    """After the engine has laid the parameters out, the builders' one mask buffer mirrors the flat parameter buffer and both
    optimizers take it as their flat mask without rebuilding it; the stale packed filters are dropped by Trainer.prune."""
    torch.manual_seed(12345678)
    model = M.PB_FCN(32, 5, 1, False, 0).to(DEV)
    x, t = O.synthetic_batch(2, 32, 32, seed=5)
    x, t = x.to(DEV), t.to(DEV)
    tr = Trainer(model, class_weights=PB_W, optimizer=SGD(model, lr=1e-1, momentum=0.0, weight_decay=1e-3))
    tr.step(x, t)
    fl = model._get_engine().flat
    masks = _quiet(tr.prune, "pruneModel2", ratio=0.3, lT=1000, hT=50000)
    store = masks[0].untyped_storage()
    assert store.nbytes() == fl.numel
    tr.step(x, t)
    flat = tr.optimizer._prune_flat
    assert flat.data_ptr() == store.data_ptr() and flat.numel() == fl.numel
    big = [k for k, p in enumerate(fl.params) if p.dim() > 1]
    assert int(flat.sum()) == sum(int(m.sum()) for m in masks)
    for k, m in zip(big, masks):
        assert torch.equal(flat[fl.offsets[k]:fl.offsets[k] + m.numel()].view(m.shape).bool(), m)
        assert float(fl.params[k].detach()[m].abs().sum()) == 0.0
    from robocupvision_amd.optim import _adopt_flat_mask
    assert _adopt_flat_mask(masks, fl).data_ptr() == store.data_ptr()
    assert _adopt_flat_mask([m.clone() for m in masks], fl) is None                     # arbitrary user masks keep the old path
