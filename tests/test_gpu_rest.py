"""GPU: the rest of the reference's ``model.py`` -- ConvPoolDouble, ConvSep, trConvSep as standalone blocks and FCN as a network, in
training and in inference with the trained weights the reference ships for it -- against the golden vectors of the imported
reference (tests/golden/make_golden_rest.py).  Bars: those of tests/test_gpu_blocks.py (blocks) and of
tests/test_gpu_pbfcn.py::test_pb_fcn_step_vs_golden_small (the training step)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, sd_hash
import batch_prep_restatement as BR
import robocupvision_amd
import robocupvision_amd.model as M
from robocupvision_amd import data as D
from robocupvision_amd.metrics import ValidationState
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer
from test_gpu_blocks import close, _t, _load_block, _run_block
from test_gpu_net import check_mask
from test_gpu_pbfcn import pb_step, _check_after, PB_W
from test_rest import load_parts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rest_kats():
    return load_parts("rest_kats")


@pytest.fixture(scope="module")
def rest_meta():
    with open(os.path.join(GOLDEN, "rest.json")) as f:
        return json.load(f)


class _Kats:
    """The ``.files`` / item surface of an npz over the union of the fixture's parts (what _load_block and _run_block read)."""

    def __init__(self, d):
        self.d, self.files = d, list(d)

    def __getitem__(self, k):
        return self.d[k]


@pytest.mark.parametrize("name,cin,cout", [("cpd_16_32", 16, 32), ("cpd_32_64", 32, 64)])
def test_conv_pool_double_block(rest_kats, name, cin, cout):
    kats = _Kats(rest_kats)
    _run_block(kats, name, _load_block(kats, name, M.ConvPoolDouble(cin, cout)))


def _run_sep_block(kats, name, mod):
    """_run_block for a block with two BatchNorms (bn1, bn2 in place of the single ``bn`` that helper reads): train-mode output, input
    gradient, every parameter gradient, the running statistics of both, then the eval-mode output -- same bars."""
    x = _t(kats[name + "/x"]).to(DEV).requires_grad_(True)
    mod.train()
    y = mod(x)
    close(y, _t(kats[name + "/y_train"]), name + " y_train")
    y.backward(_t(kats[name + "/gy"]).to(DEV))
    torch.cuda.synchronize()
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        close(p.grad, _t(kats["%s/g/%s" % (name, k)]), "%s grad %s" % (name, k), floor=1.0)
    close(x.grad, _t(kats[name + "/gx"]), name + " gx", floor=1.0)
    for bn in ("bn1", "bn2"):
        close(getattr(mod, bn).running_mean, _t(kats["%s/after/%s.running_mean" % (name, bn)]), "%s %s running_mean" % (name, bn))
        close(getattr(mod, bn).running_var, _t(kats["%s/after/%s.running_var" % (name, bn)]), "%s %s running_var" % (name, bn))
        assert int(getattr(mod, bn).num_batches_tracked) == 1
    mod.eval()
    with torch.no_grad():
        ye = mod(x.detach())
    close(ye, _t(kats[name + "/y_eval"]), name + " y_eval")


@pytest.mark.parametrize("name,make", [("convsep_16_32_s1", lambda: M.ConvSep(16, 32, 3, 1)), ("convsep_16_32_s2", lambda: M.ConvSep(16, 32, 3, 2)),
                                       ("trconvsep_32_16", lambda: M.trConvSep(32, 16)), ("convsep_64_128_s1", lambda: M.ConvSep(64, 128, 3, 1)),
                                       ("trconvsep_128_64", lambda: M.trConvSep(128, 64))])
def test_separable_blocks_vs_reference(rest_kats, name, make):
    """ConvSep / trConvSep (model.py:333-377) at 2x16x9x13, 2x16x10x14 (stride 2), 2x32x5x7, 1x64x6x10 and 1x128x3x5: the 1-D pair as one
    cross-filter 3x3 record, the 1x1 conv on the pointwise family; the transposed pair's centre gradient reaches both parameters."""
    kats = _Kats(rest_kats)
    mod = _load_block(kats, name, make())
    _run_sep_block(kats, name, mod)
    labels = mod._engine._last[0].fwd.labels(mod._engine.handle)
    assert any(l.startswith("pw_mfma") for l in labels) and any(l.startswith("cross_pack") for l in labels), labels


def _fcn_with(name):
    m = M.FCN()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in load_parts("rest_" + name).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def fcn_nets():
    return {name: _fcn_with(name) for name in ("seg1", "seg1_pruned")}


@pytest.mark.parametrize("shape", [(2, 3, 48, 64), (1, 3, 120, 160)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["seg1", "seg1_pruned"])
def test_fcn_eval_with_the_shipped_weights(rest_kats, rest_meta, fcn_nets, name, shape):
    """FCN in eval mode with bestModelSeg1.pth / bestModelSeg1FinetunedPruned.pth (parameter arrays from the fixtures; 73.7 % of the
    pruned one's conv weights are zero): logits within close(), the mask exact outside the golden near-ties, ``predict`` the arg-max
    of the module's own logits bit for bit, ``validate`` booking CrossEntropyLoss2d's loss, count_zero_weights as stored."""
    tag = "%s_%s" % (name, "x".join(map(str, shape)))
    info = rest_meta["checkpoints"][name]
    net = fcn_nets[name]
    gg = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=gg).to(DEV)
    t = _t(rest_kats[tag + "/t"]).to(DEV)
    near = rest_kats[tag + "/near_tie_idx"]
    pixels = shape[0] * shape[2] * shape[3]
    assert near.size <= 1e-3 * pixels, "the fixture has %d near-ties of %d pixels: not a usable case" % (near.size, pixels)
    with torch.no_grad():
        logits = net(x)
    close(logits, _t(rest_kats[tag + "/logits"]), tag + " logits")
    check_mask(torch.max(logits, 1)[1], rest_kats[tag + "/argmax"], near, tag)
    lab = net.predict(x)
    assert lab.dtype == torch.uint8 and torch.equal(lab, torch.max(logits, 1)[1].to(torch.uint8))
    w = torch.tensor(PB_W, dtype=torch.float32, device=DEV)
    state = ValidationState(5, DEV)
    lab2 = net.validate(x, t, state, weight=w, labels=True)
    assert torch.equal(lab2, lab)
    loss = float(M.CrossEntropyLoss2d(w)(logits, t))
    got = state.compute()
    print("%s: loss %.8f (module) %.8f (validate) %.8f (reference)" % (tag, loss, got["loss"], info["eval"][tag]["loss"]))
    assert abs(got["loss"] - loss) <= 1e-5 * abs(loss)          # 16-channel tail: sums over other pixel sets, equal to rounding
    assert abs(loss - info["eval"][tag]["loss"]) <= 1e-3 * info["eval"][tag]["loss"]
    assert M.count_zero_weights(net) == pytest.approx(info["count_zero_weights"], abs=1e-7)


def test_fcn_through_the_segmenter(fcn_nets):
    """detect.py's frames -> class map and colour mask with FCN as the network: the composition of the loader and ``predict``."""
    net = fcn_nets["seg1"]
    frames = torch.from_numpy(np.ascontiguousarray(BR.synthetic_frames(2, 48, 64, 9)[0])).to(DEV)
    lab, col = robocupvision_amd.Segmenter(net, img_size=(48, 64))(frames)
    imgs = D.prepare_batch(frames, torch.zeros(2, 48, 64, dtype=torch.uint8, device=DEV), (48, 64), train=False)[0]
    want = torch.max(net(imgs), 1)[1].to(torch.uint8)
    assert tuple(lab.shape) == (2, 48, 64) and torch.equal(lab, want) and tuple(col.shape) == (2, 48, 64, 3)


@pytest.mark.parametrize("fused", [False, True], ids=["torch_sgd", "fused_sgd"])
def test_fcn_step_vs_golden(rest_kats, rest_meta, fused):
    """trainer.py:205-221 on FCN: two optim.SGD steps (lr 1e-1, momentum 0.5, weight decay 1e-3, weights [1, 6, 1.5, 3, 3]) from seed
    12345678 at 2x3x48x64, the bars of test_pb_fcn_step_vs_golden_small.  The reference has 2 near-ties of 6 144 pixels here."""
    tag = "fcn_2x48x64"
    m = rest_meta[tag]
    torch.manual_seed(12345678)
    model = M.FCN()
    assert sd_hash(model.state_dict()) == m["sd_hash_init"]
    model = model.to(DEV)
    x, t = _t(rest_kats[tag + "/x"]).to(DEV), _t(rest_kats[tag + "/t"]).to(DEV)
    opt = SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3) if fused else None
    res = pb_step(model, x, t, opt)
    close(res["pred"], _t(rest_kats[tag + "/logits"]), tag + " logits")
    assert abs(res["loss"] - m["loss"]) <= 1e-3 * abs(m["loss"])
    assert rest_kats[tag + "/near_tie_idx"].size == m["near_ties"] == 2
    check_mask(res["pc"], rest_kats[tag + "/argmax"], rest_kats[tag + "/near_tie_idx"], tag)
    assert sorted(k for k, g in res["grads"].items() if g is None) == sorted(m["none_grads"]) == []
    for k, g in res["grads"].items():
        if k.startswith("up") and k.endswith("conv.bias"):
            continue
        key = "%s/grad/%s" % (tag, k)
        if key in rest_kats:
            close(g, _t(rest_kats[key]), "%s grad %s" % (tag, k), rtol=1e-3, floor=1.0)
        else:
            n_ = m["grad_summary"][k][2]
            gn = float(g.double().norm())
            assert abs(gn - n_) <= 1e-3 * n_ + 1e-7, (k, gn, n_)
            close(g.reshape(-1)[:64], _t(rest_kats["%s/grad_head/%s" % (tag, k)]), "%s grad head %s" % (tag, k), rtol=1e-3, floor=1.0)
    sd = model.state_dict()
    for k in rest_kats:
        if k.startswith(tag + "/after/"):
            close(sd[k[len(tag) + 7:]], _t(rest_kats[k]), k)
    _check_after(sd, m["param_after_step_sum"], 0.1)
    res2 = pb_step(model, x, t, res["opt"])
    assert abs(res2["loss"] - m["loss_step2"]) <= 2e-3 * abs(m["loss_step2"]), (res2["loss"], m["loss_step2"])
    _check_after(model.state_dict(), m["param_after_2_steps_sum"], 0.2)
    model.eval()
    with torch.no_grad():
        pe = model(x)
    close(pe, _t(rest_kats[tag + "/eval_logits"]), tag + " eval logits", rtol=5e-3)


def test_fcn_step_through_the_trainer(rest_kats, rest_meta):
    """The same two steps once through Trainer (fused SGD, the loss from the metrics)."""
    tag = "fcn_2x48x64"
    m = rest_meta[tag]
    torch.manual_seed(12345678)
    model = M.FCN().to(DEV)
    x, t = _t(rest_kats[tag + "/x"]).to(DEV), _t(rest_kats[tag + "/t"]).to(DEV)
    tr = Trainer(model, class_weights=PB_W, optimizer=SGD(model, lr=1e-1, momentum=0.5, weight_decay=1e-3))
    pred = tr.step(x, t).clone()
    met = tr.pop_metrics()
    assert abs(met["loss"] - m["loss"]) <= 1e-3 * abs(m["loss"])
    close(pred, _t(rest_kats[tag + "/logits"]), tag + " logits through Trainer")
    ndiff = check_mask(torch.max(pred, 1)[1], rest_kats[tag + "/argmax"], rest_kats[tag + "/near_tie_idx"], tag)
    assert abs(met["correct_pixels"] - m["correct"]) <= ndiff
    _check_after(model.state_dict(), m["param_after_step_sum"], 0.1)
    tr.step(x, t)
    assert abs(tr.pop_metrics()["loss"] - m["loss_step2"]) <= 2e-3 * abs(m["loss_step2"])
    _check_after(model.state_dict(), m["param_after_2_steps_sum"], 0.2)
