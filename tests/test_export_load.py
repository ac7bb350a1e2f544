"""CPU: robot-side exports for every network and reading them back (robocupvision_amd/export.py): ``net_cfg`` against the layer-settings
files the reference ships (tests/golden/export_lp/net.cfg, export_vga.cfg), ``save_export`` against ``saveParams``, ``loadParams`` as
its inverse, ``load_export`` of the shipped LabelProp export and of round trips -- the lowered graph must be the module's own
``_graph()``, node for node -- and every refusal."""
import os

import numpy as np
import pytest
import torch

import robocupvision_amd
import robocupvision_amd.model as M
from conftest import GOLDEN
from robocupvision_amd import _lib as L
from robocupvision_amd import export as E

LP_CFG, LP_DAT = os.path.join(GOLDEN, "export_lp", "net.cfg"), os.path.join(GOLDEN, "export_lp", "weights.dat")


def _lines(text):
    return [l.strip() for l in text.strip().splitlines() if l.strip()]          # whitespace-normalised, as tests/test_export.py


def signature(graph):
    """A graph without its tensors: the input layout and, per node, every key with a tensor replaced by its shape and a BatchNorm
    by its width."""
    def plain(v):
        if torch.is_tensor(v):
            return ("tensor",) + tuple(v.shape)
        if isinstance(v, torch.nn.BatchNorm2d):
            return ("bn", v.num_features)
        return v
    return [graph["inputs"][0]["layout"]] + [{k: plain(v) for k, v in d.items()} for d in graph["nodes"]]


def seeded(make, seed=1):
    """The model with seeded random parameters and BatchNorm running statistics."""
    torch.manual_seed(seed)
    m = make()
    with torch.no_grad():
        for b in m.modules():
            if isinstance(b, torch.nn.BatchNorm2d):
                b.running_mean.normal_()
                b.running_var.uniform_(0.5, 2.0)
                b.weight.uniform_(0.5, 1.5)
                b.bias.normal_()
                b.num_batches_tracked.fill_(7)
    return m


MODELS = {"robo_unet": lambda: M.ROBO_UNet(), "robo_unet_noscale": lambda: M.ROBO_UNet(noScale=True),
          "robo_unet_cls5": lambda: M.ROBO_UNet(classSize=5), "fcn": lambda: M.FCN(), "pb_fcn": lambda: M.PB_FCN(32, 5, 1, False, 0),
          "pb_fcn_noscale": lambda: M.PB_FCN(32, 5, 1, True, 0), "pb_fcn_2": lambda: M.PB_FCN_2(False), "labelprop": lambda: M.LabelProp(5, 32, 0.0)}
SAVEPARAMS_EQUAL = ("robo_unet", "robo_unet_noscale", "robo_unet_cls5", "fcn", "labelprop")


def test_exported_names():
    for name in ("net_cfg", "save_export", "load_export", "ExportedNet", "saveParams", "loadParams"):
        assert getattr(robocupvision_amd, name) is getattr(E, name)


def test_net_cfg_labelprop_is_the_shipped_file():
    with open(LP_CFG) as f:
        assert _lines(E.net_cfg(M.LabelProp(5, 32, 0.0))) == _lines(f.read())


def test_net_cfg_vga_is_the_shipped_file():
    with open(os.path.join(GOLDEN, "export_vga.cfg")) as f:
        ref = _lines(f.read())
    assert _lines(E.net_cfg(M.PB_FCN(32, 5, 1, True, 0), img_shape=(480, 640))) == ref
    own = _lines(E.net_cfg(M.PB_FCN(32, 5, 1, True, 0)))
    assert [a for a, b in zip(own, ref) if a != b] == ["height=240", "width=320"]


def test_net_cfg_block_forms():
    text = E.net_cfg(M.ROBO_UNet())
    assert "[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\ndilation=1\nactivation=relu\nhasBias=1\n\n[batchnorm]\nactivation = linear\n" in text
    assert text.startswith("[net]\nheight=120\nwidth=160\nchannels=3\ndownscale=4\n") and text.endswith("[softmax]\n")
    assert "size=5\nstride=1\npad=2\nactivation=linear\n\n[softmax]" in E.net_cfg(M.ROBO_UNet(classSize=5))
    fcn = E.net_cfg(M.FCN())          # ConvPoolDouble: two relu convs, the stride-2 conv, [batchnorm] activation = relu
    assert ("activation=relu\nhasBias=0\n\n[convolutional]\nfilters=32\nsize=3\nstride=1\npad=2\ndilation=2\nactivation=relu\nhasBias=0\n\n"
            "[convolutional]\nfilters=32\nsize=3\nstride=2\npad=1\ndilation=1\nactivation=linear\nhasBias=0\n\n[batchnorm]\nactivation = relu") in fcn
    words = set(l for l in _lines("\n".join(E.net_cfg(mk()) for mk in MODELS.values())) if l.startswith("["))
    assert words == {"[net]", "[convolutional]", "[batchnorm]", "[transposedconv]", "[shortcut]", "[softmax]"}


def test_load_export_of_the_shipped_labelprop():
    net = E.load_export(LP_CFG, LP_DAT)
    dat = np.fromfile(LP_DAT, dtype=np.float64)
    assert dat.size == 92837
    sd = net.state_dict()
    assert not any(k.endswith("num_batches_tracked") for k in sd)
    assert np.array_equal(np.concatenate([v.numpy().reshape(-1).astype(np.float64) for v in sd.values()]), dat)
    assert all(v.dtype == torch.float32 for v in sd.values())          # (the file's values are fp32 values)
    assert signature(net._graph()) == signature(M.LabelProp(5, 32)._graph())
    assert net.net == {"height": 120, "width": 160, "channels": 8, "downscale": 4} and not net.training
    # the same values through loadParams into the module: equal state
    lp = E.loadParams(os.path.dirname(LP_DAT), M.LabelProp(5, 32, 0.0))
    a = [v for k, v in lp.state_dict().items() if not k.endswith("num_batches_tracked")]
    assert len(a) == len(sd) and all(torch.equal(x, y) for x, y in zip(a, sd.values()))


@pytest.mark.parametrize("name", list(MODELS), ids=list(MODELS))
def test_round_trip_graph_and_values(name, tmp_path):
    m = seeded(MODELS[name])
    E.save_export(str(tmp_path), m)
    with open(tmp_path / "net.cfg") as f:
        assert f.read() == E.net_cfg(m)
    dat = np.fromfile(str(tmp_path / "weights.dat"), dtype=np.float64)
    flat = E.flat_params(m)
    if name in SAVEPARAMS_EQUAL:
        assert dat.tobytes() == flat.tobytes()          # bit for bit saveParams' file
    else:                                               # ... minus the pooled patch head, which the layer list does not contain
        keep = np.concatenate([v.numpy().reshape(-1).astype(np.float64) for k, v in m.state_dict().items() if not k.startswith("classifier.")])
        assert dat.tobytes() == keep.tobytes() and dat.size < flat.size
        if name != "pb_fcn_2":      # PB_FCN: skipClassifier drops the segmenter too (`segmenter.classifier.*`); PB_FCN_2's is `segmenter.layers.Class.*`
            assert E.flat_params(m, skipClassifier=True).size < dat.size
        else:
            assert E.flat_params(m, skipClassifier=True).tobytes() == dat.tobytes()
    net = E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "weights.dat"))
    assert signature(net._graph()) == signature(m._graph())
    sd = net.state_dict()
    assert np.array_equal(np.concatenate([v.numpy().reshape(-1).astype(np.float64) for v in sd.values()]), dat)
    assert sum(k.endswith("num_batches_tracked") for k in sd) == len(M._bn_modules(m)) and all(
        int(v) == 7 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    # the tensors of corresponding nodes are equal, not only their shapes
    for a, b in zip(net._graph()["nodes"], m._graph()["nodes"]):
        for k in ("weight", "bias"):
            assert (a.get(k) is None) == (b.get(k) is None) and (a.get(k) is None or torch.equal(a[k], b[k].detach()))
        if b.get("bn") is not None:
            for k in ("weight", "bias", "running_mean", "running_var"):
                assert torch.equal(getattr(a["bn"], k), getattr(b["bn"], k).detach())


def test_img_shape_and_lowering_on_the_planner(tmp_path):
    """An export lowers to the plan of its module: same record kinds, eval and eval-proba (planning handle, no device)."""
    from robocupvision_amd.engine import Engine
    m = seeded(MODELS["robo_unet"])
    E.save_export(str(tmp_path), m, img_shape=(48, 64))
    net = E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "weights.dat"))
    assert (net.net["height"], net.net["width"]) == (48, 64)
    x = torch.zeros(2, 3, 48, 64)
    kinds = []
    for mod in (net, m):
        eng = Engine(mod._graph(), list(mod.parameters()), M._bn_modules(mod), dry_run=True)
        ev, pr = eng._plan_for([x], False), eng._plan_for([x], False, labels="proba")
        kinds.append(([op.kind for op in ev.fwd.arr[:ev.fwd.n]], [op.kind for op in pr.fwd.arr[:pr.fwd.n]]))
        assert [k for (_, k) in eng.plans] == [False, ()]          # a truth value for every reader of the cache: only True is training
        assert pr.fwd.labels(eng.handle)[-1] == "cls_proba" and pr.label_op == pr.fwd.n - 1 and pr.label_classes == 5
        assert pr.logits is None and ev.bytes - pr.bytes == 4 * 2 * 5 * 48 * 64
        assert kinds[-1][1][:-1] == kinds[-1][0][:-1] and kinds[-1][1][-1] == L.OP_CLS_PROBA == 67
    assert kinds[0] == kinds[1]


def test_with_and_without_num_batches_tracked(tmp_path):
    m = seeded(MODELS["labelprop"])
    E.save_export(str(tmp_path), m)
    full = np.fromfile(str(tmp_path / "weights.dat"), dtype=np.float64)
    bare = np.concatenate([v.numpy().reshape(-1).astype(np.float64) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")])
    assert full.size == bare.size + 10
    bare.tofile(str(tmp_path / "bare.dat"))
    a = E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "weights.dat"))
    b = E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "bare.dat"))
    assert len(a.state_dict()) == len(b.state_dict()) + 10
    for k, v in b.state_dict().items():
        assert torch.equal(v, a.state_dict()[k])
    # loadParams takes both as well, and says both counts when neither fits
    for fname in ("weights.dat", "bare.dat"):
        fresh = E.loadParams(str(tmp_path), M.LabelProp(5, 32, 0.0), fname)
        for (k, v), w in zip(fresh.state_dict().items(), m.state_dict().values()):
            assert torch.equal(v, w) or (k.endswith("num_batches_tracked") and fname == "bare.dat" and int(v) == 0)
    bare[:-1].tofile(str(tmp_path / "short.dat"))
    for call in (lambda: E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "short.dat")),
                 lambda: E.loadParams(str(tmp_path), M.LabelProp(5, 32, 0.0), "short.dat")):
        with pytest.raises(ValueError, match=r"%d values.*%d \(%d with" % (bare.size - 1, bare.size, full.size)):
            call()


@pytest.mark.parametrize("name", ["robo_unet", "pb_fcn", "fcn"])
def test_loadparams_inverts_saveparams(name, tmp_path):
    m = seeded(MODELS[name], seed=3)
    E.saveParams(str(tmp_path), m, "w.dat")
    fresh = E.loadParams(str(tmp_path), MODELS[name](), "w.dat")
    assert list(fresh.state_dict()) == list(m.state_dict())
    for v, w in zip(fresh.state_dict().values(), m.state_dict().values()):
        assert v.dtype == w.dtype and torch.equal(v, w)
    E.saveParams(str(tmp_path), fresh, "again.dat")
    assert (tmp_path / "again.dat").read_bytes() == (tmp_path / "w.dat").read_bytes()


def test_saveparams_file_of_a_pb_fcn_is_refused(tmp_path):
    m = seeded(MODELS["pb_fcn"])
    E.save_export(str(tmp_path), m)
    E.saveParams(str(tmp_path), m, "all.dat")
    n_all, n_cfg = E.flat_params(m).size, np.fromfile(str(tmp_path / "weights.dat"), dtype=np.float64).size
    assert n_all == n_cfg + 64 * 5 + 5
    with pytest.raises(ValueError, match=r"%d values.*takes %d \(%d with" % (n_all, n_cfg - len(M._bn_modules(m)), n_cfg)):
        E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "all.dat"))


def test_writer_refusals():
    with pytest.raises(TypeError, match="concatenat"):
        E.net_cfg(M.ROBO_UNet(v2=True, classSize=3))
    with pytest.raises(TypeError, match="max-pool"):
        E.net_cfg(M.ROBO_UNet(pool=True))
    with pytest.raises(TypeError, match="classify mode"):
        E.net_cfg(M.PB_FCN_2(True))
    with pytest.raises(TypeError, match="classify mode"):
        E.net_cfg(M.PB_FCN(32, 5, 1, False, 1))
    with pytest.raises(TypeError, match="segmentation networks"):
        E.net_cfg(M.Conv(8, 8, 3))


def _edited(tmp_path, old, new, count=1):
    with open(LP_CFG) as f:
        text = f.read()
    assert old in text
    path = str(tmp_path / "edited.cfg")
    with open(path, "w") as f:
        f.write(text.replace(old, new, count))
    return path


@pytest.mark.parametrize("old,new,word", [
    ("[softmax]", "[maxpool]\nsize=2\n\n[softmax]", r"section 24 is \[maxpool\]"),
    ("from=5", "from=4", r"section 16 \[shortcut\]: from=4 is not the closing layer"),
    ("from=5", "from=40", r"section 16 \[shortcut\]: from=40 is not the closing layer"),
    ("from=1", "from=7", r"section 22 \[shortcut\]: from=7 has 32 channels, more than the 16"),
    ("[batchnorm]\nactivation = relu\n\n[shortcut]", "[batchnorm]\nactivation = linear\n\n[shortcut]", r"section 15 \[batchnorm\]"),
    ("outpad=1", "outpad=0", r"section 14 \[transposedconv\]"),
    ("size=3\nstride=1\npad=1", "size=3\nstride=1\npad=2", r"section 0 \[convolutional\]: feature convs"),
    ("activation=linear\nhasBias=0\n\n[batchnorm]\nactivation = relu", "activation=relu\nhasBias=0\n\n[batchnorm]\nactivation = relu",
     r"section 1 \[batchnorm\]: conv activation=relu followed by batchnorm activation = relu"),
    ("channels=8", "channels=6", "channels=6"),
    ("hasBias=0", "groups=2", "no key 'groups'"),
    ("[softmax]", "[softmax]\n\n[batchnorm]\nactivation = relu", r"section 25 \[batchnorm\]: nothing may follow"),
    ("[convolutional]\nfilters=5\nsize=1\nstride=1\npad=0\nactivation=linear\n\n[softmax]", "[softmax]", r"section 23 \[softmax\]: a \[softmax\] cannot stand here"),
])
def test_reader_refusals(tmp_path, old, new, word):
    with pytest.raises(ValueError, match=word):
        E.load_export(_edited(tmp_path, old, new), LP_DAT)


def test_exported_net_is_inference_only():
    net = E.load_export(LP_CFG, LP_DAT)
    with pytest.raises(L.RcvError, match="inference network"):
        net.train()
    assert net.eval() is net and not net.training and not any(p.requires_grad for p in net.parameters())
    with pytest.raises(L.RcvError, match="HIP device only"):
        net.proba(torch.zeros(1, 8, 24, 32))
    with pytest.raises(ValueError, match=r"\[B,8,H,W\]"):
        net._engine_inputs(torch.zeros(1, 3, 24, 32))
    with pytest.raises(ValueError, match="multiples of 8"):
        net._engine_inputs(torch.zeros(1, 8, 20, 32))
