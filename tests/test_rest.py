"""Without a GPU: the rest of the reference's ``model.py`` surface -- View, ConvPoolDouble, DownSamplerThick, FCN, ConvSep, trConvSep
(model.py:84-90, 144-164, 235-254, 311-377) -- against the fixtures of tests/golden/make_golden_rest.py: exported names, seeded
construction (state_dict hash), the key lists of the three FCN checkpoints the reference ships, every plan of FCN and of the blocks
on the planner handle, the constructor refusals, the record queries of the pointwise family, and the float64 restatement of that
family and of the cross filters (tests/pw_restatement.py) pinned to torch's float64 conv2d / conv_transpose2d."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, sd_hash
import pw_restatement as R
import robocupvision_amd
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd.engine import Engine

NAMES = ["View", "ConvPoolDouble", "DownSamplerThick", "FCN", "ConvSep", "trConvSep"]
FCN_SHAPES = [(2, 3, 48, 64), (1, 3, 120, 160)]
# the blocks of tests/test_gpu_rest.py: (fixture name, constructor, input N x C x H x W)
BLOCKS = [("convsep_16_32_s1", lambda: M.ConvSep(16, 32, 3, 1), (2, 16, 9, 13)),
          ("convsep_16_32_s2", lambda: M.ConvSep(16, 32, 3, 2), (2, 16, 10, 14)),
          ("trconvsep_32_16", lambda: M.trConvSep(32, 16), (2, 32, 5, 7)),
          ("convsep_64_128_s1", lambda: M.ConvSep(64, 128, 3, 1), (1, 64, 6, 10)),
          ("trconvsep_128_64", lambda: M.trConvSep(128, 64), (1, 128, 3, 5)),
          ("cpd_16_32", lambda: M.ConvPoolDouble(16, 32), (2, 16, 12, 16)),
          ("cpd_32_64", lambda: M.ConvPoolDouble(32, 64), (2, 32, 10, 14))]
PW_PAIRS = [(8, 8), (16, 8), (16, 16), (32, 16), (128, 64), (128, 128)]


def load_parts(prefix):
    """The union of the numbered parts prefix_<i>.npz (make_golden_rest.save_parts)."""
    out = {}
    files = sorted(glob.glob(os.path.join(GOLDEN, prefix + "_[0-9]*.npz")))
    assert files, prefix
    for f in files:
        with np.load(f) as z:
            for k in z.files:
                out[k] = z[k]
    return out


@pytest.fixture(scope="module")
def rest_meta():
    with open(os.path.join(GOLDEN, "rest.json")) as f:
        return json.load(f)


def test_names_are_exported():
    for name in NAMES:
        assert name in M.__all__ and hasattr(M, name) and getattr(robocupvision_amd, name) is getattr(M, name), name
    ns = {}
    exec("from robocupvision_amd.model import *", ns)
    assert all(name in ns for name in NAMES)
    assert M.View(4)(torch.arange(8.0).reshape(2, 2, 2)).shape == (2, 4)


@pytest.mark.parametrize("what,make", [("FCN()", lambda: M.FCN()), ("ConvSep(16,32,3,1)", lambda: M.ConvSep(16, 32, 3, 1)),
                                       ("ConvSep(16,32,3,2)", lambda: M.ConvSep(16, 32, 3, 2)), ("trConvSep(32,16)", lambda: M.trConvSep(32, 16)),
                                       ("ConvPoolDouble(16,32)", lambda: M.ConvPoolDouble(16, 32)),
                                       ("DownSamplerThick(32)", lambda: M.DownSamplerThick(32))])
def test_seeded_construction_matches_the_reference(rest_meta, what, make):
    """Same children in the same order drawing from torch's generator in the same order: the state_dict of a model built after
    torch.manual_seed(12345678) hashes to the reference's (keys and bytes)."""
    torch.manual_seed(12345678)
    assert sd_hash(make().state_dict()) == rest_meta["sd_hash"][what]


def test_parameter_order_of_fcn_is_the_state_dict_order():
    m = M.FCN()
    sd_params = [k for k in m.state_dict() if "running" not in k and "num_batches" not in k]
    assert [k for k, _ in m.named_parameters()] == sd_params
    # (the shipped checkpoints predate num_batches_tracked: 59 keys, 10 fewer than today's state_dict)
    assert len(m.state_dict()) == 69 and sum("num_batches" in k for k in m.state_dict()) == 10


@pytest.mark.parametrize("name", ["seg1", "seg1_finetuned", "seg1_pruned"])
def test_checkpoint_key_lists_load_strictly(rest_meta, name):
    """pth/bestModelSeg1*.pth of the reference: 59 keys, 294 789 elements; a state dict of exactly these keys, shapes and dtypes loads
    with strict=True (they predate ``num_batches_tracked``, which torch then supplies, as it does for the reference)."""
    info = rest_meta["checkpoints"][name]
    assert len(info["keys"]) == 59 and info["elements"] == 294789
    sd = {k: torch.zeros(shape, dtype=getattr(torch, dt)) for k, shape, dt in info["keys"]}
    res = M.FCN().load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [k for k, _, _ in info["keys"]] == [k for k in M.FCN().state_dict() if "num_batches" not in k]


@pytest.mark.parametrize("name", ["seg1", "seg1_pruned"])
def test_stored_checkpoints_load_and_hash(rest_meta, name):
    m = M.FCN()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in load_parts("rest_" + name).items()}, strict=True)
    assert sd_hash(m.state_dict()) == rest_meta["checkpoints"][name]["sd_hash"]
    assert M.count_zero_weights(m) == pytest.approx(rest_meta["checkpoints"][name]["count_zero_weights"], abs=1e-7)


@pytest.mark.parametrize("shape", FCN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("training,labels", [(True, False), (False, False), (False, True), (False, "valid")],
                         ids=["training", "eval", "labels", "valid"])
def test_every_plan_of_fcn_lowers(shape, training, labels):
    """No record of FCN is refused: the 3 -> 16 dilated first layer, 16 -> 16 dilation 2 at full resolution, the two stacked
    relu(conv) of ConvPoolDouble, the 16-channel classifier in all its tails."""
    m = M.FCN()
    eng = Engine(m._graph(), list(m.parameters()), M._bn_modules(m), dry_run=True)
    plan = eng._plan_for([torch.zeros(shape)], training, labels)
    fl = plan.fwd.labels(eng.handle)
    assert len(fl) == plan.fwd.n and fl[-1].startswith({False: "cls_fwd", True: "cls_label", "valid": "valid_fold"}[labels])
    assert sum(l.startswith(("conv", "tconv")) for l in fl) == 14        # 11 convs, 3 transposed convs
    if training:
        bl = plan.bwd.labels(eng.handle)
        assert len(bl) == plan.bwd.n and bl[0] == "cls_bwd" and all(eng.param_used)
    else:
        assert plan.bwd.n == 0 and "combine" not in fl      # folded inference: the skip adds ride in the transposed convs


def _lower_block(make, shape, training):
    mod = make()
    eng = Engine(mod._block_graph(), list(mod.parameters()), M._bn_modules(mod), dry_run=True)
    n, c, h, w = shape
    return mod, eng, eng._plan_for([torch.zeros(n, h, w, c)], training)


@pytest.mark.parametrize("name,make,shape", BLOCKS, ids=[b[0] for b in BLOCKS])
@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
def test_blocks_lower(name, make, shape, training):
    mod, eng, plan = _lower_block(make, shape, training)
    fl = plan.fwd.labels(eng.handle)
    sep = isinstance(mod, (M.ConvSep, M.trConvSep))
    assert sum(l.startswith("pw_mfma") for l in fl) == int(sep) and sum(l.startswith("cross_pack") for l in fl) == int(sep)
    if sep:      # the cross filter is written ahead of the pack launch that reads it
        assert fl.index([l for l in fl if l.startswith("cross_pack")][0]) < fl.index("pack") < plan.n_head + 1
    if training:
        bl = plan.bwd.labels(eng.handle)
        assert all(eng.param_used)
        if sep:
            # data gradient = the same kernel with the filter transposed; the gather closes the list behind every reduction
            assert sum(l.startswith("pw_mfma") and l.endswith(",t>") for l in bl) == 1
            assert sum(l.startswith("pw_wgrad_mfma") for l in bl) == 1 and "pw_wgrad_reduce" in bl
            assert bl[-1].startswith("cross_grad") and max(k for k, l in enumerate(bl) if "reduce" in l) < len(bl) - 1
            assert plan.bwd_marks == [(len(bl), 0)]


def test_constructor_refusals_name_what_is_built():
    with pytest.raises(NotImplementedError, match="size=3"):
        M.ConvSep(16, 32, 5)
    with pytest.raises(NotImplementedError, match="even number of planes"):
        M.ConvSep(16, 31, 3)
    with pytest.raises(L.RcvError, match="FCN's graph"):
        M.DownSamplerThick(32)(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="multiples of 8"):
        M.FCN()._engine_inputs(torch.zeros(1, 3, 12, 16))


def test_getcomp_of_convsep_is_the_reference_formula():
    m = M.ConvSep(16, 32, 3, 2)
    comp, W, H = m.getComp(160, 120, False)
    assert (W, H) == (80, 60) and comp == 3 * 80 * 60 * 16 * 32 * 2 * 2 + 80 * 60 * 32 * 32 * 2 + 80 * 60 * 32 * 8
    with torch.no_grad():
        m.conv_1x1.weight[:16].zero_()
    assert m.getComp(160, 120, True)[0] == 3 * 80 * 60 * 16 * 32 * 2 * 2 + 80 * 60 * 32 * 32 * 2 * 0.5 + 80 * 60 * 32 * 8


# ------------------------------------------------------------------ the pointwise family's records on the planner handle
def _pw(cin, cout, n=2, h=9, w=13, flags=0, **kw):
    return L.make_op(L.OP_PW, flags, n=n, h=h, w=w, cin=cin, cout=cout, **kw)


def test_op_numbers_and_entry_points():
    assert (L.OP_PW, L.OP_PW_WGRAD, L.OP_PW_WGRAD_REDUCE, L.OP_CROSS_PACK, L.OP_CROSS_GRAD) == (62, 63, 64, 65, 66)
    assert L.OP_CONV1X1 == 18 and {"rcv_conv_pw", "rcv_wgrad_pw"} <= set(L.EXPORTS)
    lib, h = L.load(), L.planner_handle(256)
    assert lib.rcv_conv_pw.argtypes and lib.rcv_wgrad_pw.argtypes
    assert lib.rcv_conv_pw(h, L.make_op(L.OP_CONV, 0), None) != 0 and b"RCV_OP_PW" in lib.rcv_last_error()
    assert lib.rcv_wgrad_pw(h, _pw(8, 8), None) != 0 and b"RCV_OP_PW_WGRAD" in lib.rcv_last_error()


@pytest.mark.parametrize("cin,cout", PW_PAIRS + [(24, 40), (8, 128), (128, 8)])
def test_pointwise_records_plan(cin, cout):
    """Rows: one per pixel tile of 64 * WN pixels (WN = 4, or 2 with more than 64 output channels); the filter gradient splits into
    the rows of pw_restatement.wgrad_rows, [Cout][Cin] floats each."""
    h = L.planner_handle(256)
    for (n, hh, ww) in [(1, 1, 1), (2, 9, 13), (3, 16, 20), (64, 60, 80)]:
        P = n * hh * ww
        tile = 128 if cout > 64 else 256
        for flags in (0, L.F_TRANSPOSED_SRC):
            op = _pw(cin, cout, n, hh, ww, flags, stats=L.STATS_FWD)
            assert L.op_workspace(h, op) == -(-P // tile) * 2 * cout * 4 and op.i[L.RCV_I_NPART] == -(-P // tile)
            assert L.OpList([op]).labels(h)[0].startswith("pw_mfma<")
        assert L.op_workspace(h, _pw(cin, cout, n, hh, ww)) == 0
        wop = L.make_op(L.OP_PW_WGRAD, 0, n=n, h=hh, w=ww, cin=cin, cout=cout, inmode2=L.LOAD_GRAD_DEC)
        ns = R.wgrad_rows(P, cin, cout)
        assert L.op_workspace(h, wop) == ns * cin * cout * 4 and wop.i[L.RCV_I_NSPLIT] == ns
        assert L.OpList([L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=cin, cout=cout, nsplit=ns)]).labels(h) == ["pw_wgrad_reduce"]


@pytest.mark.parametrize("op,what", [
    (lambda: _pw(4, 8), "channels 4 -> 8"), (lambda: _pw(8, 136), "channels 8 -> 136"), (lambda: _pw(12, 16), "channels 12 -> 16"),
    (lambda: _pw(8, 8, inmode=L.LOAD_NCHW), "load mode 4"), (lambda: _pw(8, 8, n=0), "empty shape"),
    (lambda: _pw(128, 128, n=4096, h=64, w=64), "2\\^31"), (lambda: _pw(8, 8, stats=7), "statistics kind 7"),
    (lambda: L.make_op(L.OP_PW_WGRAD, 0, n=1, h=4, w=4, cin=8, cout=8, inmode=L.LOAD_GRAD_DEC), "load mode 3 of the layer input"),
    (lambda: L.make_op(L.OP_PW_WGRAD, 0, n=1, h=4, w=4, cin=8, cout=8, inmode2=L.LOAD_AFFINE), "load mode 1 of the output gradient"),
    (lambda: L.make_op(L.OP_PW_WGRAD_REDUCE, 0, cin=8, cout=8, nsplit=0), "0 partial rows"),
    (lambda: L.make_op(L.OP_CROSS_PACK, 0, cin=8, cout=7, aux0=0), "even first dimension"),
    (lambda: L.make_op(L.OP_CROSS_GRAD, 0, cin=8, cout=8, aux0=2), "form 2 unknown"),
])
def test_pointwise_refusals_sit_in_front_of_the_query(op, what):
    with pytest.raises(L.RcvError, match=what):
        L.OpList([op()]).labels(L.planner_handle(256))


# ------------------------------------------------------------------ the float64 restatement against torch
@pytest.mark.parametrize("cin,cout", PW_PAIRS)
def test_restated_pointwise_conv_is_conv2d(cin, cout):
    g = torch.Generator().manual_seed(cin * 131 + cout)
    x, aux, c = torch.randn(2, 9, 13, cin, generator=g), torch.randn(2, 9, 13, cin, generator=g), torch.randn(5, cin, generator=g) * 0.5
    w = torch.randn(cout, cin, 1, 1, generator=g) * 0.1
    bias, scale, resid = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(2, 9, 13, cout, generator=g)
    for mode in (R.LOAD_PLAIN, R.LOAD_AFFINE, R.LOAD_AFFINE_RELU, R.LOAD_GRAD_ENC, R.LOAD_GRAD_DEC):
        v = R.load(mode, x, c, aux)
        ref = F.conv2d(v.permute(0, 3, 1, 2), w.double()).permute(0, 2, 3, 1)
        assert float((R.pw_conv(v, w) - ref).abs().max()) <= 1e-13
    v = R.load(R.LOAD_AFFINE_RELU, x, c)
    ref = F.relu(F.conv2d(v.permute(0, 3, 1, 2), w.double() * scale.double()[:, None, None, None], bias.double())).permute(0, 2, 3, 1) + resid.double()
    assert float((R.pw_conv(v, w, scale=scale, bias=bias, relu=True, resid=resid) - ref).abs().max()) <= 1e-13
    # the data gradient is the same product with the filter transposed, and the filter gradient the pixel sum of outer products
    vd = v.clone().requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    gy = torch.randn(2, 9, 13, cout, generator=g).double()
    F.conv2d(vd.permute(0, 3, 1, 2), wd).permute(0, 2, 3, 1).backward(gy)
    assert float((R.pw_conv(gy, w, transposed=True) - vd.grad).abs().max()) <= 1e-13
    assert float((R.pw_wgrad(v, gy) - wd.grad[:, :, 0, 0]).abs().max()) <= 1e-12


@pytest.mark.parametrize("cin,cout", [(8, 8), (24, 40), (128, 64)])
def test_matmul_form_of_the_restatement_is_the_plain_form(cin, cout):
    """pw_conv / pw_wgrad with matmul=True (what the multi-round GPU cases use at 10^5 pixels): bit for bit the plain form on integer
    operands, where every float64 sum is exact, and within 1e-12 of it on randn (sums of at most 128 / 960 terms of magnitude ~1)."""
    g = torch.Generator().manual_seed(5 * cin + cout)
    ints = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    rnd = lambda *s: torch.randn(*s, generator=g)
    for make, bar in ((ints, 0.0), (rnd, 1e-12)):
        x, gy, resid = make(3, 16, 20, cin), make(3, 16, 20, cout), make(3, 16, 20, cout)
        w, wt, bias = make(cout, cin, 1, 1), make(cin, cout, 1, 1), make(cout)
        scale = torch.randint(1, 4, (cout,), generator=g).float() if bar == 0.0 else torch.rand(cout, generator=g) + 0.5
        pairs = [(R.pw_conv(x, w), R.pw_conv(x, w, matmul=True)),
                 (R.pw_conv(x, w, scale=scale, bias=bias, relu=True), R.pw_conv(x, w, scale=scale, bias=bias, relu=True, matmul=True)),
                 (R.pw_conv(x, wt, transposed=True, resid=resid), R.pw_conv(x, wt, transposed=True, resid=resid, matmul=True)),
                 (R.pw_wgrad(x, gy), R.pw_wgrad(x, gy, matmul=True))]
        for plain, mm in pairs:
            assert plain.shape == mm.shape and plain.dtype == mm.dtype == torch.float64
            if bar == 0.0:
                assert torch.equal(plain, mm)
            else:
                assert float((plain - mm).abs().max()) <= bar


def test_restated_reductions_follow_their_documented_order():
    """pw_reduce: 16 lanes over the rows l, l + 16, ..., lane sums in lane order, rounded once; wgrad5_reduce: rows in order, the filter
    part transposed to [class][CIN][5][5].  On integer rows every order gives the plain sum; on order_sensitive_rows the order shows
    in the fp32 result (rows l and l + 16 exchanged: at least a quarter of the elements change), which is what lets the GPU test see
    a reordered loop."""
    import cls5_restatement as R5
    g = torch.Generator().manual_seed(11)
    for ns in (1, 17, 64, 113):
        part = torch.randint(-9, 10, (ns, 40, 24), generator=g).float()
        assert torch.equal(R.pw_reduce(part).double(), part.double().sum(0)) and torch.equal(R.pw_reduce(part, swap=True), R.pw_reduce(part))
    for ns in (113, 128, 1024):      # (two groups of four per lane or more: the first starts from zero, its order cannot show)
        for shape in ((8, 8), (40, 24)):
            rows = R.order_sensitive_rows(g, ns, *shape)
            changed = float((R.pw_reduce(rows, swap=True) != R.pw_reduce(rows)).float().mean())
            assert changed >= (0.25 if ns >= 128 else 0.02), (ns, shape, changed)      # (113 rows: lane 0 alone has a second group)
    rows = R.order_sensitive_rows(g, 113, 40, 24)
    assert float((R.pw_reduce(rows).double() - rows.double().sum(0)).abs().max()) <= 113 * 2.0 ** -10      # (the big terms cancel)
    part = torch.randint(-9, 10, (7, 25 * 8 * 16 + 8), generator=g).float()
    dw, db = R5.wgrad5_reduce(part, 16, 5)
    total = part.double().sum(0)
    assert dw.shape == (5, 16, 5, 5) and db.shape == (5,)
    for co, ci, t in ((0, 0, 0), (4, 15, 24), (2, 7, 13)):
        assert float(dw[co, ci, t // 5, t % 5]) == float(total[(t * 8 + co) * 16 + ci])
    assert torch.equal(db.double(), total[25 * 8 * 16:25 * 8 * 16 + 5])


@pytest.mark.parametrize("stride", [1, 2])
def test_cross_filter_is_the_concatenated_pair(stride):
    """cat(conv_nx1(x), conv_1xn(x)) == one 3x3 conv with the cross filter: same stride, dilation, padding = dilation (ConvSep's
    own layers, model.py:340-349)."""
    torch.manual_seed(3)
    m = M.ConvSep(16, 32, 3, stride).double()
    x = torch.randn(2, 16, 10, 14, dtype=torch.float64)
    d = 1 if stride > 1 else 2
    ref = torch.cat([m.conv_nx1(x), m.conv_1xn(x)], 1)
    dense = R.cross_pack(m.conv_nx1.weight.detach(), m.conv_1xn.weight.detach(), 0)
    assert float((F.conv2d(x, dense, stride=stride, padding=d, dilation=d) - ref).abs().max()) == 0.0
    ga, gb = R.cross_grad(dense, 0)
    assert torch.equal(ga, m.conv_nx1.weight.detach()) and torch.equal(gb, m.conv_1xn.weight.detach())
    assert int((dense != 0).sum()) == m.conv_nx1.weight.numel() + m.conv_1xn.weight.numel()


def test_cross_filter_is_the_summed_transposed_pair():
    """trconv1x3(x) + trconv3x1(x) == one 3x3 stride-2 transposed conv (pad 1, output_padding 1) with the cross filter whose centre
    is the sum of the two centres; its gradient's centre goes to both filters."""
    torch.manual_seed(4)
    m = M.trConvSep(32, 16).double()
    x = torch.randn(2, 16, 5, 7, dtype=torch.float64)
    a, b = m.trconv1x3.weight, m.trconv3x1.weight
    y = m.trconv1x3(x) + m.trconv3x1(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    dense = R.cross_pack(a.detach(), b.detach(), 1).requires_grad_(True)
    yd = F.conv_transpose2d(x, dense, stride=2, padding=1, output_padding=1)
    assert float((yd - y.detach()).abs().max()) <= 1e-14
    yd.backward(gy)
    ga, gb = R.cross_grad(dense.grad, 1)
    assert float((ga - a.grad).abs().max()) <= 1e-13 and float((gb - b.grad).abs().max()) <= 1e-13
    assert torch.equal(ga[:, :, 0, 1], gb[:, :, 1, 0])
