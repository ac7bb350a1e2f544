"""LabelProp's input from a prediction (RCV_OP_LP_INPUT, ``labelprop_next``, ``labelprop_batch(prior_logits=...)``,
``infer.LabelPropagator``) without a device: the float64 restatement (tests/lp_input_restatement.py) pinned to torch on the CPU, what
the library's query accepts and refuses, the argument errors of the Python surface, and the proof that the soft prior's rounding bound
tells the wrong kernels apart."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lp_input_restatement as R      # noqa: E402
import robocupvision_amd      # noqa: E402
import robocupvision_amd.model as M      # noqa: E402
from oracle import cpu_reference as O      # noqa: E402
from robocupvision_amd import _lib as L      # noqa: E402
from robocupvision_amd import infer      # noqa: E402


# ------------------------------------------------------------------------------------------ the restatement against torch
def _frames(B, C, H, W, seed):
    return np.random.default_rng(seed).standard_normal((B, C, H, W)).astype(np.float32)


def test_hard_prior_equals_label_to_pred():
    lab = np.random.default_rng(1).integers(0, 5, (3, 7, 5))
    ref = O.label_to_pred(torch.from_numpy(lab), 5)
    assert np.array_equal(R.hard_prior(lab), ref.double().numpy())
    assert np.array_equal(R.hard_prior(lab.astype(np.uint8)), ref.double().numpy())


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_out_of_range_values_select_no_class(dtype):
    lab = R.class_map_case(1, 7, 5, 2, dtype)
    p = R.hard_prior(lab)
    outside = (lab.astype(np.int64) < 0) | (lab.astype(np.int64) >= 5)
    assert outside.any() and (~outside).any()
    assert (p[:, :, outside[0]] == -1).all()
    assert ((p == 1).sum(axis=1) == (~outside)).all()           # exactly one +1 where the value is a class, none elsewhere
    for v in (5, 255) + ((-100, 2 ** 32 + 2) if dtype == np.int64 else ()):
        assert (lab == v).any()


def test_stream_form_is_the_loop_body_of_makeLPImages():
    cur, prev = _frames(3, 3, 13, 17, 3), _frames(3, 1, 13, 17, 4)
    lab = np.random.default_rng(5).integers(0, 5, (3, 13, 17))
    tc, tp = torch.from_numpy(cur), torch.from_numpy(prev)
    ref = torch.cat([tc[:, 0:1], tp[:, 0:1], tc[:, 0:1] - tp[:, 0:1], O.label_to_pred(torch.from_numpy(lab), 5)], 1)
    assert np.array_equal(R.lp_input(cur, prev, lab), ref.double().numpy())
    assert np.array_equal(R.lp_input(cur, prev[:, 0], lab), ref.double().numpy())      # a [B,H,W] plane is channel 0


def test_pair_form_is_the_assembly_loop_of_labelPropTrain():
    """labelPropTrain.py:177-193 written with torch ops."""
    images = torch.from_numpy(_frames(6, 3, 8, 9, 6)).view(3, 2, 3, 8, 9)
    labels = torch.from_numpy(np.random.default_rng(7).integers(0, 5, (3, 2, 8, 9)))
    inputs, outputs = torch.empty(6, 8, 8, 9), torch.empty(6, 8, 9, dtype=torch.int64)
    cnt = 0
    for img, lab in zip(images, labels):
        preds = O.label_to_pred(lab, 5)
        inputs[cnt] = torch.cat([img[0][0][None], img[1][0][None], (img[0][0] - img[1][0])[None], preds[1]])
        inputs[cnt + 1] = torch.cat([img[1][0][None], img[0][0][None], (img[1][0] - img[0][0])[None], preds[0]])
        outputs[cnt], outputs[cnt + 1] = lab[0], lab[1]
        cnt += 2
    got = R.lp_input(images.numpy(), None, labels.view(6, 8, 9).numpy(), pair=True)
    assert np.array_equal(got, inputs.double().numpy())
    assert torch.equal(outputs, labels.view(6, 8, 9))              # the script's targets are the label tensor itself
    both = O.labelprop_inputs(images[1, 0, 0], images[1, 1, 0], labels[1, 0], labels[1, 1])
    assert np.array_equal(got[2:4], both.double().numpy())


@pytest.mark.parametrize("case", ["ordinary", "equal", "spread60", "offset1e4"])
def test_soft_prior_equals_torch_softmax_in_float64(case):
    z = R.soft_logit_cases(2, 6, 7, 11)[case]
    ref = torch.softmax(torch.from_numpy(z).double(), 1) * 2 - 1
    assert np.abs(R.soft_prior(z) - ref.numpy()).max() <= 1e-14
    assert np.isfinite(R.soft_prior(z)).all()


def test_the_bound_is_what_the_derivation_gives():
    u = 2.0 ** -24
    dq = (1 / np.e + 4 / np.e + 13) * u
    assert 2 * dq + u <= R.SOFT_BOUND <= 1.1 * (2 * dq + u)


def _fp32_contract(z):
    """The op's stated arithmetic in float32 numpy (np.exp for expf): what a correct kernel computes, to expf's last bits."""
    z = z.astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    S = (((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]) + e[:, 4]
    return np.float32(2) * (e / S[:, None]) - np.float32(1)


def test_the_bound_admits_the_contract_and_excludes_the_wrong_kernels():
    cases = R.soft_logit_cases(2, 8, 8, 13)
    leaves = {v: set() for v in R.VARIANTS if v}
    for name, z in cases.items():
        ref = R.soft_prior(z)
        assert np.abs(_fp32_contract(z).astype(np.float64) - ref).max() <= R.SOFT_BOUND, name
        for v in ("no_max", "no_scale", "class_order"):
            if not (np.abs(R.soft_prior(z, v) - ref) <= R.SOFT_BOUND).all():      # (NaN leaves the bound too)
                leaves[v].add(name)
        cur = _frames(2, 3, 8, 8, 14).reshape(1, 2, 3, 8, 8)
        full, own = R.lp_input(cur, None, z, pair=True), R.lp_input(cur, None, z, pair=True, variant="own_prior")
        assert np.array_equal(full[:, :3], own[:, :3])
        if not (np.abs(own - full) <= R.SOFT_BOUND).all():
            leaves["own_prior"].add(name)
    assert "offset1e4" in leaves["no_max"]                          # exp(1e4) overflows: inf / inf
    assert leaves["no_scale"] == set(cases)
    assert {"ordinary", "spread60", "offset1e4"} <= leaves["class_order"]
    assert {"ordinary", "spread60", "offset1e4"} <= leaves["own_prior"]


# ------------------------------------------------------------------------------------------ the library's query
def _op(n=2, h=3, w=4, cin=3, cout=5, inmode=L.LP_PRIOR_U8, aux0=0, **kw):
    return L.make_op(L.OP_LP_INPUT, 0, n=n, h=h, w=w, cin=cin, cout=cout, inmode=inmode, aux0=aux0, **kw)


def _label(op):
    return L.OpList([op]).labels(L.planner_handle(256))[0]


def test_the_op_kind_and_entry_point_exist():
    assert L.OP_LP_INPUT == 59 and "rcv_lp_input" in L.EXPORTS and L.load().rcv_lp_input.argtypes
    assert (L.LP_PRIOR_U8, L.LP_PRIOR_LOGITS, L.LP_PRIOR_I64) == (1, 4, 8)


@pytest.mark.parametrize("mode,name", [(1, "u8"), (8, "i64"), (4, "logits")])
def test_the_query_names_the_kernel(mode, name):
    assert _label(_op(inmode=mode)) == "lp_input<%s,stream>" % name
    assert _label(_op(inmode=mode, aux0=1)) == "lp_input<%s,pair>" % name
    assert _label(_op(inmode=mode, aux1=1)) == "lp_input<%s,stream>" % name          # previous frames as planes
    op = _op(inmode=mode, n=32, h=120, w=160)
    assert L.op_workspace(L.planner_handle(256), op) == 0 and op.i[L.RCV_I_NPART] == 0
    _label(_op(n=1, h=4096, w=8192, cin=1))                        # 2^28 output elements: accepted


@pytest.mark.parametrize("op,what", [
    (lambda: _op(cout=4), "4 classes unsupported"),
    (lambda: _op(cout=8), "8 classes unsupported"),
    (lambda: _op(inmode=0), "prior form 0 unsupported"),
    (lambda: _op(inmode=2), "prior form 2 unsupported"),
    (lambda: _op(aux0=2), "pairing 2 unsupported"),
    (lambda: _op(aux0=-1), "pairing -1 unsupported"),
    (lambda: _op(n=3, aux0=1), "even number of frames (got 3)"),
    (lambda: _op(n=0), "shape 0 x 3 x 3 x 4 unsupported"),
    (lambda: _op(cin=0), "shape 2 x 0 x 3 x 4 unsupported"),
    (lambda: _op(h=0), "shape 2 x 3 x 0 x 4 unsupported"),
    (lambda: _op(w=-1), "shape 2 x 3 x 3 x -1 unsupported"),
    (lambda: _op(n=4, h=8192, w=8192, cin=1), "fewer than 2^31 elements"),          # the output: 2^28 pixels x 8
    (lambda: _op(n=1, h=4096, w=8192, cin=64), "fewer than 2^31 elements"),         # the frames: 2^25 pixels x 64 channels
    (lambda: _op(n=1, h=4096, w=8192, cin=1, aux1=64), "fewer than 2^31 elements"),  # the previous frames
    (lambda: _op(aux1=-1), "-1 channels in the previous frames"),
])
def test_the_query_refuses_with_a_message(op, what):
    with pytest.raises(L.RcvError) as e:
        _label(op())
    assert what in str(e.value), str(e.value)
    with pytest.raises(L.RcvError) as e:      # the workspace query refuses the same records with the same words
        L.op_workspace(L.planner_handle(256), op())
    assert what in str(e.value), str(e.value)


def test_a_planner_handle_enqueues_nothing():
    lib = L.load()
    assert lib.rcv_lp_input(L.planner_handle(256), None, None, 0, None, 1, 0, 2, 3, 8, 8, 5, None, None, None) != 0


# ------------------------------------------------------------------------------------------ argument errors of the Python surface
def test_labelprop_next_argument_errors():
    cur, prev = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8)
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    assert robocupvision_amd.labelprop_next is M.labelprop_next and "labelprop_next" in M.__all__
    with pytest.raises(TypeError):
        M.labelprop_next(cur.numpy(), prev, lab)
    with pytest.raises(TypeError):
        M.labelprop_next(cur.double(), prev, lab)
    with pytest.raises(TypeError):
        M.labelprop_next(cur, prev.half(), lab)
    with pytest.raises(TypeError):
        M.labelprop_next(cur, prev, lab.to(torch.int32))
    with pytest.raises(TypeError):
        M.labelprop_next(cur, prev, None)
    with pytest.raises(ValueError):
        M.labelprop_next(cur[0, 0], prev, lab)
    with pytest.raises(ValueError):
        M.labelprop_next(cur, torch.zeros(2, 8, 9), lab)
    with pytest.raises(ValueError):
        M.labelprop_next(cur, prev, torch.zeros(3, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        M.labelprop_next(cur, prev, torch.zeros(2, 4, 8, 8))           # logits with four classes
    with pytest.raises(ValueError):
        M.labelprop_next(cur, prev, torch.zeros(2, 8, 8))              # a float prior must be logits
    for prior in (lab, lab.long(), torch.zeros(2, 5, 8, 8)):
        with pytest.raises(L.RcvError, match="HIP device only"):
            M.labelprop_next(cur, prev, prior, keep_plane=True)


def test_labelprop_batch_prior_logits_argument_errors():
    images, labels, z = torch.zeros(2, 2, 3, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.int64), torch.zeros(2, 2, 5, 8, 8)
    with pytest.raises(TypeError):
        M.labelprop_batch(images, labels, prior_logits=z.double())
    with pytest.raises(TypeError):
        M.labelprop_batch(images, labels, prior_logits=z.numpy())
    with pytest.raises(TypeError):
        M.labelprop_batch(images, labels.int(), prior_logits=z)
    with pytest.raises(ValueError):
        M.labelprop_batch(images, labels, prior_logits=z.view(4, 5, 8, 8))
    with pytest.raises(ValueError):
        M.labelprop_batch(images, labels, prior_logits=torch.zeros(2, 2, 4, 8, 8))
    with pytest.raises(ValueError):
        M.labelprop_batch(images, labels[:1], prior_logits=z)
    with pytest.raises(ValueError):
        M.labelprop_batch(images, labels, 4, prior_logits=z)
    with pytest.raises(L.RcvError, match="HIP device only"):
        M.labelprop_batch(images, labels, prior_logits=z)
    with pytest.raises(L.RcvError, match="HIP device only"):      # without the keyword: the call it always was
        M.labelprop_batch(images, labels)


def test_label_propagator_argument_errors():
    seg, lp = M.ROBO_UNet(), M.LabelProp(5, 32)
    assert robocupvision_amd.LabelPropagator is infer.LabelPropagator
    p = infer.LabelPropagator(seg.train(), lp.train(), key_every=3, soft=True)
    assert not seg.training and not lp.training and p.key_every == 3 and p.soft
    with pytest.raises(TypeError, match="seg_model"):
        infer.LabelPropagator(torch.nn.Conv2d(3, 5, 1), lp)
    with pytest.raises(TypeError, match="lp_model"):
        infer.LabelPropagator(seg, torch.nn.Conv2d(8, 5, 1))
    with pytest.raises(L.RcvError, match="classify mode"):
        infer.LabelPropagator(M.PB_FCN(32, 5, 1, False, 1), lp)
    with pytest.raises(ValueError, match="key_every"):
        infer.LabelPropagator(seg, lp, key_every=-1)
    with pytest.raises(ValueError, match="key_every"):
        infer.LabelPropagator(seg, lp, key_every=2.5)
    with pytest.raises(TypeError):
        p(torch.zeros(2, 3, 24, 32, dtype=torch.float64))
    with pytest.raises(TypeError):
        p(torch.zeros(3, 24, 32))
    with pytest.raises(L.RcvError, match="HIP device only"):
        p(torch.zeros(2, 3, 24, 32))
