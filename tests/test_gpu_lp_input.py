"""GPU: LabelProp's input from a prediction (RCV_OP_LP_INPUT, csrc/lp_input.hip) against the float64 restatement
(tests/lp_input_restatement.py) -- hard priors bit for bit, the soft prior inside the counted rounding bound -- the pair form against
``labelprop_batch``, the kept plane and the NHWC layout, and ``infer.LabelPropagator`` against the same frames run through the ops that
existed before it.

The soft prior's bound (derived at lp_input_restatement.SOFT_BOUND; u = 2^-24): out_c = 2 * (e_c / S) - 1 with d_c = z_c - m one
rounding (it moves e_c by the relative amount |d_c| u), expf within 2 ulp = 4 u relative (ASSUMED: ROCm's table of device-function
accuracy is not at hand), the four additions of S (4 u), the division (u): |d q_c| <= (5 / e + 13) u = 14.84 u since q_c |d_c| <= 1 / e,
q_c <= 1 and S >= 1; doubling is exact and the final subtraction rounds a value of magnitude <= 1 (u): 30.7 u, stated as 32 u =
1.9e-6 absolute.  Eager ``torch.softmax(z, 1) * 2 - 1`` in fp32 is granted the same bound against float64, hence twice the bound
between the two."""
import numpy as np
import pytest
import torch

import lp_input_restatement as R
import robocupvision_amd.model as M
from robocupvision_amd import _lib as L
from robocupvision_amd import infer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, H, W, C): pixel counts that are no multiple of 64 or 256 (the grid-stride tail), C = 3 (a wrong plane stride shows)
SHAPES = [(1, 7, 5, 1), (3, 13, 17, 3), (2, 24, 40, 3), (4, 16, 16, 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))


def _frames(B, C, H, W, seed):
    return np.random.default_rng(seed).standard_normal((B, C, H, W)).astype(np.float32)


# ------------------------------------------------------------------------------------------ hard priors: exact
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_hard_prior_equals_the_restatement(si, dtype):
    B, H, W, C = SHAPES[si]
    cur, prev = _frames(B, C, H, W, 10 + si), _frames(B, C, H, W, 20 + si)
    lab = R.class_map_case(B, H, W, 30 + si, dtype)
    for prev_form in (prev, prev[:, 0]):                      # frames of C channels, and [B,H,W] planes
        got = M.labelprop_next(_dev(cur), _dev(prev_form), _dev(lab))
        assert tuple(got.shape) == (B, 8, H, W) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), _f32(R.lp_input(cur, prev_form, lab)))
    outside = torch.from_numpy((lab.astype(np.int64) < 0) | (lab.astype(np.int64) >= 5))
    assert bool(outside.any()) and bool((got.cpu()[:, 3:].permute(0, 2, 3, 1)[outside] == -1).all())


def test_hard_prior_past_the_grid_cap():
    """33 x 120 x 160 = 633 600 pixels: more than the 8 x 256 CUs x 256 threads of the capped grid, so the grid-stride loop takes a
    second, partial round; an odd sample count in the stream form."""
    B, H, W, C = 33, 120, 160, 1
    cur, prev = _frames(B, C, H, W, 140), _frames(B, C, H, W, 141)
    lab = R.class_map_case(B, H, W, 142, np.uint8)
    got, plane = M.labelprop_next(_dev(cur), _dev(prev[:, 0]), _dev(lab), keep_plane=True)
    assert torch.equal(got.cpu(), _f32(R.lp_input(cur, prev, lab)))
    assert torch.equal(plane.cpu(), torch.from_numpy(cur[:, 0]))


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_pair_form_with_int64_labels_is_labelprop_batch(si):
    P, H, W, C = SHAPES[si]                                   # P pairs = 2P frames
    B = 2 * P
    images = _dev(_frames(B, C, H, W, 40 + si).reshape(P, 2, C, H, W))
    labels = _dev(R.class_map_case(B, H, W, 50 + si, np.int64).reshape(P, 2, H, W))
    ref, tgt = M.labelprop_batch(images, labels)
    n = B * H * W * 8
    out = torch.full((n + 256,), float("nan"), device=DEV)      # a guard behind the output: nothing may be written there
    op = L.make_op(L.OP_LP_INPUT, 0, n=B, h=H, w=W, cin=C, cout=5, inmode=L.LP_PRIOR_I64, aux0=1, p_in=images.data_ptr(),
                   p_x0=labels.data_ptr(), p_out=out.data_ptr())
    L.OpList([op]).run(L.handle(0), torch.cuda.current_stream(DEV).cuda_stream)
    assert torch.equal(out[:n].view(B, H, W, 8).permute(0, 3, 1, 2), ref)
    assert bool(torch.isnan(out[n:]).all())
    assert torch.equal(tgt, labels.view(B, H, W))


# ------------------------------------------------------------------------------------------ the soft prior: inside the bound
CASES = ["ordinary", "equal", "spread60", "offset1e4"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_soft_prior_is_inside_the_rounding_bound(si, case):
    B, H, W, C = SHAPES[si]
    cur, prev = _frames(B, C, H, W, 60 + si), _frames(B, 1, H, W, 70 + si)
    z = R.soft_logit_cases(B, H, W, 80 + si)[case]
    ref = R.lp_input(cur, prev, z)
    zd = _dev(z)
    got = M.labelprop_next(_dev(cur), _dev(prev), zd)
    assert torch.equal(got[:, :3].cpu(), _f32(ref[:, :3]))
    err = float(np.abs(got[:, 3:].cpu().double().numpy() - ref[:, 3:]).max())
    eager = torch.softmax(zd, 1) * 2 - 1
    gap = float((got[:, 3:] - eager).abs().max())
    print("soft prior %s %s: max error %.3e = %.2f of the bound; against eager torch %.3e = %.2f of twice the bound"
          % (case, SHAPES[si], err, err / R.SOFT_BOUND, gap, gap / (2 * R.SOFT_BOUND)))
    assert bool(torch.isfinite(got).all())
    assert err <= R.SOFT_BOUND
    assert gap <= 2 * R.SOFT_BOUND


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_labelprop_batch_with_prior_logits(si):
    P, H, W, C = SHAPES[si]
    B = 2 * P
    images = _frames(B, C, H, W, 90 + si).reshape(P, 2, C, H, W)
    labels = _dev(R.class_map_case(B, H, W, 91 + si, np.int64).reshape(P, 2, H, W))
    z = R.soft_logit_cases(B, H, W, 92 + si)["ordinary"]
    inputs, targets = M.labelprop_batch(_dev(images), labels, prior_logits=_dev(z).view(P, 2, 5, H, W))
    ref = R.lp_input(images, None, z, pair=True)
    assert tuple(inputs.shape) == (B, 8, H, W) and inputs.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(inputs[:, :3].cpu(), _f32(ref[:, :3]))
    err = float(np.abs(inputs[:, 3:].cpu().double().numpy() - ref[:, 3:]).max())
    print("pair form, soft prior %s: max error %.3e = %.2f of the bound" % (SHAPES[si], err, err / R.SOFT_BOUND))
    assert err <= R.SOFT_BOUND
    assert tuple(targets.shape) == (B, H, W) and targets.data_ptr() == labels.data_ptr() and torch.equal(targets, labels.view(B, H, W))
    # without the keyword: the op and the result it always had
    plain, tgt = M.labelprop_batch(_dev(images), labels)
    assert torch.equal(plain.cpu(), _f32(R.lp_input(images, None, labels.view(B, H, W).cpu().numpy(), pair=True)))
    assert tgt.data_ptr() != labels.data_ptr()


# ------------------------------------------------------------------------------------------ kept plane and layout
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_kept_plane_and_layout(si):
    B, H, W, C = SHAPES[si]
    cur, prev = _dev(_frames(B, C, H, W, 100 + si)), _dev(_frames(B, C, H, W, 110 + si))
    lab = _dev(R.class_map_case(B, H, W, 120 + si, np.uint8))
    inputs, plane = M.labelprop_next(cur, prev, lab, keep_plane=True)
    assert torch.equal(plane, cur[:, 0]) and plane.is_contiguous() and plane.data_ptr() != cur.data_ptr()
    assert inputs.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(inputs, M.labelprop_next(cur, prev, lab))


@pytest.mark.parametrize("size", [(16, 16), (24, 40)])
def test_labelprop_in_training_mode_reads_it_without_a_relayout(size):
    H, W = size
    torch.manual_seed(3)
    model = M.LabelProp(5, 32).to(DEV).train()
    cur, prev = _dev(_frames(2, 3, H, W, 130)), _dev(_frames(2, 3, H, W, 131))
    for prior in (_dev(R.class_map_case(2, H, W, 132, np.uint8)), _dev(R.soft_logit_cases(2, H, W, 133)["ordinary"])):
        out = model(M.labelprop_next(cur, prev, prior))
        assert tuple(out.shape) == (2, 5, H, W) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------ the driver
def _count(obj, name, log, tag):
    fn = getattr(obj, name)

    def counted(*a, **kw):
        log.append(tag)
        return fn(*a, **kw)
    setattr(obj, name, counted)
    return fn


def _models():
    torch.manual_seed(12345678)
    return M.ROBO_UNet().to(DEV), M.LabelProp(5, 32).to(DEV)


def _stream(n, B=2, H=24, W=32):
    return [_dev(_frames(B, 3, H, W, 200 + k)) for k in range(n)]


def test_label_propagator_hard():
    seg, lp = _models()
    p = infer.LabelPropagator(seg, lp, key_every=3)
    log = []
    seg_predict, lp_predict = _count(seg, "predict", log, "seg"), _count(lp, "predict", log, "lp")
    frames = _stream(5)
    prev_img = prev_lab = None
    for k, imgs in enumerate(frames):
        labels = p(imgs)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (2, 24, 32)
        if k in (0, 3):
            assert torch.equal(labels, seg_predict(imgs))
        else:
            # today's ops: the fake pair [cur, prev], labels [anything, prior], labelprop_batch, the even samples gathered contiguous
            pair = torch.stack([imgs, prev_img], 1)
            lab2 = torch.stack([torch.zeros_like(prev_lab, dtype=torch.int64), prev_lab.long()], 1)
            x = M.labelprop_batch(pair, lab2)[0].permute(0, 2, 3, 1)[0::2].contiguous().permute(0, 3, 1, 2)
            assert torch.equal(labels, lp_predict(x))
        prev_img, prev_lab = imgs, labels
    assert log == ["seg", "lp", "lp", "seg", "lp"]
    # colour is palette[labels]; reset() makes the next call a key frame
    del log[:]
    p.reset()
    labels, colour = p(frames[0], colour=True)
    assert log == ["seg"] and torch.equal(labels, seg_predict(frames[0]))
    assert colour.dtype == torch.uint8 and tuple(colour.shape) == (2, 24, 32, 3)
    labels2, colour2 = p(frames[1], colour=True)
    assert log == ["seg", "lp"] and torch.equal(colour2, infer.device_palette(None, DEV)[labels2.long()])
    with pytest.raises(L.RcvError, match="reset"):
        p(_stream(1, B=1)[0])
    with pytest.raises(L.RcvError, match="reset"):
        p(_stream(1, H=32)[0])
    assert log == ["seg", "lp"]
    p.reset()
    assert tuple(p(_stream(1, H=32)[0]).shape) == (2, 32, 32) and log == ["seg", "lp", "seg"]


def test_label_propagator_key_every_0_has_one_key_frame():
    seg, lp = _models()
    p = infer.LabelPropagator(seg, lp)
    log = []
    _count(seg, "predict", log, "seg"), _count(lp, "predict", log, "lp")
    for imgs in _stream(4):
        p(imgs)
    assert log == ["seg", "lp", "lp", "lp"]


def test_label_propagator_soft():
    seg, lp = _models()
    p = infer.LabelPropagator(seg, lp, key_every=3, soft=True)
    log = []
    seg_forward, lp_forward = _count(seg, "forward", log, "seg"), _count(lp, "forward", log, "lp")
    for k, imgs in enumerate(_stream(5)):
        plane_prev, logits_prev = p.plane, p.prior
        labels = p(imgs)
        logits = p.prior
        assert tuple(logits.shape) == (2, 5, 24, 32) and logits.dtype == torch.float32
        assert labels.dtype == torch.uint8 and torch.equal(labels.long(), torch.max(logits, 1)[1])
        assert torch.equal(p.plane, imgs[:, 0])
        with torch.no_grad():
            if k in (0, 3):
                assert torch.equal(logits, seg_forward(imgs))
            else:
                assert torch.equal(logits, lp_forward(M.labelprop_next(imgs, plane_prev, logits_prev)))
    assert log == ["seg", "lp", "lp", "seg", "lp"]
