"""GPU: the softmax tail (RCV_OP_CLS_PROBA, csrc/cls_proba.hip) at record level, through rcv_run on hand-made operands
(tests/segment_restatement.py's random cases), against tests/proba_restatement.py:
  * the probabilities are within proba_bound(C) of the float64 softmax of the fp32 logits RCV_OP_CLS_FWD (RCV_OP_NHWC_TO_NCHW for the
    logits form) writes on the same operands;
  * the class map equals RCV_OP_CLS_LABEL's, bit for bit; the confidence is the stored probability of the stored class, bit for bit;
  * the pseudo-label is an exact function of the stored confidence and class at tau in {0, 0.9, 1};
  * each output alone gives the bytes it has with all outputs together (the class bytes at an odd address), nothing else is
    written, and two runs are bitwise equal.
And ``2 * proba - 1`` against the soft prior RCV_OP_LP_INPUT forms from the same logits (the two files state one arithmetic)."""
import numpy as np
import pytest
import torch

import proba_restatement as P
import segment_restatement as S
import small_ops_cases as K
from robocupvision_amd import _lib as L
from robocupvision_amd import model as M
from robocupvision_amd.engine import CLS3_PAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = (3, 5, 7)          # 105 pixels: no multiple of 4, 64 or 256
TAUS = (0.0, 0.9, 1.0)
SENTINEL = 7777


def _h():
    return L.handle(0)


def _cus():
    return int(L.load().rcv_num_cus(_h()))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(*ops):
    L.OpList(list(ops)).run(_h(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()


def _big():
    """The odd plane beyond one grid pass of 256-pixel workgroups at 4 per CU (cls_proba.hip keeps cls_label.hip's grid rule:
    min(ceil(pixels / per_wg), 4 * CUs) workgroups of 256 or, four lanes per pixel, 64 pixels)."""
    shape = K.big_planes(_cus())["reducing"][1]
    pixels = shape[0] * shape[1] * shape[2]
    assert pixels > 256 * 4 * _cus() and pixels % 2 == 1
    return shape


class _Outputs:
    def __init__(self, shape, cout):
        N, H, W = shape
        self.prob = torch.full((N, cout, H, W), float("nan"), device=DEV)
        self.lab_store = torch.full((N * H * W + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        self.lab = self.lab_store[1:].view(N, H, W)          # the class bytes start at an odd address
        assert self.lab.data_ptr() % 2 == 1
        self.conf = torch.full((N, H, W), float("nan"), device=DEV)
        self.pseudo = torch.full((N, H, W), SENTINEL, dtype=torch.int64, device=DEV)

    def slots(self, which):
        ptrs = dict(p_x0=self.prob, p_out=self.lab, p_x1=self.conf, p_x2=self.pseudo)
        return {k: v.data_ptr() for k, v in ptrs.items() if k in which}

    def untouched(self, which):
        ok = True
        if "p_x0" not in which:
            ok &= bool(torch.isnan(self.prob).all())
        if "p_out" not in which:
            ok &= bool((self.lab_store == 0xAB).all())
        if "p_x1" not in which:
            ok &= bool(torch.isnan(self.conf).all())
        if "p_x2" not in which:
            ok &= bool((self.pseudo == SENTINEL).all())
        return ok and int(self.lab_store[0]) == 0xAB


ALL = ("p_x0", "p_out", "p_x1", "p_x2")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_record(d, shape, cin, cout, fused, form, bias, alone=True):
    N, H, W = shape
    flags = L.F_FUSED_UP if fused else 0
    keep = {k: _dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    src = dict(n=N, h=H, w=W, cin=cin, cout=cout, p_in=keep["t"].data_ptr(), p_bias=keep["bias"].data_ptr() if bias else 0)
    if form == 0:
        src["p_w"] = keep["w"].data_ptr()
    if fused:
        src.update(aux0=d["mode2"], aux1=d["r"].shape[1], p_in_c=keep["tc"].data_ptr(), p_x3=keep["r"].data_ptr(), p_x4=keep["rc"].data_ptr())
    what = "%s cin %d cout %d fused %d form %d bias %d" % (shape, cin, cout, fused, form, bias)
    # the references on the same operands: RCV_OP_CLS_LABEL's class map and the logits the logits-writing record stores
    lab_ref = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    logits = torch.full((N, cout, H, W), float("nan"), device=DEV)
    _run(L.make_op(L.OP_CLS_LABEL, flags, inmode=form, p_out=lab_ref.data_ptr(), **src),
         L.make_op(L.OP_CLS_FWD, flags, p_out=logits.data_ptr(), **src) if form == 0 else
         L.make_op(L.OP_NHWC_TO_NCHW, 0, p_out=logits.data_ptr(), **src))
    want_p, want_cls = P.proba(logits.cpu().numpy())
    assert np.array_equal(want_cls, lab_ref.cpu().numpy()), what          # (the restatement's rule is the label kernel's)
    # all outputs together, tau = 0.9
    o = _Outputs(shape, cout)
    _run(L.make_op(L.OP_CLS_PROBA, flags, inmode=form, f0=0.9, **src, **o.slots(ALL)))
    prob, lab, conf, pseudo = o.prob.cpu().numpy(), o.lab.cpu().numpy(), o.conf.cpu().numpy(), o.pseudo.cpu().numpy()
    err = float(np.abs(prob.astype(np.float64) - want_p).max())
    print("%s: max |p - float64| = %.2f u (bound %.0f u), %d of %d pixels pass 0.9" % (what, err / P.U, P.proba_bound(cout) / P.U,
                                                                                    int((pseudo >= 0).sum()), pseudo.size))
    assert not np.isnan(prob).any() and err <= P.proba_bound(cout), what
    assert int(o.lab_store[0]) == 0xAB and torch.equal(o.lab, lab_ref), what
    assert np.array_equal(conf.view(np.uint32), P.confidence(prob, lab).view(np.uint32)), what
    assert np.array_equal(pseudo, P.pseudo_labels(conf, lab, 0.9)), what
    if cout == 1:
        assert bool((prob == 1.0).all())
    # a second run: bitwise the same
    o2 = _Outputs(shape, cout)
    _run(L.make_op(L.OP_CLS_PROBA, flags, inmode=form, f0=0.9, **src, **o2.slots(ALL)))
    for a, b in ((o.prob, o2.prob), (o.lab_store, o2.lab_store), (o.conf, o2.conf), (o.pseudo, o2.pseudo)):
        assert torch.equal(_bits(a), _bits(b)), what
    if not alone:
        return
    # each output alone: the same bytes, nothing else written; the pseudo-label at every threshold
    for slot, got in (("p_x0", "prob"), ("p_out", "lab_store"), ("p_x1", "conf")):
        o1 = _Outputs(shape, cout)
        _run(L.make_op(L.OP_CLS_PROBA, flags, inmode=form, f0=0.9, **src, **o1.slots((slot,))))
        assert torch.equal(_bits(getattr(o1, got)), _bits(getattr(o, got))) and o1.untouched((slot,)), "%s, %s alone" % (what, slot)
    for tau in TAUS:
        o1 = _Outputs(shape, cout)
        _run(L.make_op(L.OP_CLS_PROBA, flags, inmode=form, f0=tau, **src, **o1.slots(("p_x2",))))
        assert o1.untouched(("p_x2",)), what
        got = o1.pseudo.cpu().numpy()
        assert np.array_equal(got, P.pseudo_labels(conf, lab, tau)), "%s, tau %g" % (what, tau)
        if tau == 0.0:
            assert np.array_equal(got, lab.astype(np.int64))


CONFIGS = [("c8", 8, False, S.PLAIN, None), ("c8_up_affine_relu", 8, True, S.AFFINE_RELU, 8), ("c8_up_skip4", 8, True, S.AFFINE, 4),
           ("c16", 16, False, S.PLAIN, None), ("c16_up_skip8", 16, True, S.AFFINE_RELU, 8), ("c16_up_plain16", 16, True, S.PLAIN, 16)]


@pytest.mark.parametrize("tag,cin,fused,mode2,rch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_record_from_features(tag, cin, fused, mode2, rch):
    rng = np.random.default_rng(6700 + cin + 3 * fused)
    for cout in (1, 2, 5, 8):
        for bias in (True, False):
            d = S.random_case(rng, SMALL, cin, cout, fused, mode2, rch)
            _check_record(d, SMALL, cin, cout, fused, 0, bias)
    big = _big()
    _check_record(S.random_case(rng, big, cin, 5, fused, mode2, rch), big, cin, 5, fused, 0, True, alone=False)


def test_record_from_padded_logits():
    rng = np.random.default_rng(6800)

    def case(shape, cout):
        n = shape[0] * shape[1] * shape[2]
        return dict(t=(2.0 * rng.standard_normal((n, CLS3_PAD))).astype(np.float32), bias=(0.1 * rng.standard_normal(cout)).astype(np.float32))

    for cout in (1, 2, 5, 8):
        for bias in (True, False):
            _check_record(case(SMALL, cout), SMALL, CLS3_PAD, cout, False, 1, bias)
    big = _big()
    _check_record(case(big, 5), big, CLS3_PAD, 5, False, 1, True, alone=False)


def test_both_sides_of_the_threshold_and_wide_logits():
    """Logits spread over +-60 and logits of 1e4 + small (lp_input_restatement's cases, 5 classes in 8 floats per pixel): the maximum
    is subtracted before expf; and at 0.9 pixels fall on both sides."""
    rng = np.random.default_rng(6900)
    n = SMALL[0] * SMALL[1] * SMALL[2]
    seen = set()
    for name, z in (("ordinary", 3.0 * rng.standard_normal((n, 8))), ("spread60", rng.uniform(-60.0, 60.0, (n, 8))),
                    ("offset1e4", 1e4 + rng.standard_normal((n, 8))), ("equal", np.repeat(rng.standard_normal((n, 1)), 8, axis=1))):
        t = _dev(z.astype(np.float32))
        o = _Outputs(SMALL, 5)
        _run(L.make_op(L.OP_CLS_PROBA, 0, n=SMALL[0], h=SMALL[1], w=SMALL[2], cin=8, cout=5, inmode=1, f0=0.9, p_in=t.data_ptr(), **o.slots(ALL)))
        want = P.softmax(z.astype(np.float32)[:, :5]).reshape(SMALL + (5,)).transpose(0, 3, 1, 2)
        assert float(np.abs(o.prob.cpu().numpy().astype(np.float64) - want).max()) <= P.proba_bound(5), name
        pseudo = o.pseudo.cpu().numpy()
        seen |= {bool(v) for v in (pseudo >= 0).reshape(-1)}
        if name == "equal":
            assert bool((o.lab == 0).all()) and bool((o.prob == 0.2).all()) and bool((pseudo == P.IGNORE).all())
    assert seen == {True, False}


def test_refusals():
    x = torch.zeros(105, 8, device=DEV)
    w = torch.zeros(5, 8, device=DEV)
    out = torch.zeros(3, 5, 5, 7, device=DEV)
    base = dict(n=3, h=5, w=7, cin=8, cout=5, p_in=x.data_ptr(), p_w=w.data_ptr())
    for kw, word in ((dict(inmode=0), "no output"), (dict(inmode=2, p_x0=out.data_ptr()), "source form"),
                     (dict(inmode=0, cout=9, p_x0=out.data_ptr()), "classes"), (dict(inmode=0, cin=12, p_x0=out.data_ptr()), "input channels"),
                     (dict(inmode=1, cin=6, p_x0=out.data_ptr()), "floats per pixel")):
        with pytest.raises(L.RcvError, match=word):
            _run(L.make_op(L.OP_CLS_PROBA, 0, **{**base, **kw}))
    with pytest.raises(L.RcvError, match="RCV_F_FUSED_UP"):
        _run(L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, **{**base, "inmode": 1, "p_x0": out.data_ptr()}))


def test_c_entry_point():
    rng = np.random.default_rng(6950)
    d = S.random_case(rng, SMALL, 8, 5, False)
    x, w, b = _dev(d["t"]), _dev(d["w"]), _dev(d["bias"])
    o, o2 = _Outputs(SMALL, 5), _Outputs(SMALL, 5)
    L.check(L.load().rcv_cls_proba(_h(), x.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 5, 7, 8, 5, o.prob.data_ptr(), o.lab.data_ptr(),
                                   o.conf.data_ptr(), o.pseudo.data_ptr(), 0.9, torch.cuda.current_stream(DEV).cuda_stream), "rcv_cls_proba")
    _run(L.make_op(L.OP_CLS_PROBA, 0, n=3, h=5, w=7, cin=8, cout=5, inmode=0, f0=0.9, p_in=x.data_ptr(), p_w=w.data_ptr(), p_bias=b.data_ptr(),
                   **o2.slots(ALL)))
    for a, c in ((o.prob, o2.prob), (o.lab_store, o2.lab_store), (o.conf, o2.conf), (o.pseudo, o2.pseudo)):
        assert torch.equal(_bits(a), _bits(c))


def test_proba_is_the_soft_prior_of_lp_input():
    """C = 5: 2 * proba - 1 equals, bit for bit, the soft-prior channels RCV_OP_LP_INPUT forms from model(x): one arithmetic, stated in
    two files (2 * q is exact and the subtraction rounds once, contracted or not)."""
    torch.manual_seed(31)
    net = M.ROBO_UNet().to(DEV).eval()
    x = torch.randn(2, 3, 40, 56, device=DEV)
    with torch.no_grad():
        z = net(x)
        p = net.proba(x)
        inputs = M.labelprop_next(x, x, z)
    prior = inputs[:, 3:8].contiguous()
    assert torch.equal(_bits(2.0 * p - 1.0), _bits(prior))
