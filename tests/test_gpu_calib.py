"""GPU: the calibration tail (RCV_OP_CLS_CALIB, csrc/cls_calib.hip) at record level through rcv_run, against the numpy restatement
(tests/calib_restatement.py); every figure is an integer, so every comparison is exact.
  * form 2 on hand-made maps (edge values and one ulp below, 0, 1, NaN, class bytes >= C, targets -100, C, 2^32 + c), on the small
    plane and on the odd plane beyond one grid pass: state, guard words, accumulation, reproducibility, no targets, one target moved;
  * forms 0 and 1 on segment_restatement's random operands: the state equals the restatement of what RCV_OP_CLS_PROBA stores on the
    same operands (class map and confidence), with edges chosen among those stored confidences;
  * for every edge the labelled pixels RCV_OP_CLS_PROBA's gate keeps at f[0] = edge are the report's ``kept``;
  * ``model.calibrate`` / ``Trainer.calibrate`` on the networks against the restatement of their own ``proba`` maps.

Edges and bins: every edge is a stored confidence where enough distinct ones exist, so a pixel sits exactly on every such edge.  At
least min(3, K + 1) bins are non-empty (K = 1 has two bins).  One class is the exception the arithmetic forces: its softmax is 1.0 at
every pixel, so all pixels share one bin -- there the test asserts that they sit exactly on the edge 1.0."""
import numpy as np
import pytest
import torch

import calib_restatement as R
import segment_restatement as S
import small_ops_cases as K
from robocupvision_amd import _lib as L
from robocupvision_amd import export as E
from robocupvision_amd import metrics as MT
from robocupvision_amd import model as M
from robocupvision_amd.engine import CLS3_PAD
from robocupvision_amd.optim import SGD
from robocupvision_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = (3, 5, 7)          # 105 pixels: no multiple of 4, 64 or 256
GUARD = 16
SENTINEL = -0x5A5A5A5A5A5A5A5B


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
    """The odd plane beyond one grid pass of 256-pixel workgroups at 4 per CU (cls_calib.hip keeps cls_proba.hip's grid rule)."""
    shape = K.big_planes(_cus())["reducing"][1]
    pixels = shape[0] * shape[1] * shape[2]
    assert pixels > 256 * 4 * _cus() and pixels % 2 == 1
    return shape


class _State:
    """int64 [K + 1][C][C + 3], zero, between guard words."""

    def __init__(self, k, c):
        self.n = (k + 1) * c * (c + 3)
        self.store = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        self.view = self.store[GUARD:GUARD + self.n]
        self.view.zero_()
        self.shape = (k + 1, c, c + 3)

    def ptr(self):
        return self.view.data_ptr()

    def table(self):
        s = self.store.cpu().numpy()
        assert (s[:GUARD] == SENTINEL).all() and (s[GUARD + self.n:] == SENTINEL).all(), "guard words written"
        return s[GUARD:GUARD + self.n].reshape(self.shape).copy()


def _maps_op(shape, c, edges, cls, conf, t, state):
    return L.make_op(L.OP_CLS_CALIB, 0, n=shape[0], h=shape[1], w=shape[2], cin=1, cout=c, inmode=2, count=edges.numel(), p_in=cls.data_ptr(),
                     p_x1=conf.data_ptr(), p_in2=t.data_ptr() if t is not None else 0, p_x0=edges.data_ptr(), p_x2=state.ptr())


@pytest.mark.parametrize("plane", ["small", "big"])
def test_maps_form_on_handmade_maps(plane):
    C = 5
    shape = SMALL if plane == "small" else _big()
    cls_h, conf_h, t_h = R.handmade_maps(shape, C)
    n = cls_h.size
    second = 256 * 4 * _cus()          # the first pixel of the second grid pass
    if plane == "big":
        assert second < n
        cls_h.reshape(-1)[second], conf_h.reshape(-1)[second], t_h.reshape(-1)[second] = 2, np.float32(0.625), 3
    want = R.table(cls_h, conf_h, t_h, R.HAND_EDGES, C)
    assert want[:, :, :C + 1].sum() == int(((cls_h < C) & ~np.isnan(conf_h)).sum()) < n
    cls, conf, t, edges = _dev(cls_h), _dev(conf_h), _dev(t_h), _dev(R.HAND_EDGES)
    s = _State(edges.numel(), C)
    _run(_maps_op(shape, C, edges, cls, conf, t, s))
    got = s.table()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # a second launch accumulates; a fresh run is bitwise the first
    _run(_maps_op(shape, C, edges, cls, conf, t, s))
    assert np.array_equal(s.table(), 2 * want)
    s2 = _State(edges.numel(), C)
    _run(_maps_op(shape, C, edges, cls, conf, t, s2))
    assert np.array_equal(s2.table(), got)
    # without targets every count sits in column C and every sum in column C + 2
    s3 = _State(edges.numel(), C)
    _run(_maps_op(shape, C, edges, cls, conf, None, s3))
    none = s3.table()
    assert np.array_equal(none, R.table(cls_h, conf_h, None, R.HAND_EDGES, C))
    assert not none[:, :, :C].any() and not none[:, :, C + 1].any() and none[:, :, C].sum() == want[:, :, :C + 1].sum()
    assert np.array_equal(none[:, :, C + 2], want[:, :, C + 1] + want[:, :, C + 2])
    if plane == "big":
        # one target of the second grid pass becomes -100: one count and its q move, nothing else does
        t_h.reshape(-1)[second] = -100
        s4 = _State(edges.numel(), C)
        _run(_maps_op(shape, C, edges, cls, conf, _dev(t_h), s4))
        diff = s4.table() - want
        b = int(R.bin_index(np.float32(0.625), R.HAND_EDGES)[0])
        q = int(R.fixed_point(np.float32(0.625))[0])
        expect = np.zeros_like(diff)
        expect[b, 2, 3], expect[b, 2, C], expect[b, 2, C + 1], expect[b, 2, C + 2] = -1, 1, -q, q
        assert b == 3 and q == 5 * 2 ** 23 and np.array_equal(diff, expect)


def choose_edges(conf, k):
    """k strictly ascending fp32 edges, stored confidences wherever enough distinct ones exist (evenly spaced ranks), else filled up
    from a grid in [0, 1)."""
    u = np.unique(conf[~np.isnan(conf)])
    idx = np.unique(np.round(np.linspace(0, u.size - 1, k + 2)[1:-1]).astype(int)) if u.size > 1 else np.array([0])
    chosen = list(u[idx][:k])
    for v in np.linspace(0.0, 1.0, 4 * k + 1, endpoint=False).astype(np.float32):
        if len(chosen) >= k:
            break
        if v not in chosen:
            chosen.append(v)
    e = np.sort(np.array(chosen, np.float32))
    assert e.size == k and (np.diff(e) > 0).all() if k > 1 else e.size == 1
    return e


def _source(d, shape, cin, cout, fused, form, bias):
    N, H, W = shape
    keep = {k: _dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    src = dict(n=N, h=H, w=W, cin=cin, cout=cout, inmode=form, p_in=keep["t"].data_ptr(), p_bias=keep["bias"].data_ptr() if bias else 0)
    if form == 0:
        src["p_w"] = keep["w"].data_ptr()
    if fused:
        src.update(aux0=d["mode2"], aux1=d["r"].shape[1], p_in_c=keep["tc"].data_ptr(), p_x3=keep["r"].data_ptr(), p_x4=keep["rc"].data_ptr())
    return src, keep


def _targets(shape, C, seed):
    """int64 labels with -100, C and 2^32 + c among them."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, C, shape).astype(np.int64)
    t.reshape(-1)[::41] = -100
    t.reshape(-1)[5::53] = C
    t.reshape(-1)[7::59] = 2 ** 32 + (C - 1)
    return t


def _check_record(d, shape, cin, cout, fused, form, bias, ks):
    flags = L.F_FUSED_UP if fused else 0
    src, keep = _source(d, shape, cin, cout, fused, form, bias)
    what = "%s cin %d cout %d fused %d form %d bias %d" % (shape, cin, cout, fused, form, bias)
    lab = torch.full(shape, 0xAB, dtype=torch.uint8, device=DEV)
    conf = torch.full(shape, float("nan"), device=DEV)
    _run(L.make_op(L.OP_CLS_PROBA, flags, p_out=lab.data_ptr(), p_x1=conf.data_ptr(), **src))
    lab_h, conf_h = lab.cpu().numpy(), conf.cpu().numpy()
    assert not np.isnan(conf_h).any() and int(lab_h.max()) < cout, what
    t_h = _targets(shape, cout, 68 + cout)
    t = _dev(t_h)
    for k in ks:
        edges_h = choose_edges(conf_h.reshape(-1), k)
        bins = R.bin_index(conf_h, edges_h)
        on_edge = int(np.isin(conf_h.reshape(-1), edges_h).sum())
        filled = np.unique(bins).size
        print("%s K %d: %d bins filled, %d pixels on an edge" % (what, k, filled, on_edge))
        assert on_edge >= 1, what
        if cout > 1:
            assert filled >= min(3, k + 1), what
        else:          # one class: softmax is 1.0 everywhere, one bin, every pixel on the edge 1.0
            assert (conf_h == 1.0).all() and on_edge == conf_h.size and edges_h[-1] == 1.0, what
        edges = _dev(edges_h)
        s = _State(k, cout)
        _run(L.make_op(L.OP_CLS_CALIB, flags, count=k, p_in2=t.data_ptr(), p_x0=edges.data_ptr(), p_x2=s.ptr(), **src))
        got, want = s.table(), R.table(lab_h, conf_h, t_h, edges_h, cout)
        assert np.array_equal(got, want), (what, k, np.argwhere(got != want)[:8])
        assert got[:, :, :cout + 1].sum() == conf_h.size


CONFIGS = [("c8", 8, False, S.PLAIN, None), ("c8_up_affine_relu", 8, True, S.AFFINE_RELU, 8), ("c8_up_skip4", 8, True, S.AFFINE, 4),
           ("c16", 16, False, S.PLAIN, None), ("c16_up_skip8", 16, True, S.AFFINE_RELU, 8), ("c16_up_plain16", 16, True, S.PLAIN, 16)]
KS = (1, 7, 32)


@pytest.mark.parametrize("tag,cin,fused,mode2,rch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_record_from_features(tag, cin, fused, mode2, rch):
    rng = np.random.default_rng(6800 + cin + 3 * fused)
    for cout in (1, 2, 5, 8):
        for bias in (True, False):
            _check_record(S.random_case(rng, SMALL, cin, cout, fused, mode2, rch), SMALL, cin, cout, fused, 0, bias, KS)


@pytest.mark.parametrize("tag,cin,fused,mode2,rch", [CONFIGS[1], CONFIGS[3]], ids=[CONFIGS[1][0], CONFIGS[3][0]])
def test_record_from_features_beyond_one_grid_pass(tag, cin, fused, mode2, rch):
    """(with four lanes per pixel a workgroup sweeps 64 pixels: the 16-channel form passes its cap four times sooner)"""
    big = _big()
    _check_record(S.random_case(np.random.default_rng(6810 + cin), big, cin, 5, fused, mode2, rch), big, cin, 5, fused, 0, True, (16,))


def _logit_case(rng, shape, cout):
    n = shape[0] * shape[1] * shape[2]
    return dict(t=(2.0 * rng.standard_normal((n, CLS3_PAD))).astype(np.float32), bias=(0.1 * rng.standard_normal(cout)).astype(np.float32))


def test_record_from_padded_logits():
    rng = np.random.default_rng(6820)
    for cout in (1, 2, 5, 8):
        for bias in (True, False):
            _check_record(_logit_case(rng, SMALL, cout), SMALL, CLS3_PAD, cout, False, 1, bias, KS)
    big = _big()
    _check_record(_logit_case(rng, big, 5), big, CLS3_PAD, 5, False, 1, True, (16,))


def test_kept_is_what_the_pseudo_label_gate_keeps():
    """For every edge: per class, the labelled pixels with pseudo-label >= 0 at f[0] = edge are the report's ``kept``."""
    rng = np.random.default_rng(6830)
    shape, cin, cout, k = SMALL, 8, 5, 7
    d = S.random_case(rng, shape, cin, cout, True, S.AFFINE_RELU, 8)
    src, keep = _source(d, shape, cin, cout, True, 0, True)
    conf = torch.full(shape, float("nan"), device=DEV)
    _run(L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, p_x1=conf.data_ptr(), **src))
    edges_h = choose_edges(conf.cpu().numpy().reshape(-1), k)
    t_h = _targets(shape, cout, 70)
    t, edges = _dev(t_h), _dev(edges_h)
    s = _State(k, cout)
    _run(L.make_op(L.OP_CLS_CALIB, L.F_FUSED_UP, count=k, p_in2=t.data_ptr(), p_x0=edges.data_ptr(), p_x2=s.ptr(), **src))
    rep = MT.calibration_report(s.table().tolist(), edges_h.tolist(), cout)
    labelled = (t_h >= 0) & (t_h < cout)
    for j, e in enumerate(edges_h):
        pseudo = torch.full(shape, 7777, dtype=torch.int64, device=DEV)
        _run(L.make_op(L.OP_CLS_PROBA, L.F_FUSED_UP, f0=float(e), p_x2=pseudo.data_ptr(), **src))
        p = pseudo.cpu().numpy()
        assert rep["kept"][j] == [int(((p == c) & labelled).sum()) for c in range(cout)], (j, float(e))
        assert rep["kept_unlabelled"][j] == [int(((p == c) & ~labelled).sum()) for c in range(cout)]
    assert rep["kept"][0] != rep["kept"][-1]


def test_launch_refusals_and_c_entry_point():
    rng = np.random.default_rng(6840)
    d = S.random_case(rng, SMALL, 8, 5, False)
    x, w, b, edges = _dev(d["t"]), _dev(d["w"]), _dev(d["bias"]), _dev(np.array([0.5, 0.9], np.float32))
    lab = torch.zeros(SMALL, dtype=torch.uint8, device=DEV)
    s = _State(2, 5)
    base = dict(n=3, h=5, w=7, cin=8, cout=5, inmode=0, count=2, p_in=x.data_ptr(), p_w=w.data_ptr(), p_x0=edges.data_ptr(), p_x2=s.ptr())
    for kw, word in ((dict(p_in=0), "null input"), (dict(p_x0=0), "null edges"), (dict(p_x2=0), "null state"), (dict(p_w=0), "null classifier"),
                     (dict(inmode=2, p_in=lab.data_ptr()), "null confidence map"), (dict(count=33), "edges")):
        with pytest.raises(L.RcvError, match=word):
            _run(L.make_op(L.OP_CLS_CALIB, 0, **{**base, **kw}))
    assert not s.table().any()
    t = _dev(_targets(SMALL, 5, 71))
    L.check(L.load().rcv_cls_calib(_h(), x.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 5, 7, 8, 5, t.data_ptr(), edges.data_ptr(), 2, s.ptr(),
                                   torch.cuda.current_stream(DEV).cuda_stream), "rcv_cls_calib")
    s2 = _State(2, 5)
    _run(L.make_op(L.OP_CLS_CALIB, 0, **{**base, "p_bias": b.data_ptr(), "p_in2": t.data_ptr(), "p_x2": s2.ptr()}))
    assert np.array_equal(s.table(), s2.table()) and s2.table()[:, :, :6].sum() == 105


def _build(make, seed=5):
    torch.manual_seed(seed)
    net = make()
    for m in net.modules():          # running statistics an inference pass would meet, not the initial (0, 1)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net.to(DEV).eval()


def _restate(net, x, t, edges_h):
    _, lab, conf = net.proba(x, labels=True, confidence=True)
    return R.table(lab.cpu().numpy(), conf.cpu().numpy(), None if t is None else t.cpu().numpy(), edges_h, 5)


NETS = [("robo", lambda: M.ROBO_UNet(), (2, 3, 48, 64)), ("pb_fcn_k5", lambda: M.PB_FCN(32, 5, 5, False, 0), (2, 3, 48, 64)),
        ("labelprop", lambda: M.LabelProp(5, 32, 0), (2, 8, 48, 64))]
EDGES = (0.3, 0.5, 0.7, 0.9, 0.99)


@pytest.mark.parametrize("tag,make,shape", NETS, ids=[n[0] for n in NETS])
def test_network_calibrate_equals_the_restatement_of_proba(tag, make, shape):
    net = _build(make)
    torch.manual_seed(33)
    batches = [(torch.randn(*shape, device=DEV), _dev(_targets((shape[0],) + shape[2:], 5, 80 + k))) for k in range(2)]
    state = MT.CalibrationState(5, EDGES, DEV)
    edges_h = np.array(state.edges, np.float32)
    assert net.calibrate(batches[0][0], state, batches[0][1]) is None
    want0 = _restate(net, *batches[0], edges_h)
    assert np.array_equal(state.buf.cpu().numpy(), want0) and want0[:, :, :6].sum() == shape[0] * 48 * 64
    print("%s: bins %s" % (tag, want0[:, :, :6].sum((1, 2)).tolist()))
    # frames without labels
    state.reset()
    net.calibrate(batches[1][0], state)
    assert np.array_equal(state.buf.cpu().numpy(), _restate(net, batches[1][0], None, edges_h))
    # Trainer.calibrate over both batches: the sum; a bare tensor is a batch without labels
    tr = Trainer(net, class_weights=(1, 10, 30, 10, 2), optimizer=None if isinstance(net, M.ROBO_UNet) else SGD(net, lr=1e-2, momentum=0.5,
                                                                                                                  weight_decay=1e-3))
    fresh = MT.CalibrationState(5, EDGES, DEV)
    rep = tr.calibrate(batches, fresh)
    want = want0 + _restate(net, *batches[1], edges_h)
    assert np.array_equal(fresh.buf.cpu().numpy(), want)
    ref = R.report(want, edges_h)
    assert rep["all"]["kept"] == ref["all_kept"].tolist() and np.array_equal(rep["kept_confusion"].numpy(), ref["kept_confusion"])
    assert abs(rep["ece"] - ref["ece"]) <= 8 * 2.0 ** -53 and rep["labelled"] + rep["unlabelled"] == 2 * shape[0] * 48 * 64
    rep2 = tr.calibrate([batches[0][0], (batches[1][0],)], edges=(0.5,))
    assert rep2["edges"] == [0.5] and rep2["labelled"] == 0 and rep2["unlabelled"] == 2 * shape[0] * 48 * 64
    assert sum(1 for (_, k) in net._get_engine().plans if k == frozenset()) == 1          # one eval-calib plan, in the one cache
    with pytest.raises(L.RcvError, match="classes"):
        net.calibrate(batches[0][0], MT.CalibrationState(3, EDGES, DEV))
    with pytest.raises(L.RcvError, match=r"call `\.eval\(\)` first"):
        net.train().calibrate(batches[0][0], state)


def test_exported_net_calibrates_as_its_module(tmp_path):
    m = _build(lambda: M.ROBO_UNet())
    E.save_export(str(tmp_path), m, img_shape=(48, 64))
    net = E.load_export(str(tmp_path / "net.cfg"), str(tmp_path / "weights.dat")).to(DEV)
    x = torch.randn(2, 3, 48, 64, generator=torch.Generator().manual_seed(12)).to(DEV)
    t = _dev(_targets((2, 48, 64), 5, 90))
    a, b = MT.CalibrationState(5, EDGES, DEV), MT.CalibrationState(5, EDGES, DEV)
    net.calibrate(x, a, t)
    m.calibrate(x, b, t)
    want = _restate(net, x, t, np.array(a.edges, np.float32))
    assert np.array_equal(a.buf.cpu().numpy(), want) and torch.equal(a.buf, b.buf)
    rep = a.compute()
    assert rep["labelled"] + rep["unlabelled"] == 2 * 48 * 64 and rep["kept"][0] == R.report(want, a.edges)["kept"][0].tolist()


def test_classify_mode_and_state_maps():
    x = torch.zeros(1, 3, 48, 64, device=DEV)
    with pytest.raises(L.RcvError, match="classify mode"):
        M.PB_FCN_2(True).to(DEV).eval().calibrate(x, MT.CalibrationState(5, EDGES, DEV))
    # CalibrationState.update_from_maps is the maps form
    cls_h, conf_h, t_h = R.handmade_maps(SMALL, 5)
    st = MT.CalibrationState(5, R.HAND_EDGES.tolist(), DEV)
    st.update_from_maps(_dev(cls_h), _dev(conf_h), _dev(t_h))
    st.update_from_maps(_dev(cls_h), _dev(conf_h))
    want = R.table(cls_h, conf_h, t_h, R.HAND_EDGES, 5) + R.table(cls_h, conf_h, None, R.HAND_EDGES, 5)
    assert np.array_equal(st.buf.cpu().numpy(), want)
    rep, ref = st.compute(), R.report(want, R.HAND_EDGES)
    assert rep["kept"] == ref["kept"].tolist() and rep["all"]["correct"] == ref["all_correct"].tolist()
    st.reset()
    assert not bool(st.buf.any())
