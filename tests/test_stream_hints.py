"""CPU: the streaming-hint policy (csrc/stream_hint.h, rcv_internal.h rcv_stream_hints) through the query path of the planning-only
handle: rcv_op_stream_hints answers RCV_F_STREAM_OUT / RCV_F_STREAM_PW exactly for the records whose tensor reaches the handle's
threshold (default 128 MiB; RCV_STREAM_MIN_MB, handed over once per handle by _lib), 0 MiB clears every hint, the record flags force one
whatever the size, and of the headline step (ROBO-UNet 640 x 480, batch 32) the 314 MB and 157 MB tensors are marked and nothing of the
128-channel belly."""
import ctypes as C

import pytest

from robocupvision_amd import _lib as L

MIB = 1 << 20


@pytest.fixture
def planner():
    """A planning-only handle of this test's own (the shared one of _lib keeps its threshold)."""
    lib = L.load()
    made = []

    def make(mb=None):
        out = C.c_void_p()
        L.check(lib.rcv_create_planner(256, C.byref(out)), "rcv_create_planner")
        made.append(out)
        if mb is not None:
            L.check(lib.rcv_set_stream_min_mb(out, mb), "rcv_set_stream_min_mb")
        return out
    yield make
    for h in made:
        lib.rcv_destroy(h)


def _conv(n, h, w, cin, cout, s=1, flags=0, mode=None, handle=None):
    op = L.make_op(L.OP_CONV, L.F_BIAS | flags, n=n, h=h, w=w, cin=cin, cout=cout, ho=(h - 1) // s + 1, wo=(w - 1) // s + 1, stride=s, dil=1,
                   inmode=(L.LOAD_NCHW if cin <= 4 else L.LOAD_AFFINE) if mode is None else mode, stats=L.STATS_FWD)
    if handle is not None:
        op.i[L.RCV_I_AUX0] = L.op_filter_layout(handle, op)
    return op


def _tconv(n, h, w, cin, cout, flags=0):
    return L.make_op(L.OP_TCONV, L.F_BIAS | flags, n=n, h=h, w=w, cin=cin, cout=cout, ho=2 * h, wo=2 * w, stride=2, dil=1,
                     inmode=L.LOAD_AFFINE, aux0=1 if cout <= 32 else 0, stats=L.STATS_FWD)


def _wgrad(n, h, w, cin, cout, s=1, flags=0):
    return L.make_op(L.OP_WGRAD, flags, n=n, h=h, w=w, cin=cin, cout=cout, ho=(h - 1) // s + 1, wo=(w - 1) // s + 1, stride=s, dil=1,
                     inmode=L.LOAD_NCHW if cin <= 4 else L.LOAD_AFFINE, inmode2=L.LOAD_GRAD_ENC)


def _combine(n, h, w, c, flags=0):
    return L.make_op(L.OP_COMBINE, flags, n=n, h=h, w=w, cout=c, inmode2=L.LOAD_AFFINE)


def test_flag_follows_the_tensor_size_exactly(planner):
    """One byte under the threshold: no hint; at the threshold: the hint.  The tensor that counts is the record's output (conv,
    transposed conv, combine) or its pointwise operand (filter gradient, combine)."""
    h = planner()
    # N * 64 * 128 * 8 channels * 4 bytes = N * 256 KiB: N = 512 is 128 MiB exactly
    for n, want in ((511, 0), (512, L.F_STREAM_OUT), (700, L.F_STREAM_OUT)):
        assert L.op_stream_hints(h, _conv(n, 64, 128, 8, 8)) == want, n
        assert L.op_stream_hints(h, _tconv(n, 32, 64, 16, 8)) == want, n          # the OUTPUT plane is 64 x 128
        assert L.op_stream_hints(h, _conv(n, 128, 256, 8, 8, s=2)) == want, n     # stride 2: again the output plane
        assert L.op_stream_hints(h, _combine(n, 64, 128, 8)) == (L.F_STREAM_OUT | L.F_STREAM_PW if want else 0), n
        assert L.op_stream_hints(h, _wgrad(n, 64, 128, 8, 8)) == (L.F_STREAM_PW if want else 0), n
    # concat writes twice the channels: its output reaches the threshold before its inputs do
    assert L.op_stream_hints(h, _combine(256, 64, 128, 8, L.F_CONCAT)) == L.F_STREAM_OUT
    assert L.op_stream_hints(h, _combine(255, 64, 128, 8, L.F_CONCAT)) == 0
    # another threshold, fractional: 0.25 MiB = one image of the shape above
    h2 = planner(0.25)
    assert L.op_stream_hints(h2, _conv(1, 64, 128, 8, 8)) == L.F_STREAM_OUT
    assert L.op_stream_hints(h2, _conv(1, 64, 127, 8, 8)) == 0
    # kinds without hinted kernels answer 0 whatever their size
    assert L.op_stream_hints(h2, L.make_op(L.OP_MEMSET, 0, count=1 << 30)) == 0


def test_zero_switches_every_hint_off_and_flags_force_one(planner):
    off, on = planner(0.0), planner()
    big = dict(n=32, h=480, w=640)
    for op in (_conv(cin=8, cout=8, **big), _tconv(32, 240, 320, 16, 8), _wgrad(cin=8, cout=8, **big), _combine(32, 480, 640, 8)):
        assert L.op_stream_hints(on, op) != 0 and L.op_stream_hints(off, op) == 0, op.kind
    # forced: a tiny record carries the hint on either handle, and only the forced one
    for h in (off, on):
        assert L.op_stream_hints(h, _conv(2, 12, 20, 8, 8, flags=L.F_STREAM_OUT)) == L.F_STREAM_OUT
        assert L.op_stream_hints(h, _tconv(2, 8, 12, 16, 8, flags=L.F_STREAM_OUT)) == L.F_STREAM_OUT
        assert L.op_stream_hints(h, _wgrad(2, 12, 20, 8, 8, flags=L.F_STREAM_PW)) == L.F_STREAM_PW
        assert L.op_stream_hints(h, _combine(2, 12, 20, 8, L.F_STREAM_OUT)) == L.F_STREAM_OUT
        assert L.op_stream_hints(h, _combine(2, 12, 20, 8, L.F_STREAM_OUT | L.F_STREAM_PW)) == L.F_STREAM_OUT | L.F_STREAM_PW
        assert L.op_stream_hints(h, _conv(2, 12, 20, 8, 8)) == 0
    # the hints are no part of a plan: same label, same workspace with and without
    a, b = _conv(2, 37, 53, 16, 16), _conv(2, 37, 53, 16, 16, flags=L.F_STREAM_OUT)
    assert L.op_workspace(on, a) == L.op_workspace(on, b) and a.i[L.RCV_I_NPART] == b.i[L.RCV_I_NPART]
    assert L.OpList([a]).labels(on) == L.OpList([b]).labels(on)
    # a record the planner refuses is refused here too
    with pytest.raises(L.RcvError):
        L.op_stream_hints(on, _conv(2, 12, 20, 8, 6))


def test_environment_value_is_handed_over_once_per_handle(monkeypatch):
    """RCV_STREAM_MIN_MB is read by the binding when it creates a handle (the library reads no environment)."""
    lib = L.load()
    big = _conv(32, 480, 640, 8, 8)
    for ev, want in (("0", 0), ("512", 0), ("128", L.F_STREAM_OUT), (None, L.F_STREAM_OUT)):
        if ev is None:
            monkeypatch.delenv("RCV_STREAM_MIN_MB", raising=False)
        else:
            monkeypatch.setenv("RCV_STREAM_MIN_MB", ev)
        out = C.c_void_p()
        L.check(lib.rcv_create_planner(256, C.byref(out)), "rcv_create_planner")
        h = L._apply_stream_min(out)
        try:
            assert L.op_stream_hints(h, big) == want, ev
            monkeypatch.setenv("RCV_STREAM_MIN_MB", "0")          # a later change of the environment does not reach the handle
            assert L.op_stream_hints(h, big) == want, ev
        finally:
            lib.rcv_destroy(h)


def test_headline_plan_marks_the_large_tensors_only(planner):
    """The layer shapes of the headline step (bench.py robo_unet_640x480_bs32: 8 planes, depth 4, 128-channel belly at 30 x 40): the
    8-channel full-resolution tensors (314 MB) and the 16-channel half-resolution tensors (157 MB) are stream-once; the 32-channel
    quarter-resolution tensors (79 MB), everything below and the whole belly are not."""
    h = planner()
    N = 32
    levels = [(480, 640, 8), (240, 320, 16), (120, 160, 32), (60, 80, 64), (30, 40, 128)]
    marked, unmarked = set(), set()

    def note(op, what, nbytes, bit):
        got = L.op_stream_hints(h, op)
        assert got in (0, bit) or what.startswith("combine"), (what, got)
        assert bool(got & bit) == (nbytes >= 128 * MIB), (what, nbytes, got)
        (marked if got else unmarked).add((what, nbytes))

    note(_conv(N, 480, 640, 3, 8, handle=h), "first", N * 480 * 640 * 8 * 4, L.F_STREAM_OUT)
    note(_wgrad(N, 480, 640, 3, 8), "wgrad first", N * 480 * 640 * 8 * 4, L.F_STREAM_PW)
    for k, (H, W, Cc) in enumerate(levels):
        nbytes = N * H * W * Cc * 4
        note(_conv(N, H, W, Cc, Cc, handle=h), "conv %d" % Cc, nbytes, L.F_STREAM_OUT)
        note(_conv(N, H, W, Cc, Cc, mode=L.LOAD_GRAD_ENC, flags=L.F_RESID, handle=h), "dgrad %d" % Cc, nbytes, L.F_STREAM_OUT)
        note(_wgrad(N, H, W, Cc, Cc), "wgrad %d" % Cc, nbytes, L.F_STREAM_PW)
        if k + 1 < len(levels):
            H2, W2, C2 = levels[k + 1]
            note(_conv(N, H, W, Cc, C2, s=2, handle=h), "down %d" % C2, N * H2 * W2 * C2 * 4, L.F_STREAM_OUT)
            note(_wgrad(N, H, W, Cc, C2, s=2), "wgrad down %d" % C2, N * H2 * W2 * C2 * 4, L.F_STREAM_PW)
            note(_tconv(N, H2, W2, C2, Cc), "up %d" % Cc, nbytes, L.F_STREAM_OUT)
            note(_combine(N, H, W, Cc), "combine %d" % Cc, nbytes, L.F_STREAM_OUT)
    assert {b for _, b in marked} == {N * 480 * 640 * 8 * 4, N * 240 * 320 * 16 * 4}      # 314.6 MB and 157.3 MB
    assert max(b for _, b in unmarked) == N * 120 * 160 * 32 * 4
    assert not any("128" in what for what, _ in marked)
