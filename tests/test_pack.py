"""CPU: the numpy restatement of the filter packer (tests/pack_restatement.py) against the torch operations each packed filter stands
for, in float64 -- independently of the kernel.  Every combination of (rows_from_d1, flip, layout, scale) that engine.py emits, on wide,
narrow, ragged and image-layer channel pairs: unpack_apply(pack(...)) equals the operation to 1e-12 of its largest entry.  The device's
packer is then compared with pack() itself (tests/test_gpu_pack.py), and the records behind the flip and scale branches with float64
(tests/test_gpu_kernels.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pack_restatement as R      # noqa: E402

BAR = 1e-12


def cases():
    """(record, rows_from_d1, flip, layout, scaled, rows, cols, rows_pad): every combination on every channel pair; the classifier's
    data gradient with 1..8 class rows padded to 8."""
    for rec, rfd1, flip, layouts, scaled in R.COMBINATIONS:
        for layout in layouts:
            for sc in ((False, True) if scaled else (False,)):
                if rec == "cls_dgrad":
                    for n_class in range(1, 9):
                        for cols in (8, 16, 12, 40):
                            yield rec, rfd1, flip, layout, sc, n_class, cols, R.CLS_ROWS_PAD
                else:
                    for rows, cols in R.CHANNEL_PAIRS:
                        yield rec, rfd1, flip, layout, sc, rows, cols, None


def geometries(rec, layout):
    """(stride, dilation) a record of this kind runs the layout at."""
    if rec in ("tconv",):
        return [(2, 1)]
    if rec == "tconv_dgrad":
        return [(2, 1)]
    if rec in ("dgrad", "cls_dgrad"):
        return [(1, 1), (1, 2)] if layout == 0 and rec == "dgrad" else [(1, 1)]
    return {0: [(1, 1), (2, 1), (1, 2), (2, 2)], 2: [(1, 1)], 3: [(1, 1), (2, 1)], 5: [(2, 1)]}[layout]


def torch_reference(rec, x, w, s, d):
    """x NHWC float64, w the parameter tensor [D0][D1][3][3] float64 (already scaled); NHWC result of the torch operation."""
    xt, wt = torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w)
    if rec == "conv":
        y = F.conv2d(xt, wt, stride=s, padding=d, dilation=d)
    elif rec == "tconv":
        y = F.conv_transpose2d(xt, wt, stride=2, padding=1, output_padding=1)
    elif rec in ("dgrad", "cls_dgrad"):
        y = torch.nn.grad.conv2d_input((xt.shape[0], wt.shape[1], xt.shape[2], xt.shape[3]), wt, xt, stride=1, padding=d, dilation=d)
    else:       # the data gradient of conv_transpose2d(k3, s2, p1, op1), by autograd
        inp = torch.zeros(xt.shape[0], wt.shape[0], xt.shape[2] // 2, xt.shape[3] // 2, dtype=torch.float64, requires_grad=True)
        out = F.conv_transpose2d(inp, wt, stride=2, padding=1, output_padding=1)
        y, = torch.autograd.grad(out, inp, xt.contiguous())
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("rec,layout,scaled", sorted({(c[0], c[3], c[4]) for c in cases()}))
def test_packed_filter_applies_as_the_torch_operation(rec, layout, scaled):
    rng = np.random.default_rng(100 + 7 * layout + scaled)
    n = 0
    for c in cases():
        if (c[0], c[3], c[4]) != (rec, layout, scaled):
            continue
        _, rfd1, flip, _, _, rows, cols, rp_fixed = c
        D0, D1 = (cols, rows) if rfd1 else (rows, cols)
        rp, cp, nfl = R.pack_dims(rows, cols, layout)
        if rp_fixed:
            rp = rp_fixed
        w = rng.standard_normal((D0, D1, 3, 3)).astype(np.float32)
        scale = (rng.uniform(0.25, 4.0, cols) * rng.choice([-1.0, 1.0], cols)).astype(np.float32) if scaled else None
        P = R.pack(w, D0, D1, rfd1, flip, rp, cp, layout, scale=scale, dtype=np.float64)
        assert P.dtype == np.float64 and (P.size == 2 * nfl if layout in (3, 4, 5) else P.size == nfl or rp_fixed)
        w64 = w.astype(np.float64)
        if scaled:      # the scale belongs to the column (output) channel: D0 of a conv filter, D1 of a transposed one
            w64 = w64 * (scale.astype(np.float64)[:, None, None, None] if rfd1 else scale.astype(np.float64)[None, :, None, None])
        for s, d in geometries(rec, layout):
            H, W = (6, 8) if rec == "tconv_dgrad" else (5, 7)      # (odd planes: the ragged Winograd tile, the stride-2 edge)
            x = rng.standard_normal((2, H, W, rows))
            got = R.unpack_apply(P, x, rows, cols, rp, cp, layout, "tconv" if rec == "tconv" else "conv", stride=s, dilation=d)
            ref = torch_reference(rec, x, w64, s, d)
            assert got.shape == ref.shape, (c, got.shape, ref.shape)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= BAR, (c, s, d, err)
            n += 1
    assert n > 0


def test_float32_packs_hold_the_rounded_product_and_zero_padding():
    """dtype float32 (the device's format): layouts 0 / 1 hold float32(src * scale); the three bf16 planes of layouts 3 / 4 / 5 are
    bf16 values whose sum is that float32 exactly; every pad is zero."""
    rng = np.random.default_rng(5)
    for rec, rfd1, flip, layouts, scaled in R.COMBINATIONS:
        for layout in layouts:
            if layout == 2:
                continue
            for rows, cols in ((24, 40), (4, 12), (64, 64)):
                D0, D1 = (cols, rows) if rfd1 else (rows, cols)
                rp, cp, _ = R.pack_dims(rows, cols, layout)
                w = rng.standard_normal((D0, D1, 3, 3)).astype(np.float32)
                scale = rng.uniform(0.25, 4.0, cols).astype(np.float32) if scaled else None
                P32 = R.pack(w, D0, D1, rfd1, flip, rp, cp, layout, scale=scale, dtype=np.float32)
                assert P32.dtype == np.float32
                base = 1 if layout == 4 else (0 if layout in (3, 5) else layout)
                plain = R.pack(w, D0, D1, rfd1, flip, rp, cp, base, scale=scale, dtype=np.float32)
                if layout in (3, 4, 5):
                    assert np.array_equal(R.bf16_rne(P32), P32)
                    assert np.array_equal(R.decode_split(P32, layout, rp, cp), plain.astype(np.float64))
                taps = plain.shape[0]
                mask = np.zeros((taps, rp, cp), bool)
                mask[:, :rows, :cols * (4 if base == 1 else 1)] = True
                assert not plain[~mask].any() and plain[mask].any()


@pytest.mark.parametrize("n_class", [1, 2, 3, 4, 5, 8])
def test_classifier_data_gradient_filter_has_the_tap_pitch_of_its_record(n_class):
    """The 3x3 classifier's data gradient contracts over 8 padded class channels (its record carries cin = 8), so its flipped filter
    is [9][8][cols_pad] for every class count: packed with the rows of the parameter alone (rows_pad 4 for 1..4 classes) the taps lie
    at half the pitch the kernel reads them at.  Dry-run lowering of the v2 net (concat skips, 3x3 classifier)."""
    import ctypes as C
    import robocupvision_amd.model as M
    from robocupvision_amd import _lib as L
    from robocupvision_amd.engine import CLS3_PAD, Engine
    model = M.ROBO_UNet(nClass=n_class, v2=True, classSize=3, levels=1, bellySize=2)
    eng = Engine(model._graph(), list(model.parameters()), M._bn_modules(model), dry_run=True)
    plan = eng._plan_for([torch.zeros(2, 3, 48, 64)], True)
    packs = [plan.fwd.arr[k] for k in range(plan.fwd.n) if plan.fwd.arr[k].kind == L.OP_PACK]
    assert len(packs) == 1
    count = packs[0].i[L.RCV_I_COUNT]
    tables = [t for t in plan.keep if t.dtype == torch.uint8 and t.numel() == count * C.sizeof(L.RcvPackJob)]
    assert len(tables) == 1
    jobs = (L.RcvPackJob * count).from_buffer_copy(tables[0].cpu().numpy().tobytes())
    ops = [plan.fwd.arr[k] for k in range(plan.fwd.n)] + [plan.bwd.arr[k] for k in range(plan.bwd.n)]
    # the classifier's data gradient is the one conv record of the backward list that reads its gradient plainly (no BatchNorm / ReLU
    # backward in the load: the class gradient itself)
    dgrads = [o for o in ops[plan.fwd.n:] if o.kind == L.OP_CONV and o.i[L.RCV_I_INMODE] == L.LOAD_PLAIN]
    assert len(dgrads) == 1 and dgrads[0].i[L.RCV_I_CIN] == CLS3_PAD
    flipped = [j for j in jobs if j.dst == dgrads[0].p[L.RCV_P_W]]
    assert len(flipped) == 1
    j = flipped[0]
    assert (j.D0, j.rows_from_d1, j.flip, j.merged) == (n_class, 0, 1, 0) and dgrads[0].i[L.RCV_I_COUT] == j.D1
    assert (j.rows_pad, j.cols_pad) == (CLS3_PAD, (j.D1 + 15) // 16 * 16)
    # every job of the plan: rows_pad is the padded contraction width of the record that reads it
    for jb in jobs:
        readers = [o for o in ops if o.kind in (L.OP_CONV, L.OP_TCONV) and o.p[L.RCV_P_W] == jb.dst]
        assert len(readers) == 1
        cin = readers[0].i[L.RCV_I_CIN]
        assert jb.rows_pad == R.pack_dims(cin, 1, jb.merged)[0], (jb.D0, jb.D1, jb.merged, jb.rows_pad, cin)


def test_pack_dims_are_the_engines():
    from test_gpu_kernels import _pack_dims
    from robocupvision_amd.engine import _round_up
    for c in cases():
        _, _, _, layout, _, rows, cols, _ = c
        merged = layout in (1, 4)
        assert R.pack_dims(rows, cols, layout, merged) == _pack_dims(rows, cols, layout, merged=merged), c
        # engine._Lowering.add_pack, restated once more from its own rounding helper
        split = layout in (3, 4, 5)
        rp = _round_up(rows, (16 if layout == 5 else (32 if rows > 32 else 8)) if split else 4)
        cp = _round_up(cols * (4 if merged else 1), 16)
        assert R.pack_dims(rows, cols, layout, merged)[:2] == (rp, cp), c
