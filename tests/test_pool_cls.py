"""CPU: the float64 restatement of the pooled classification head (tests/pool_cls_restatement.py) against float64 torch autograd --
max_pool2d(k) or adaptive_avg_pool2d(1), a per-(n, c) keep-scale, a 1x1 conv -- with the first-maximum tie rule, the statistics
rows from their definition, and the preconditions of every exact case of tests/test_gpu_pool_cls.py (sized for 256 CUs here; on
the device the planes follow rcv_num_cus)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cls_restatement as PR
import small_ops_restatement as S
from robocupvision_amd import _lib as L

CUS = 256


def _autograd(case, r, cst, w, b, scale, dl):
    N, H, W, C, nC, k = case[:6]
    v = torch.from_numpy(PR.load(r.astype(np.float64), cst.astype(np.float64), case[6])).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    bt = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    pooled = F.max_pool2d(v, k) if k else F.adaptive_avg_pool2d(v, 1)
    pd = pooled if scale is None else pooled * torch.from_numpy(scale.astype(np.float64)).reshape(N, C, 1, 1)
    logits = F.conv2d(pd, wt, bt)
    (logits * torch.from_numpy(dl.astype(np.float64))).sum().backward()
    return (pooled.detach().permute(0, 2, 3, 1).numpy(), logits.detach().numpy(), wt.grad.numpy(), bt.grad.numpy(),
            v.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("k,plane", [(2, (2, 9, 11)), (4, (2, 9, 11)), (4, (3, 6, 13)), (0, (2, 5, 7)), (0, (3, 4, 8))])
@pytest.mark.parametrize("mode", PR.MODES)
@pytest.mark.parametrize("drop", [False, True])
def test_restatement_equals_float64_autograd(k, plane, mode, drop):
    """Random operands, and integer-grid operands whose windows are full of ties: torch routes a window's gradient to its first
    maximum in row-major order, and so does the restatement."""
    N, H, W = plane
    for C, nC in ((8, 3), (20, 8)):
        case = (N, H, W, C, nC, k, mode, PR.STATS_NONE, False, drop)
        rng = np.random.default_rng(10 * k + mode + C)
        Hp, Wp = PR.pooled_plane(H, W, k)
        for tied in (False, True):
            if tied:
                r, cst = S.grid(rng, (N, H, W, C), 1), S.grid_consts(rng, C)
            else:
                r, cst = rng.standard_normal((N, H, W, C)), rng.standard_normal((5, C))
            w, b, dl = rng.standard_normal((nC, C, 1, 1)), rng.standard_normal(nC), rng.standard_normal((N, nC, Hp, Wp))
            scale = (2.0 * (rng.random((N, C)) < 0.5)) if drop else None
            if tied and k:
                win = PR.windows(PR.load(r.astype(np.float64), cst.astype(np.float64), mode), k)
                top = np.sort(win, 3)
                assert (top[:, :, :, -1] == top[:, :, :, -2]).mean() > 0.3
            got = PR.reference(case, r, cst, w, b, scale, dl, None)
            for name, a, t in zip(("pooled", "logits", "dW", "db", "d source"), got, _autograd(case, r, cst, w, b, scale, dl)):
                assert a.shape == t.shape or name == "dW", (name, a.shape, t.shape)
                assert np.abs(a.reshape(t.shape) - t).max() <= 1e-12 * max(1.0, np.abs(t).max()), (name, tied)
            if k and (H % k or W % k):         # the floor remainder gets no gradient
                assert not got[4][:, Hp * k:].any() and not got[4][:, :, Wp * k:].any()
            res = rng.standard_normal((N, H, W, C))
            assert np.array_equal(PR.reference(case[:8] + (True, drop), r, cst, w, b, scale, dl, res)[4], got[4] + res)


@pytest.mark.parametrize("kind", [PR.STATS_BWD_ENC, PR.STATS_BWD_DEC])
def test_statistics_rows_follow_their_definition(kind):
    """pool_cls_scatter_kernel's header: row 0 = sum v, row 1 = sum v (e - mu) with v = dy (ENC) or dy where e c0 + c1 > 0 (DEC),
    e = the stored tensor, c0 / c1 / mu = rows 0 / 1 / 2 of the producer's constants -- spelled out pixel by pixel; the remainder
    pixels of a max plane carry the residual alone and still count."""
    case = (2, 5, 7, 8, 3, 2, PR.LOAD_AFFINE_RELU, kind, True, True)
    c = PR.build(case)
    r, cst = c["r"].astype(np.float64), c["cst"].astype(np.float64)
    dy, st = PR.reference(case, *PR.operands(c))[4:]
    rows = np.zeros((2, 8))
    for n in range(2):
        for y in range(5):
            for x in range(7):
                for ch in range(8):
                    v = dy[n, y, x, ch]
                    if kind == PR.STATS_BWD_DEC and not r[n, y, x, ch] * cst[0, ch] + cst[1, ch] > 0:
                        v = 0.0
                    rows[0, ch] += v
                    rows[1, ch] += v * (r[n, y, x, ch] - cst[2, ch])
    assert np.array_equal(rows, st) and np.array_equal(st, S.stats(kind, dy, r, cst))
    assert np.array_equal(dy[:, 4], c["res"][:, 4]) and np.array_equal(dy[:, :, 6], c["res"][:, :, 6]) and c["res"][:, 4].any()
    keep = np.ones(70, bool)
    keep[34] = False                  # the remainder pixel (0, 4, 6): dropping it moves the rows by its residual
    st2 = PR.reference(case, *PR.operands(c), keep=keep)[5]
    v = dy[0, 4, 6] * ((r[0, 4, 6] * cst[0] + cst[1] > 0) if kind == PR.STATS_BWD_DEC else 1.0)
    assert np.array_equal(st[0] - st2[0], v) and np.array_equal(st[1] - st2[1], v * (r[0, 4, 6] - cst[2]))


def test_launch_geometry():
    assert [PR.block(C) for C in PR.CHANNELS] == [256, 255, 256, 195, 256]
    assert PR.pass_items(CUS, 64) == 262144 and PR.items((64, 15, 20, 64)) == 307200          # PB_FCN_2, batch 64 on 120x160: two passes


def test_small_cases_cover_the_axes_and_hold_their_preconditions():
    cases = PR.small_cases()
    assert len(set(cases)) == len(cases)
    for k in (0, 2, 4):
        mine = [c for c in cases if c[5] == k]
        assert {c[6] for c in mine} == set(PR.MODES) and {c[7] for c in mine} == set(PR.KINDS), k
        assert {c[8] for c in mine} == {False, True} and {c[9] for c in mine} == {False, True}, k
        assert {(c[3], c[4]) for c in mine} >= {(C, nC) for C in PR.CHANNELS for nC in (1, 8)}
    assert {c[:3] + (c[5],) for c in cases} >= {(2, 9, 11, 2), (2, 9, 11, 4), (1, 2, 2, 2), (1, 4, 4, 4), (3, 1, 1, 0)}
    for ci, case in enumerate(cases):
        c = PR.build(case, seed=ci)
        PR.check(c)
        if case[5]:
            win = PR.windows(PR.load(c["r"].astype(np.float64), c["cst"].astype(np.float64), case[6]), case[5])
            assert win.shape[3] == case[5] ** 2
        s = c["scale"]
        assert s is None or set(np.unique(s)) <= {0.0, 2.0}


def test_big_cases_exceed_one_pass_and_hold_their_preconditions():
    cases = PR.big_cases(CUS)
    assert {c[3] for c in cases} == set(PR.CHANNELS) and {c[4] for c in cases} >= {1, 8} and {c[5] for c in cases} == {0, 2, 4}
    sensed = 0
    for ci, case in enumerate(cases):
        cap = PR.pass_items(CUS, case[3])
        assert PR.items(case) > cap and cap % (case[3] // 4) == 0
        c = PR.build(case, second_item=cap, seed=ci)
        assert c["second"] == cap // (case[3] // 4) and 0 < c["second"] < c["npix"] - 1
        PR.check(c)
        sensed += c["sensitive"] and case[7] != PR.STATS_NONE
    assert sensed == len(cases)
    assert PR.items(cases[-1]) % PR.block(cases[-1][3]) != 0


def test_the_launcher_caps_the_big_cases_grid():
    """The query on a 256-CU planner handle: every big case gets the capped grid (one partial row per workgroup), whose single pass
    is short of the case's work items; the restated block size is the launcher's (the uncapped grid of a small plane shows it)."""
    h = L.planner_handle(CUS)
    for case in PR.big_cases(CUS) + [c for c in PR.small_cases() if c[7] != PR.STATS_NONE]:
        N, H, W, C, nC, k, mode, stats = case[:8]
        Hp, Wp = PR.pooled_plane(H, W, k)
        op = L.make_op(L.OP_POOL_CLS_BWD, 0, n=N, h=H, w=W, cin=C, cout=nC, ho=Hp, wo=Wp, aux0=k, inmode=mode, stats=stats)
        nbytes = L.op_workspace(h, op)
        n_part = op.i[L.RCV_I_NPART]
        assert n_part == min(-(-PR.items(case) // PR.block(C)), 4 * CUS) and nbytes == 4 * (n_part * 2 * C + N * Hp * Wp * C)
        assert (n_part * PR.block(C) < PR.items(case)) == (case in PR.big_cases(CUS))


def test_a_lost_second_pass_pixel_is_seen():
    """What the sensitivity check is for: the restatement without the first pixel of the second pass differs from the full one in
    every statistics entry (and in every dW entry for the mean), so a bit-for-bit comparison cannot miss such a loss."""
    for case in (PR.big_cases(CUS)[2], PR.big_cases(CUS)[3]):
        cap = PR.pass_items(CUS, case[3])
        c = PR.build(case, second_item=cap)
        idx, masks = S.drop_masks(c["npix"], c["second"])
        assert idx == [c["npix"] - 1, cap // (case[3] // 4)]
        for keep in masks:
            for a, b in zip(PR.reduced(c), PR.reduced(c, keep)):
                assert np.all(a != b)


@pytest.mark.parametrize("mode", PR.MODES)
@pytest.mark.parametrize("k", [2, 4])
def test_tie_cases(mode, k):
    c = PR.build_ties(mode, k)
    PR.check(c, unit=0.5)
    case = c["case"]
    dy = PR.reference(case, *PR.operands(c))[4] - c["res"]
    g = PR._parts(case, *PR.operands(c), None)[-1]            # d loss / d pooled
    lit = g[0] != 0
    v = PR.load(c["r"].astype(np.float64), c["cst"].astype(np.float64), mode)
    for (py, px), (wy, wx) in (((0, 0), (0, 0)), ((1, 0), (0, 1)), ((1, 1), (0, 0))):
        win = dy[0, py * k:(py + 1) * k, px * k:(px + 1) * k]
        flat = v[0, py * k, px * k] == v[0, py * k + wy, px * k + wx]          # a ReLU-zero window: its first pixel wins
        assert np.array_equal(np.where(flat, win[0, 0], win[wy, wx]), g[0, py, px]), (py, px)
        assert int((win != 0).sum()) == int(lit[py, px].sum()), (py, px)
    assert not (v[0, k, 0] == v[0, k, 1])[16:].any() and (mode != PR.LOAD_AFFINE_RELU or (v[0, k, 0] == v[0, k, 1])[:16].all())
    win = dy[0, :k, k:2 * k]                                  # columns repeat: the gradient stays in the first
    assert np.array_equal(win[:, 0].sum(0), g[0, 0, 1]) and not win[:, 1:].any() and int((win != 0).sum()) == int(lit[0, 1].sum())
    assert lit[:2, :2].all()
    assert (v[0, k, 1] == v[0, 2 * k - 1, k - 1]).all() and (v[0, k:2 * k, :k].max((0, 1)) == v[0, k, 1]).all()
    if mode == PR.LOAD_AFFINE_RELU:
        assert not v[0, k:2 * k, k:2 * k].any()
