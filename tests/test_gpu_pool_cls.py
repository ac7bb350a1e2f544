"""GPU: the pooled classification head kernels (RCV_OP_POOL_CLS_FWD / _BWD, csrc/pool_cls.hip) driven through the C ABI (one record,
rcv_run) against float64 numpy: k x k max (k = 2, 4) with planes that leave a floor remainder, the plane mean, all three load modes,
both BatchNorm-backward statistics kinds, 1..8 classes, 64 / 96 / 128 channels, Dropout2d keep-scales, the skip-gradient add.  Inputs
carry ties on purpose (whole windows of one value, ReLU zeros): the gradient must reach the FIRST maximum of a window in row-major
order.  Two backward runs must be bitwise identical.

Further down, the exact cases (operands on the integer grid of small_ops_restatement, built and pre-checked by
tests/pool_cls_restatement.py, whose float64 answers the kernels must equal bit for bit): the small planes with every channel count
the block size depends on (4, 20, 64, 260, 512) and 1 / 8 classes; one plane per channel count whose work items exceed one grid
pass of pool_cls_scatter_kernel (4 workgroups per CU, sized from rcv_num_cus at run time; each case asserts the inequality and
prints both numbers); the tie constructions; the launcher's refusals, which must launch nothing."""
import numpy as np
import pytest
import torch

import pool_cls_restatement as PR
from pool_cls_restatement import reference as _reference
from robocupvision_amd import _lib as L
from test_gpu_blocks import close
from test_gpu_small_ops import _exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# N, H, W, C, nC, k (0 = mean), load mode, statistics, resid, dropout
CASES = [
    (2, 9, 11, 64, 8, 2, L.LOAD_AFFINE_RELU, L.STATS_BWD_DEC, True, True),
    (3, 8, 8, 64, 1, 4, L.LOAD_AFFINE, L.STATS_BWD_ENC, False, False),
    (2, 6, 13, 128, 5, 4, L.LOAD_PLAIN, L.STATS_NONE, True, False),
    (5, 4, 4, 64, 5, 4, L.LOAD_AFFINE_RELU, L.STATS_BWD_DEC, False, False),      # the reference's size: 32x32 patches -> 4x4 f3
    (2, 8, 10, 96, 3, 2, L.LOAD_AFFINE, L.STATS_BWD_ENC, False, True),
    (4, 15, 20, 64, 5, 0, L.LOAD_AFFINE, L.STATS_BWD_ENC, False, True),          # PB_FCN_2 on 120x160
    (2, 5, 7, 128, 8, 0, L.LOAD_AFFINE_RELU, L.STATS_BWD_DEC, True, False),
    (2, 4, 4, 64, 1, 0, L.LOAD_PLAIN, L.STATS_NONE, False, True),
]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _case_inputs(case, seed):
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((N, H, W, C)).astype(np.float32)
    if k:
        Hp, Wp = H // k, W // k
        for n in range(N):                       # ties: whole windows of one value, and a window whose first column repeats
            r[n, 0:k, 0:k, :] = r[n, 0, 0, :]
            if Wp > 1:
                r[n, 0:k, k:2 * k, :] = r[n, 0:k, k:k + 1, :]
    cst = np.zeros((5, C), np.float32)
    cst[0] = rng.uniform(0.5, 1.5, C)
    cst[1] = rng.uniform(-0.5, 0.5, C)
    cst[1, : C // 4] = -2.5                      # mostly ReLU zeros on a quarter of the channels: all-zero windows
    cst[2] = rng.uniform(-0.3, 0.3, C)           # the batch mean the statistics are centred on
    w = (rng.standard_normal((nC, C, 1, 1)) * 0.2).astype(np.float32)
    b = rng.standard_normal(nC).astype(np.float32)
    scale = ((rng.random((N, C)) < 0.6) / 0.6).astype(np.float32) if drop else None
    return r, cst, w, b, scale


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_pool_cls_kernels_vs_float64(ci):
    case = CASES[ci]
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    Hp, Wp = (H // k, W // k) if k else (1, 1)
    r, cst, w, b, scale = _case_inputs(case, 100 + ci)
    rng = np.random.default_rng(200 + ci)
    dl = rng.standard_normal((N, nC, Hp, Wp)).astype(np.float32)
    res = rng.standard_normal((N, H, W, C)).astype(np.float32) if resid else None
    h = L.handle(0)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    r_d, cst_d, w_d, b_d = _dev(r), _dev(cst), _dev(w), _dev(b)
    s_d = _dev(scale) if scale is not None else None
    pooled_d = torch.zeros(N, Hp, Wp, C, device=DEV)
    logits_d = torch.zeros(N, nC, Hp, Wp, device=DEV)
    common = dict(n=N, h=H, w=W, cin=C, cout=nC, ho=Hp, wo=Wp, aux0=k, inmode=mode, p_in_c=cst_d.data_ptr(), p_w=w_d.data_ptr(),
                  p_x0=(s_d.data_ptr() if s_d is not None else 0), p_x1=pooled_d.data_ptr())
    fop = L.make_op(L.OP_POOL_CLS_FWD, 0, p_in=r_d.data_ptr(), p_bias=b_d.data_ptr(), p_out=logits_d.data_ptr(), **common)
    assert L.OpList([fop]).labels(h)[0].startswith("pool_cls_fwd<")
    L.OpList([fop]).run(h, stream)
    torch.cuda.synchronize()
    pooled, logits, dW, db, dy, st = _reference(case, r, cst, w, b, scale, dl, res)
    close(pooled_d, torch.from_numpy(pooled), "pooled", rtol=1e-5)
    close(logits_d, torch.from_numpy(logits), "logits", rtol=1e-4)

    dl_d = _dev(dl)
    res_d = _dev(res) if res is not None else None
    dw_d = torch.zeros(nC, C, 1, 1, device=DEV)
    db_d = torch.zeros(nC, device=DEV)
    dy_d = torch.zeros(N, H, W, C, device=DEV)
    bop = L.make_op(L.OP_POOL_CLS_BWD, L.F_RESID if resid else 0, stats=stats, p_in=dl_d.data_ptr(), p_epi_aux=r_d.data_ptr(),
                    p_epi_c=cst_d.data_ptr(), p_x2=dw_d.data_ptr(), p_x3=db_d.data_ptr(), p_out=dy_d.data_ptr(),
                    p_resid=(res_d.data_ptr() if res_d is not None else 0), **common)
    nbytes = L.op_workspace(h, bop)
    n_part = bop.i[L.RCV_I_NPART]
    assert nbytes == 4 * (n_part * 2 * C + N * Hp * Wp * C) and (n_part > 0) == (stats != L.STATS_NONE)
    part_d = torch.zeros(nbytes // 4, device=DEV)
    bop.p[L.RCV_P_PART] = part_d.data_ptr()
    assert L.OpList([bop]).labels(h)[0].startswith("pool_cls_bwd<")
    outs = []
    for _ in range(2):
        for t in (dw_d, db_d, dy_d, part_d):
            t.fill_(7.0)
        L.OpList([bop]).run(h, stream)
        torch.cuda.synchronize()
        outs.append([t.cpu().clone() for t in (dw_d, db_d, dy_d, part_d[:n_part * 2 * C])])
    for a, bb in zip(*outs):
        assert torch.equal(a, bb), "two backward runs differ"
    gw, gb, gy, gpart = outs[0]
    close(gw, torch.from_numpy(dW), "dW", rtol=1e-4, floor=1.0)
    close(gb, torch.from_numpy(db), "db", rtol=1e-4, floor=1.0)
    close(gy, torch.from_numpy(dy), "d source", rtol=1e-4)
    if k:       # the routing itself, exactly: where the reference puts a window's gradient (and nowhere else)
        base = torch.from_numpy(res) if res is not None else torch.zeros(N, H, W, C)
        got_nz, ref_nz = (gy - base).abs() > 1e-6, torch.from_numpy(np.abs(dy - base.double().numpy()) > 1e-6)
        assert torch.equal(got_nz, ref_nz), "%d elements routed differently" % int((got_nz != ref_nz).sum())
    if st is not None:
        rows = gpart.reshape(n_part, 2, C).double().sum(0)
        close(rows, torch.from_numpy(st), "statistics rows", rtol=1e-4, floor=1.0)


# ------------------------------------------------------------------------------------------ exact cases
assert (L.LOAD_PLAIN, L.LOAD_AFFINE, L.LOAD_AFFINE_RELU) == PR.MODES and (L.STATS_BWD_ENC, L.STATS_BWD_DEC, L.STATS_NONE) == PR.KINDS


def _cus():
    return int(L.load().rcv_num_cus(L.handle(0)))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _records(c, dev):
    """The forward and backward records of a case dict of PR.build (operands uploaded into `dev`, outputs NaN-filled)."""
    N, H, W, C, nC, k, mode, stats, resid, drop = c["case"]
    Hp, Wp = PR.pooled_plane(H, W, k)
    for name in ("r", "cst", "w", "b", "dl", "res", "scale"):
        dev[name] = _dev(c[name]) if c[name] is not None else None
    dev.update(pooled=_nan(N, Hp, Wp, C), logits=_nan(N, nC, Hp, Wp), dW=_nan(nC, C, 1, 1), db=_nan(nC), dy=_nan(N, H, W, C))
    ptr = lambda name: dev[name].data_ptr() if dev[name] is not None else 0
    common = dict(n=N, h=H, w=W, cin=C, cout=nC, ho=Hp, wo=Wp, aux0=k, inmode=mode, p_in_c=ptr("cst"), p_w=ptr("w"), p_x0=ptr("scale"),
                  p_x1=ptr("pooled"))
    fop = L.make_op(L.OP_POOL_CLS_FWD, 0, p_in=ptr("r"), p_bias=ptr("b"), p_out=ptr("logits"), **common)
    bop = L.make_op(L.OP_POOL_CLS_BWD, L.F_RESID if resid else 0, stats=stats, p_in=ptr("dl"), p_epi_aux=ptr("r"), p_epi_c=ptr("cst"),
                    p_x2=ptr("dW"), p_x3=ptr("db"), p_out=ptr("dy"), p_resid=ptr("res"), **common)
    return fop, bop


def _check_exact(c, what):
    """Forward once, backward twice (outputs and workspace NaN-filled before each): everything equals the restatement bit for bit,
    the partial statistics rows folded in float64, and the two backward runs are bitwise equal.  -> the number of partial rows."""
    N, H, W, C, nC, k, mode, stats, resid, drop = c["case"]
    h, stream = L.handle(0), torch.cuda.current_stream(DEV).cuda_stream
    dev = {}
    fop, bop = _records(c, dev)
    pooled, logits, dW, db, dy, st = _reference(c["case"], *PR.operands(c))
    L.OpList([fop]).run(h, stream)
    torch.cuda.synchronize()
    _exact(dev["pooled"], pooled, what + " pooled")
    _exact(dev["logits"], logits, what + " logits")
    nbytes = L.op_workspace(h, bop)
    n_part = bop.i[L.RCV_I_NPART]
    M = N * (H // k if k else 1) * (W // k if k else 1)
    assert nbytes == 4 * (n_part * 2 * C + M * C) and (n_part > 0) == (stats != L.STATS_NONE)
    assert n_part in (0, min(-(-PR.items(c["case"]) // PR.block(C)), 4 * _cus()))
    part = _nan(nbytes // 4)
    bop.p[L.RCV_P_PART] = part.data_ptr()
    outs = []
    for _ in range(2):
        for name in ("dW", "db", "dy"):
            dev[name].fill_(float("nan"))
        part.fill_(float("nan"))
        L.OpList([bop]).run(h, stream)
        torch.cuda.synchronize()
        outs.append([dev[name].clone() for name in ("dW", "db", "dy")] + [part[:n_part * 2 * C].clone()])
    gw, gb, gy, gpart = outs[0]
    _exact(gw, dW, what + " dW")
    _exact(gb, db, what + " db")
    _exact(gy, dy, what + " d source")
    if st is not None:
        _exact(gpart.reshape(n_part, 2, C).double().sum(0), st, what + " statistics rows")
    for a, b_ in zip(*outs):
        assert torch.equal(_bits(a), _bits(b_)), what + ": two backward runs differ"
    return n_part


@pytest.mark.parametrize("C", PR.CHANNELS)
def test_pool_cls_exact_small_planes(C):
    """2x9x11 (the remainder rows and columns get exactly 0 + resid and still count in the statistics), single windows, the 1x1 mean
    of three images, small plane means; every load mode, statistics kind (and none), with and without residual and dropout."""
    for ci, case in enumerate(PR.small_cases()):
        if case[3] != C:
            continue
        c = PR.build(case, seed=ci)
        PR.check(c)
        _check_exact(c, "pool_cls %s" % (case,))
        if case[:3] == (2, 9, 11) and case[8]:
            N, H, W, _, _, k = case[:6]
            assert c["res"][:, (H // k) * k:].any() and c["res"][:, :, (W // k) * k:].any()


BIG = len(PR.big_cases(256))


@pytest.mark.parametrize("bi", range(BIG))
def test_pool_cls_exact_beyond_one_grid_pass(bi):
    """One case per channel count (and two more: a plane mean without residual at C = 4, a work-item count that is no multiple of the
    block) sized from the device's CU count so that pool_cls_scatter_kernel goes round its grid-stride loop a second time: the
    statistics accumulators carried across the passes, the item -> (n, y, x, quad) decode beyond the first pass.  The first pixel of
    the second pass and the last pixel carry non-zero terms in every channel (PR.check: losing either changes every statistics
    entry, and every dW entry for the mean)."""
    cus = _cus()
    case = PR.big_cases(cus)[bi]
    C = case[3]
    cap = PR.pass_items(cus, C)
    print("pool_cls %s: %d work items, one grid pass covers %d (%d CUs x 4 workgroups x %d threads)" % (case, PR.items(case), cap, cus, PR.block(C)))
    assert PR.items(case) > cap
    if bi == BIG - 1:
        assert PR.items(case) % PR.block(C) != 0
    c = PR.build(case, second_item=cap, seed=bi)
    assert c["sensitive"] and c["second"] == cap // (C // 4)
    PR.check(c)
    n_part = _check_exact(c, "pool_cls %s" % (case,))
    assert n_part == 4 * cus and n_part * PR.block(C) < PR.items(case), "the launcher's grid is not the capped one this case was sized for"


@pytest.mark.parametrize("mode", PR.MODES)
@pytest.mark.parametrize("k", [2, 4])
def test_pool_cls_ties_exact(mode, k):
    """Whole windows of one value, a window whose columns repeat, a maximum that comes again in the window's last position only, an
    all -2.5 window (zero after the ReLU: the first pixel wins), channels that are ReLU zeros almost everywhere."""
    c = PR.build_ties(mode, k)
    PR.check(c, unit=0.5)
    _check_exact(c, "pool_cls ties k=%d mode %d" % (k, mode))


def test_pool_cls_refusals_launch_nothing():
    """What the launcher refuses it refuses before any launch: the outputs keep their fill."""
    h, stream = L.handle(0), torch.cuda.current_stream(DEV).cuda_stream
    big = torch.zeros(1 << 16, device=DEV)
    outs = [torch.full((1 << 16,), 7.0, device=DEV) for _ in range(6)]
    base = dict(n=2, h=8, w=8, cin=64, cout=5, ho=4, wo=4, aux0=2, inmode=L.LOAD_AFFINE)
    bad = [dict(cin=516), dict(cin=6), dict(cin=0), dict(cout=9), dict(cout=0), dict(aux0=3), dict(aux0=1), dict(h=3, w=3, aux0=4, ho=0, wo=0),
           dict(h=3, w=3, aux0=4, ho=1, wo=1), dict(ho=3), dict(wo=5), dict(ho=8, wo=8), dict(aux0=0), dict(aux0=4)]
    for kw in bad:
        rec = dict(base)
        rec.update(kw)
        fop = L.make_op(L.OP_POOL_CLS_FWD, 0, p_in=big.data_ptr(), p_in_c=big.data_ptr(), p_w=big.data_ptr(), p_bias=big.data_ptr(),
                        p_x1=outs[0].data_ptr(), p_out=outs[1].data_ptr(), **rec)
        bop = L.make_op(L.OP_POOL_CLS_BWD, 0, stats=L.STATS_BWD_ENC, p_in=big.data_ptr(), p_in_c=big.data_ptr(), p_w=big.data_ptr(),
                        p_epi_aux=big.data_ptr(), p_epi_c=big.data_ptr(), p_x1=big.data_ptr(), p_x2=outs[2].data_ptr(), p_x3=outs[3].data_ptr(),
                        p_out=outs[4].data_ptr(), p_part=outs[5].data_ptr(), npart=1, **rec)
        for op in (fop, bop):
            with pytest.raises(L.RcvError):
                L.op_workspace(h, op)
            with pytest.raises(L.RcvError):
                L.OpList([op]).run(h, stream)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all()), "a refused record wrote to its outputs"
