"""GPU: the pooled classification head kernels (RCV_OP_POOL_CLS_FWD / _BWD, csrc/pool_cls.hip) driven through the C ABI (one record,
rcv_run) against float64 numpy: k x k max (k = 2, 4) with planes that leave a floor remainder, the plane mean, all three load modes,
both BatchNorm-backward statistics kinds, 1..8 classes, 64 / 96 / 128 channels, Dropout2d keep-scales, the skip-gradient add.  Inputs
carry ties on purpose (whole windows of one value, ReLU zeros): the gradient must reach the FIRST maximum of a window in row-major
order.  Two backward runs must be bitwise identical."""
import numpy as np
import pytest
import torch

from robocupvision_amd import _lib as L
from test_gpu_blocks import close

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


def _load(r, cst, mode):
    if mode == L.LOAD_PLAIN:
        return r
    v = r * cst[0] + cst[1]
    return np.maximum(v, 0.0) if mode == L.LOAD_AFFINE_RELU else v


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


def _reference(case, r, cst, w, b, scale, dl, res):
    N, H, W, C, nC, k, mode, stats, resid, drop = case
    r64, c64 = r.astype(np.float64), cst.astype(np.float64)
    v = _load(r64, c64, mode)
    Hp, Wp = (H // k, W // k) if k else (1, 1)
    if k:
        win = v[:, :Hp * k, :Wp * k, :].reshape(N, Hp, k, Wp, k, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, k * k, C)
        pooled = win.max(axis=3)
        first = win.argmax(axis=3)               # numpy: the first occurrence of the maximum = row-major window order
    else:
        pooled = v.mean(axis=(1, 2)).reshape(N, 1, 1, C)
    s = np.ones((N, 1, 1, C)) if scale is None else scale.astype(np.float64).reshape(N, 1, 1, C)
    pd = pooled * s
    w2 = w.reshape(nC, C).astype(np.float64)
    logits = np.einsum("nyxc,oc->noyx", pd, w2) + b.astype(np.float64).reshape(1, nC, 1, 1)
    dl64 = dl.astype(np.float64)
    dW = np.einsum("noyx,nyxc->oc", dl64, pd).reshape(nC, C, 1, 1)
    db = dl64.sum(axis=(0, 2, 3))
    dpool = np.einsum("noyx,oc->nyxc", dl64, w2) * s
    dy = np.zeros((N, H, W, C))
    if k:
        for j in range(k * k):
            sel = (first == j)
            dy[:, j // k:Hp * k:k, j % k:Wp * k:k, :][:, :Hp, :Wp, :] = np.where(sel, dpool, 0.0)
    else:
        dy[:] = dpool / (H * W)
    if res is not None:
        dy += res.astype(np.float64)
    st = None
    if stats != L.STATS_NONE:
        g = dy if stats == L.STATS_BWD_ENC else np.where(r64 * c64[0] + c64[1] > 0, dy, 0.0)
        st = np.stack([g.sum(axis=(0, 1, 2)), (g * (r64 - c64[2])).sum(axis=(0, 1, 2))])
    return pooled, logits, dW, db, dy, st


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
