"""GPU: RCV_OP_PRUNE (csrc/prune.hip) -- the three mask builders of the prune stage, one launch per model -- through the C ABI
(rcv_prune) and through model.pruneModelNew / pruneModel / pruneModel2, against the reference's recorded answers
(tests/golden/prune.npz), the numpy restatement (tests/prune_restatement.py) and torch.topk composed on the same card.  Everything
is exact: the rules decide on integer counts, a maximum and the fp32 rounding of float64 sums.

The tensors sit either in separate allocations or, as the engine lays parameters out, in one buffer -- here at float offsets that are
odd and run through every residue mod 4, so the float4 path has to peel."""
import contextlib
import io

import numpy as np
import pytest
import torch

import prune_restatement as R
from robocupvision_amd import _lib as L
import robocupvision_amd.model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLACEMENTS = ["separate", "flat"]


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def _weights(g, prefix="w"):
    return [g["%s%d" % (prefix, k)] for k in range(len(R.SHAPES))]


def _place(arrs, placement):
    """Device copies of ``arrs``: separate tensors, or views of one buffer at offsets 1, 2, 3 (mod 4) in turn."""
    if placement == "separate":
        return [torch.from_numpy(a.copy()).to(DEV) for a in arrs]
    offs, n = [], 0
    for k, a in enumerate(arrs):
        n += 1
        while n % 4 != (k % 3) + 1:
            n += 1
        offs.append(n)
        n += a.size
    buf = torch.full((n + 5,), 7.0, dtype=torch.float32, device=DEV)          # the gaps must come back untouched
    out = []
    for a, o in zip(arrs, offs):
        v = buf[o:o + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 != 0
        out.append(v)
    _place.last = (buf, offs, [a.size for a in arrs])
    return out


def _gaps_untouched():
    buf, offs, sizes = _place.last
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = False
    return bool((buf[keep] == 7.0).all())


def _abi(tensors, rule, ratio=0.0, lower=0.0, upper=0.0, amounts=None):
    """rcv_prune over the tensors with dim() > 1 -> (masks as numpy bool arrays, the job rows read back)."""
    big = [t for t in tensors if t.dim() > 1]
    total = sum(t.numel() for t in big)
    mbuf = torch.full((total + 3,), 255, dtype=torch.uint8, device=DEV)       # every mask byte must be written, amount == 0 included
    table = (L.RcvPruneJob * len(big))()
    off = 1                                                                    # masks need no alignment at all
    offs = []
    for k, t in enumerate(big):
        j = table[k]
        j.w, j.mask, j.n = t.data_ptr(), mbuf.data_ptr() + off, t.numel()
        j.amount = 0 if amounts is None else amounts[k]
        j.ratio, j.lower, j.upper = ratio, lower, upper
        offs.append(off)
        off += t.numel()
    lib = L.load()
    assert lib.rcv_prune_check(table, len(big), rule) == 0, lib.rcv_last_error()
    jobs = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    L.check(lib.rcv_prune(L.handle(0), jobs.data_ptr(), len(big), rule, torch.cuda.current_stream().cuda_stream), "rcv_prune")
    rows = (L.RcvPruneJob * len(big)).from_buffer_copy(jobs.cpu().numpy().tobytes())
    host = mbuf.cpu().numpy()
    assert host[0] == 255 and np.all(host[off:] == 255)
    for r, o, t in zip(rows, offs, big):          # a job that ends with status 0 wrote every mask byte; a refused one wrote none
        assert set(np.unique(host[o:o + t.numel()])) <= ({0, 1} if r.result[3] == 0 else {255})
    masks = [host[o:o + t.numel()].reshape(tuple(t.shape)) == 1 for o, t in zip(offs, big)]
    return masks, rows


def _py(fn, tensors, *args):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        masks = fn(tensors, *args)
    assert all(m.dtype == torch.bool and m.device.type == "cuda" for m in masks)
    assert len({m.untyped_storage().data_ptr() for m in masks}) <= 1          # views of ONE buffer
    assert out.getvalue().count("Pruned ") == len(masks)
    return [m.cpu().numpy() for m in masks], out.getvalue()


def _run(via, tensors, rule, **kw):
    if via == "abi":
        return _abi(tensors, rule, **kw)[0]
    if rule == L.PRUNE_MAX_RATIO:
        return _py(M.pruneModelNew, tensors, kw["ratio"])[0]
    if rule == L.PRUNE_STD_SEARCH:
        return _py(M.pruneModel, tensors, kw["lower"], kw["upper"])[0]
    return _py(M.pruneModel2, tensors, *kw["py_args"])[0]


def _amounts(arrs, ratio):
    return [R.amount_for(a.size, ratio, R.LT, R.HT) for a in arrs if a.ndim > 1]


def _check_against(tensors, masks, want_w, want_m, what):
    assert len(masks) == len(want_m)
    for k, (t, w) in enumerate(zip(tensors, want_w)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), np.asarray(w).view(np.uint32)), "%s: weights of tensor %d" % (what, k)
    for j, (m, wm) in enumerate(zip(masks, want_m)):
        assert m.shape == wm.shape and np.array_equal(m, wm), "%s: mask %d" % (what, j)


@pytest.mark.parametrize("via", ["abi", "python"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule0_vs_golden_and_cpu_path(gold, placement, via):
    ws = _weights(gold)
    ts = _place(ws, placement)
    masks = _run(via, ts, L.PRUNE_MAX_RATIO, ratio=R.RATIO0)
    n_masks = len(masks)
    _check_against(ts, masks, _weights(gold, "r0_w"), [gold["r0_m%d" % j] for j in range(n_masks)], "pruneModelNew vs golden")
    cpu = [torch.from_numpy(w.copy()) for w in ws]
    with contextlib.redirect_stdout(io.StringIO()):
        cpu_masks = M.pruneModelNew(cpu, R.RATIO0)
    _check_against(ts, masks, [c.numpy() for c in cpu], [m.numpy() for m in cpu_masks], "pruneModelNew vs its CPU path")
    assert placement == "separate" or _gaps_untouched()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule0_rows(gold, placement):
    ws = _weights(gold)
    _, rows = _abi(_place(ws, placement), L.PRUNE_MAX_RATIO, ratio=R.RATIO0)
    for r, w in zip(rows, [w for w in ws if w.ndim > 1]):
        _, _, thresh, n_below, n_nonzero = R.rule0(w, R.RATIO0)
        assert np.float32(r.thresh).view(np.uint32) == thresh.view(np.uint32)
        assert (r.result[0], r.result[1], r.result[2], r.result[3]) == (n_below, n_nonzero, 0, 0)


@pytest.mark.parametrize("via", ["abi", "python"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule1_vs_golden(gold, placement, via):
    ts = _place(_weights(gold), placement)
    masks = _run(via, ts, L.PRUNE_STD_SEARCH, lower=R.LOWER, upper=R.UPPER)
    _check_against(ts, masks, _weights(gold, "r1_w"), [gold["r1_m%d" % j] for j in range(len(masks))], "pruneModel vs golden")
    assert placement == "separate" or _gaps_untouched()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule1_thresholds_and_steps(gold, placement):
    ws = _weights(gold)
    _, rows = _abi(_place(ws, placement), L.PRUNE_STD_SEARCH, lower=R.LOWER, upper=R.UPPER)
    for r, w in zip(rows, [w for w in ws if w.ndim > 1]):
        _, _, thresh, n_below, n_nonzero, steps, status = R.rule1(w, R.LOWER, R.UPPER)
        print("n %6d  thresh %.9g (restatement %.9g)  steps %d (%d)" % (w.size, r.thresh, thresh, r.result[2], steps))
        assert np.float32(r.thresh).view(np.uint32) == thresh.view(np.uint32)
        assert (r.result[0], r.result[1], r.result[2], r.result[3]) == (n_below, n_nonzero, steps, status) and status == 0


def _topk_composed(tensors, amounts):
    """model.py:656-670 with torch ops on the same card"""
    out_w, out_m = [], []
    it = iter(amounts)
    for t in tensors:
        t = t.clone()
        if t.dim() > 1:
            amount = next(it)
            flat = t.reshape(-1)
            if amount > 0:
                _, idx = torch.topk(torch.abs(flat), amount, dim=0, largest=False)
                flat[idx] = 0.0
            out_m.append((t == 0.0).cpu().numpy())
        out_w.append(t.cpu().numpy())
    return out_w, out_m


@pytest.mark.parametrize("via", ["abi", "python"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule2_tie_free_two_rounds(gold, placement, via):
    ws = _weights(gold)
    ts = _place(ws, placement)
    for ratio, tag in ((R.RATIO2, "r2"), (R.RATIO2B, "r2b")):          # round two runs on the output of round one: its zeros go first
        amounts = _amounts(ws, ratio)
        assert amounts[0] == 0 and len(set(amounts)) >= 4               # r = 0, 0.8 ratio, ratio and 1.05 ratio all occur
        want_w, want_m = _topk_composed(ts, amounts)
        masks = _run(via, ts, L.PRUNE_SMALLEST_K, amounts=amounts, py_args=(ratio, R.LT, R.HT)) if via == "python" else \
            _abi(ts, L.PRUNE_SMALLEST_K, amounts=amounts)[0]
        _check_against(ts, masks, _weights(gold, tag + "_w"), [gold["%s_m%d" % (tag, j)] for j in range(len(masks))], tag + " vs golden")
        _check_against(ts, masks, want_w, want_m, tag + " vs torch.topk on the card")
        assert not masks[0].any()                                       # amount == 0: the mask is written all the same
    assert placement == "separate" or _gaps_untouched()


@pytest.mark.parametrize("via", ["abi", "python"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rule2_heavy_ties(placement, via):
    ws = [R.grid_weights(100 + k, s) for k, s in enumerate(R.SHAPES)]
    ts = _place(ws, placement)
    amounts = _amounts(ws, R.RATIO2)
    masks = _run(via, ts, L.PRUNE_SMALLEST_K, amounts=amounts, py_args=(R.RATIO2, R.LT, R.HT)) if via == "python" else \
        _abi(ts, L.PRUNE_SMALLEST_K, amounts=amounts)[0]
    j = 0
    for k, (w, t) in enumerate(zip(ws, ts)):
        got = t.cpu().numpy()
        if w.ndim == 1:
            assert np.array_equal(got.view(np.uint32), w.view(np.uint32))          # bit-identical: no job, not touched
            continue
        amount, m = amounts[j], masks[j]
        j += 1
        a, flat, gone = np.abs(w).reshape(-1), got.reshape(-1), m.reshape(-1)
        zeros_before = int((w == 0).sum())
        assert int(gone.sum()) == max(amount, zeros_before) and np.array_equal(gone, flat == 0)
        assert np.array_equal(flat[~gone].view(np.uint32), w.reshape(-1)[~gone].view(np.uint32))      # kept weights keep their bits
        if gone.any() and (~gone).any():
            boundary = a[gone].max()
            assert boundary <= a[~gone].min()
            tied = np.nonzero(a == boundary)[0]
            n_gone = int(gone[tied].sum())
            assert np.array_equal(np.nonzero(gone[tied])[0], np.arange(n_gone))    # of the boundary value the lowest indices went
        want_w, want_m = R.rule2(w, amount)
        assert np.array_equal(got.view(np.uint32), want_w.view(np.uint32)) and np.array_equal(m, want_m)
    assert placement == "separate" or _gaps_untouched()


def test_search_cap_is_reported_and_raises():
    w = R.oscillating_tensor()
    out = R.rule1(w, R.LOWER, R.UPPER)
    assert out[6] == R.ST_NO_END and out[5] == R.MAX_ITER                 # the restatement oscillates between 50 % and 100 %
    ok = R.tie_free(np.random.default_rng(9), (8, 3, 3, 3))
    ts = [torch.from_numpy(ok.copy()).to(DEV), torch.from_numpy(w.copy()).to(DEV)]
    _, rows = _abi(ts, L.PRUNE_STD_SEARCH, lower=R.LOWER, upper=R.UPPER)
    assert rows[0].result[3] == 0
    assert rows[1].result[3] == L.PRUNE_ST_NO_END and rows[1].result[2] == L.PRUNE_MAX_ITER
    assert np.float32(rows[1].thresh).view(np.uint32) == out[2].view(np.uint32)
    assert np.array_equal(ts[1].cpu().numpy(), w)                          # untouched
    ts = [torch.from_numpy(ok.copy()).to(DEV), torch.from_numpy(w.copy()).to(DEV)]
    with pytest.raises(L.RcvError, match="parameter 1"):
        _py(M.pruneModel, ts, R.LOWER, R.UPPER)


def test_device_refusals():
    with pytest.raises(ZeroDivisionError, match="parameter 1"):
        _py(M.pruneModel, [torch.ones(4, 4, device=DEV).cumsum(0), torch.zeros(5, 5, device=DEV)])
    with pytest.raises(L.RcvError, match="job 0"):
        _py(M.pruneModel, [torch.ones(1, 1, device=DEV)])
    with pytest.raises(L.RcvError, match="amount"):
        _py(M.pruneModel2, [torch.ones(20, 10, device=DEV)], 1.5, 1000, 50000)
    assert _py(M.pruneModelNew, [torch.ones(3, device=DEV)])[0] == []        # nothing with dim() > 1: no launch, no masks
