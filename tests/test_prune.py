"""CPU: the prune stage's mask builders (model.pruneModelNew / pruneModel / pruneModel2) against the reference's recorded answers
(tests/golden/prune.npz, written by tests/golden/make_golden_prune.py) and the numpy restatement (tests/prune_restatement.py); the
refusals of the device entry points (rcv_prune_check, rcv_prune on a planning handle, the status rows) without any compute."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import prune_restatement as R
from robocupvision_amd import _lib as L
import robocupvision_amd.model as M


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def _weights(g):
    return [g["w%d" % k] for k in range(len(R.SHAPES))]


def _big(arrs):
    return [(k, a) for k, a in enumerate(arrs) if a.ndim > 1]


def _quiet(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


def test_names_are_exported():
    assert "pruneModel" in M.__all__ and "pruneModel2" in M.__all__ and "pruneModelNew" in M.__all__
    assert callable(M.pruneModel) and callable(M.pruneModel2)


def test_golden_shapes(gold):
    ws = _weights(gold)
    assert [w.shape for w in ws] == R.SHAPES and all(w.dtype == np.float32 for w in ws)
    assert sum(w.size for w in ws) < 20000


def test_restatement_reproduces_the_reference(gold):
    ws = _weights(gold)
    for j, (k, w) in enumerate(_big(ws)):
        w0, m0 = R.rule0(w, R.RATIO0)[:2]
        assert np.array_equal(w0, gold["r0_w%d" % k]) and np.array_equal(m0, gold["r0_m%d" % j])
        out = R.rule1(w, R.LOWER, R.UPPER)
        assert out[6] == R.ST_OK
        assert np.array_equal(out[0], gold["r1_w%d" % k]) and np.array_equal(out[1], gold["r1_m%d" % j])
        amount = R.amount_for(w.size, R.RATIO2, R.LT, R.HT)
        w2, m2 = R.rule2(w, amount)
        assert np.array_equal(w2, gold["r2_w%d" % k]) and np.array_equal(m2, gold["r2_m%d" % j])
        assert int(m2.sum()) == amount
        amount_b = R.amount_for(w.size, R.RATIO2B, R.LT, R.HT)
        w2b, m2b = R.rule2(w2, amount_b)
        assert np.array_equal(w2b, gold["r2b_w%d" % k]) and np.array_equal(m2b, gold["r2b_m%d" % j])
        assert int(m2b.sum()) == max(amount, amount_b)
    assert {R.amount_for(w.size, R.RATIO2, R.LT, R.HT) == 0 for w in ws} == {True, False}          # amount == 0 occurs
    for k, w in enumerate(ws):
        if w.ndim == 1:
            for tag in ("r0", "r1", "r2", "r2b"):
                assert np.array_equal(gold["%s_w%d" % (tag, k)], w)


@pytest.mark.parametrize("tag", ["r0", "r1", "r2", "r2b"])
def test_cpu_functions_match_the_reference(gold, tag):
    src = _weights(gold) if tag != "r2b" else [gold["r2_w%d" % k] for k in range(len(R.SHAPES))]
    ts = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in src]
    fn, args = {"r0": (M.pruneModelNew, (R.RATIO0,)), "r1": (M.pruneModel, (R.LOWER, R.UPPER)),
                "r2": (M.pruneModel2, (R.RATIO2, R.LT, R.HT)), "r2b": (M.pruneModel2, (R.RATIO2B, R.LT, R.HT))}[tag]
    masks, text = _quiet(fn, ts, *args)
    assert len(masks) == len(_big(src)) and text.count("Pruned ") == len(masks)
    for j, (k, _) in enumerate(_big(src)):
        assert masks[j].dtype == torch.bool and tuple(masks[j].shape) == R.SHAPES[k]
        assert np.array_equal(masks[j].numpy(), gold["%s_m%d" % (tag, j)])
    for k, t in enumerate(ts):
        assert np.array_equal(t.detach().numpy(), gold["%s_w%d" % (tag, k)])


def test_print_lines_are_the_references():
    w = torch.nn.Parameter(torch.from_numpy(R.tie_free(np.random.default_rng(5), (20, 30))))
    _, text = _quiet(M.pruneModel2, [w], 0.3, 1000, 50000)
    assert text == "Pruned %d of %d weights (%.3f%%)\n" % (int(600 * (0.3 * 0.8)), 600, 0.3 * 0.8)
    w = torch.nn.Parameter(torch.from_numpy(R.tie_free(np.random.default_rng(5), (20, 30))))
    _, n_below, n_nonzero = R.rule1(w.detach().numpy(), 73, 77)[2:5]
    _, text = _quiet(M.pruneModel, [w])
    assert text == "Pruned %f%% of the weights\n" % (float(n_below) / float(n_nonzero) * 100)


def test_ties_go_to_the_lowest_indices_on_cpu():
    w = R.grid_weights(3, (3, 683))
    amount = R.amount_for(w.size, R.RATIO2, R.LT, R.HT)
    want_w, want_m = R.rule2(w, amount)
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    (masks, _) = _quiet(M.pruneModel2, [p], R.RATIO2, R.LT, R.HT)
    assert np.array_equal(p.detach().numpy(), want_w) and np.array_equal(masks[0].numpy(), want_m)


def test_search_that_never_ends_is_cut_off():
    w = R.oscillating_tensor()
    out = R.rule1(w, 73, 77)
    assert out[6] == R.ST_NO_END and out[5] == R.MAX_ITER and np.array_equal(out[0], w)      # the restatement oscillates: 50 % / 100 %
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    with pytest.raises(L.RcvError, match="parameter 0"):
        _quiet(M.pruneModel, [p])
    assert np.array_equal(p.detach().numpy(), w)


def test_cpu_refusals():
    with pytest.raises(ZeroDivisionError):
        _quiet(M.pruneModel, [torch.nn.Parameter(torch.zeros(4, 4))])
    with pytest.raises(L.RcvError, match="parameter 0"):
        _quiet(M.pruneModel, [torch.nn.Parameter(torch.zeros(4, 4))])
    with pytest.raises(L.RcvError):
        _quiet(M.pruneModel, [torch.nn.Parameter(torch.ones(1, 1))])
    with pytest.raises(L.RcvError, match="amount"):
        _quiet(M.pruneModel2, [torch.nn.Parameter(torch.ones(20, 10))], 1.5, 1000, 50000)


# ---- the device entry points, without compute (the style of tests/test_lib_abi.py) ----
def _job(n=64, amount=0, w=0x1000, mask=0x2000, ratio=0.1, lower=73.0, upper=77.0):
    j = L.RcvPruneJob()
    j.w, j.mask, j.n, j.amount, j.ratio, j.lower, j.upper = w, mask, n, amount, ratio, lower, upper
    return j


def _check(jobs, rule):
    table = (L.RcvPruneJob * len(jobs))(*jobs)
    lib = L.load()
    rc = lib.rcv_prune_check(table, len(jobs), rule)
    return rc, lib.rcv_last_error().decode()


def test_job_struct_layout_matches_header():
    assert ctypes.sizeof(L.RcvPruneJob) == 8 + 8 + 8 + 8 + 8 + 8 + 4 + 4 + 4 * 8
    assert L.RcvPruneJob.result.offset == 56 and L.RcvPruneJob.thresh.offset == 52
    assert L.OP_PRUNE == 45


def test_prune_check_refuses_before_anything_runs():
    assert _check([_job(), _job(n=2)], L.PRUNE_STD_SEARCH)[0] == 0
    assert _check([_job(amount=64)], L.PRUNE_SMALLEST_K)[0] == 0
    rc, msg = _check([_job(), _job(n=64, amount=65)], L.PRUNE_SMALLEST_K)          # torch.topk's error
    assert rc == -1 and "job 1" in msg and "amount 65" in msg
    rc, msg = _check([_job(amount=-1)], L.PRUNE_SMALLEST_K)
    assert rc == -1 and "job 0" in msg
    rc, msg = _check([_job(), _job(), _job(n=1)], L.PRUNE_STD_SEARCH)               # std of one element is NaN
    assert rc == -1 and "job 2" in msg and "NaN" in msg
    assert _check([_job(n=1)], L.PRUNE_MAX_RATIO)[0] == 0
    assert _check([_job(n=0)], L.PRUNE_MAX_RATIO)[0] == -1
    assert _check([_job(n=1 << 31)], L.PRUNE_MAX_RATIO)[0] == -1
    assert _check([_job(w=0x1002)], L.PRUNE_MAX_RATIO)[0] == -1                     # 4-byte alignment is needed, no more
    assert _check([_job(w=0x1004)], L.PRUNE_MAX_RATIO)[0] == 0
    assert _check([_job(w=0)], L.PRUNE_MAX_RATIO)[0] == -1
    assert _check([_job(mask=0)], L.PRUNE_MAX_RATIO)[0] == -1
    assert _check([_job(ratio=float("nan"))], L.PRUNE_MAX_RATIO)[0] == -1
    assert _check([_job(lower=float("inf"))], L.PRUNE_STD_SEARCH)[0] == -1
    assert _check([_job()], 3)[0] == -1 and _check([_job()], -1)[0] == -1


def test_prune_needs_a_device_handle():
    h = L.planner_handle(256)
    op = L.make_op(L.OP_PRUNE, 0, count=3, aux0=L.PRUNE_SMALLEST_K)
    assert L.op_workspace(h, op) == 0
    assert L.OpList([op]).labels(h)[0] == "prune<2>"
    with pytest.raises(L.RcvError):
        L.op_workspace(h, L.make_op(L.OP_PRUNE, 0, count=3, aux0=5))
    with pytest.raises(L.RcvError):
        L.op_workspace(h, L.make_op(L.OP_PRUNE, 0, count=0, aux0=0))
    assert L.load().rcv_prune(h, 0x1000, 3, L.PRUNE_STD_SEARCH, None) == -1
    assert b"planning-only" in L.load().rcv_last_error()


def test_status_rows_become_exceptions():
    rows = (L.RcvPruneJob * 3)()
    for r in rows:
        r.result[1] = 5
    M._prune_check_rows(rows, L.PRUNE_STD_SEARCH)
    rows[2].result[3] = L.PRUNE_ST_NO_END
    with pytest.raises(L.RcvError, match="parameter 2"):
        M._prune_check_rows(rows, L.PRUNE_STD_SEARCH)
    rows[2].result[3] = L.PRUNE_ST_OK
    rows[1].result[3] = L.PRUNE_ST_ALL_ZERO                                            # the all-zero tensor of rule 1
    with pytest.raises(ZeroDivisionError, match="parameter 1"):
        M._prune_check_rows(rows, L.PRUNE_STD_SEARCH)
    with pytest.raises(L.RcvError, match="parameter 1"):
        M._prune_check_rows(rows, L.PRUNE_STD_SEARCH)
    rows[1].result[3] = L.PRUNE_ST_BAD_JOB
    with pytest.raises(L.RcvError, match="parameter 1"):
        M._prune_check_rows(rows, L.PRUNE_SMALLEST_K)


def test_sgd_mask_surface():
    from robocupvision_amd import optim
    assert hasattr(optim.SGD, "set_prune_mask")
    opt = optim.SGD(M.PB_FCN(32, 5, 1, False, 0), lr=0.1)
    opt.set_prune_mask([torch.zeros(2, 2, dtype=torch.bool)])
    assert len(opt._prune_src) == 1 and opt._prune_flat is None
    opt.set_prune_mask(None)
    assert opt._prune_src is None
