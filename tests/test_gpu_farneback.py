"""GPU: RCV_OP_FARNEBACK / RCV_OP_REMAP_LABELS (csrc/flow.hip) against the float64 restatement of the contract
(tests/farneback_restatement.py).  Flow: within 8 x e32 per case, e32 = the restatement's own float32-vs-float64 deviation on that case
(tests/golden/farneback.json, made on the CPU by tests/golden/make_golden_farneback.py).  Bitwise: runs, batch position, RGB input, the
label remap, the chain of propagate_labels and the named entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import farneback_restatement as F
import robocupvision_amd
from robocupvision_amd import _lib as L
from robocupvision_amd import flow as FL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "farneback.json")) as _f:
    GOLDEN = json.load(_f)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _flow(p, q, **params):
    f = FL.farneback_flow(_dev(p), _dev(q), **params)
    torch.cuda.synchronize()
    return f


@pytest.mark.parametrize("name", list(F.GPU_CASES))
def test_flow_vs_float64_restatement(name):
    p, q, params = F.gpu_case(name)
    rec = GOLDEN["gpu_cases"][name]
    got = _flow(p, q, **params).cpu().numpy()
    assert got.shape == (p.shape[0], 2) + p.shape[1:] and got.dtype == np.float32
    ref = np.stack([F.farneback_flow(p[b], q[b], **params) for b in range(p.shape[0])])
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: device vs float64 %.3e px, e32 %.3e, bound %.3e, max |flow| %.2f" % (name, err, rec["e32"], 8 * rec["e32"], rec["max_abs_flow"]))
    assert np.isfinite(got).all()
    if name.startswith("noise"):
        assert rec["warps_out_of_plane"] > 500 and rec["max_abs_flow"] > 5       # the out-of-plane branch of the warp is taken
    assert err <= 8 * rec["e32"], "device vs float64 restatement %.3e px > 8 x e32 = %.3e" % (err, 8 * rec["e32"])


def test_bitwise_runs_batch_position_and_rgb():
    p, q, _ = F.gpu_case("120x160_b2")
    rng = np.random.default_rng(5)
    a = _flow(p[:1], q[:1])
    assert torch.equal(a, _flow(p[:1], q[:1]))
    # the same pair at positions 0 and 2 of a batch of three
    p3, q3 = np.stack([p[0], p[1], p[0]]), np.stack([q[0], q[1], q[0]])
    f3 = _flow(p3, q3)
    assert torch.equal(f3[0], f3[2]) and torch.equal(f3[0], a[0])
    # RGB frames: gray is formed on load
    rgb_p, rgb_q = rng.integers(0, 256, (2, 67, 71, 3)).astype(np.uint8), rng.integers(0, 256, (2, 67, 71, 3)).astype(np.uint8)
    from_rgb = _flow(rgb_p, rgb_q)
    from_gray = _flow(F.rgb_to_gray(rgb_p), F.rgb_to_gray(rgb_q))
    assert torch.equal(from_rgb, from_gray)
    assert torch.equal(FL.rgb_to_gray(_dev(rgb_p)).cpu(), torch.from_numpy(F.rgb_to_gray(rgb_p)))
    # unbatched planes and the reference's names
    one = FL.optFlow(_dev(p[0]), _dev(q[0]))
    assert one.shape == (2, 120, 160) and torch.equal(one, a[0])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_update_labels_bitwise(dtype):
    rng = np.random.default_rng(6)
    p, q, _ = F.gpu_case("120x160_b2")
    flow = _flow(p, q)                                   # the device's own flow goes to both
    lab = rng.integers(0, 5, (2, 120, 160))
    if dtype == torch.int64:
        lab[0, :3, :3] = [[-1, 1 << 40, 255], [300, -(1 << 50), 7], [0, 1, 2]]
    lab_t = torch.from_numpy(lab).to(dtype)
    got = FL.update_labels(lab_t.to(DEV), flow)
    assert got.dtype == dtype and got.shape == lab_t.shape
    fl = flow.cpu().numpy()
    ref = np.stack([F.update_labels(lab_t[b].numpy(), fl[b]) for b in range(2)])
    assert (got.cpu().numpy() == ref).all() and (ref != lab_t.numpy()).any()
    # hand-built flows: exact .5 ties, sources left / right / above / below the plane, NaN and infinities
    H, W = 13, 21
    lab = torch.from_numpy(rng.integers(1, 5, (4, H, W))).to(dtype)
    fl = np.zeros((4, 2, H, W), np.float32)
    fl[0, 0], fl[0, 1] = 0.5, -0.5
    fl[1, 0], fl[1, 1] = -1.5, 2.5
    fl[2] = rng.integers(-60, 61, (2, H, W)) * 0.5
    fl[3] = rng.uniform(-4, 4, (2, H, W))
    fl[3, 0, 0, :4] = [np.nan, np.inf, -np.inf, 3e9]
    fl[3, 1, 1, :2] = [np.nan, -3e9]
    got = FL.update_labels(lab.to(DEV), _dev(fl)).cpu().numpy()
    ref = np.stack([F.update_labels(lab[b].numpy(), fl[b]) for b in range(4)])
    assert (got == ref).all()
    assert (ref[2] == 0).any() and (ref[2] != 0).any()
    # the reference's name: [H, W] in, int64 out
    one = FL.updateLabels(lab[3].to(DEV), _dev(fl[3]))
    assert one.dtype == torch.int64 and (one.cpu().numpy() == ref[3]).all()


def test_propagate_labels():
    pred, gray = F.sequences()                           # S = 2, T = 3, 64 x 64
    S, T = pred.shape[:2]
    pd, gd = _dev(pred), _dev(gray)
    out = FL.propagate_labels(pd, gd)
    assert out.shape == pd.shape and out.dtype == torch.uint8
    want = np.stack([F.propagate_labels(pred[s], gray[s]) for s in range(S)])
    for s in range(S):
        # the chain of single device calls, bit for bit
        cur = FL.update_labels(pd[s, 1], FL.farneback_flow(gd[s, 0], gd[s, 1]))
        assert torch.equal(out[s, 0], cur)
        for i in range(1, T):
            cur = FL.update_labels(cur, FL.farneback_flow(gd[s, i], gd[s, i - 1]))
            assert torch.equal(out[s, i], cur)
        assert torch.equal(FL.propagate_labels(pd[s], gd[s]), out[s])
    differ = float((out.cpu().numpy() != want).mean())
    print("propagate_labels: %.5f of the pixels differ from the float64 restatement's chain" % differ)
    assert GOLDEN["sequences"]["float32_vs_float64_pixels"] == 0 and GOLDEN["sequences"]["shape"] == list(pred.shape)
    assert differ <= 0.001
    assert (want[:, :, 16:48, 16:48] == pred[:, :, 16:48, 16:48]).mean() > 0.99      # the moved labels land on each frame's own
    # int64 class maps (what predict returns) and RGB frames
    rgb = np.repeat(gray[..., None], 3, -1)
    assert torch.equal(FL.propagate_labels(pd.long(), _dev(rgb)).to(torch.uint8), out)


def test_refusals_launch_nothing():
    z = torch.zeros(1, 40, 48, dtype=torch.uint8, device=DEV)
    for kw, msg in [(dict(flags=256), "flags 256"), (dict(pyr_scale=0.8), "pyr_scale 0.8"), (dict(winsize=14), "winsize 14"),
                    (dict(poly_n=6), "poly_n 6"), (dict(levels=9), "levels 9"), (dict(iterations=0), "iterations 0")]:
        with pytest.raises(L.RcvError, match="farneback: .*" + msg):
            FL.farneback_flow(z, z, **kw)
    with pytest.raises(L.RcvError, match="dtype"):
        FL.update_labels(torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV), torch.zeros(1, 2, 4, 4, device=DEV))
    torch.cuda.synchronize()


def test_named_entry_points():
    p, q, _ = F.gpu_case("67x71")
    pd, qd = _dev(p), _dev(q)
    lib, h = L.load(), L.handle(0)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, W = p.shape
    need = FL.FlowRecord(B, H, W).workspace_bytes(h)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    flow = torch.empty(B, 2, H, W, device=DEV)
    args = (h, pd.data_ptr(), qd.data_ptr(), 1, B, H, W, 0.5, 2, 15, 2, 7, 1.5, 0, flow.data_ptr(), ws.data_ptr())
    L.check(lib.rcv_farneback_flow(*args, need, s), "rcv_farneback_flow")
    assert torch.equal(flow, FL.farneback_flow(pd, qd))
    assert lib.rcv_farneback_flow(*args, need - 256, s) != 0 and b"workspace" in lib.rcv_last_error()
    lab = torch.randint(0, 5, (B, H, W), dtype=torch.uint8, device=DEV)
    out = torch.empty_like(lab)
    L.check(lib.rcv_update_labels(h, lab.data_ptr(), 1, flow.data_ptr(), B, H, W, out.data_ptr(), s), "rcv_update_labels")
    assert torch.equal(out, FL.update_labels(lab, flow))
    assert lib.rcv_update_labels(h, lab.data_ptr(), 1, flow.data_ptr(), B, H, W, lab.data_ptr(), s) != 0
    torch.cuda.synchronize()
