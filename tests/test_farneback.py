"""No GPU: pins the optical-flow contract (tests/farneback_restatement.py).  Each stage of the restatement against an
independent computation (numpy.linalg.lstsq, scipy.ndimage), the level rule, recovery of known whole-pixel motion, hand-written answers
of the label remap, the gray conversion in Python integers, and the library's plan-time refusals (which need no device)."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

import farneback_restatement as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_farneback as G  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "farneback.json")) as _f:
    GOLDEN = json.load(_f)


# ---- stages ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,sigma", [(7, 1.5), (5, 1.1)])
def test_poly_exp_is_the_weighted_least_squares_fit(n, sigma):
    rng = np.random.default_rng(3)
    img = np.rint(F.texture(rng, 40, 44, 0)).astype(np.uint8)
    R = F.poly_exp(img, n, sigma, np.float64)
    g = F.poly_taps(n, sigma)[0]
    i = np.arange(-n, n + 1, dtype=np.float64)
    jj, ii = np.meshgrid(i, i, indexing="ij")
    sw = np.sqrt(np.outer(g, g)).ravel()
    A = np.stack([np.ones_like(ii), ii, jj, ii * ii, jj * jj, ii * jj], -1).reshape(-1, 6) * sw[:, None]
    for y, x in [(n, n), (20, 22), (40 - n - 1, 44 - n - 1), (13, 30), (25, n)]:      # interior: the window lies inside the plane
        patch = img[y - n:y + n + 1, x - n:x + n + 1].astype(np.float64).ravel()
        c = np.linalg.lstsq(A, patch * sw, rcond=None)[0]
        assert np.abs(R[:, y, x] - c[1:]).max() <= 1e-9, (y, x, R[:, y, x], c)


def test_normal_matrix_rows_are_sparse_as_used():
    gi = np.linalg.inv(F.normal_matrix(7, 1.5))
    used = np.zeros((6, 6), bool)
    used[1, 1] = used[2, 2] = used[5, 5] = True
    used[3, [0, 3, 4]] = used[4, [0, 3, 4]] = True
    assert np.abs(gi[1:][~used[1:]]).max() < 1e-12


@pytest.mark.parametrize("winsize", [15, 9, 1])
def test_box_mean_is_scipys_uniform_filter(winsize):
    M = np.random.default_rng(4).standard_normal((5, 23, 31))
    ref = np.stack([ndi.uniform_filter(m, winsize, mode="nearest") for m in M])
    assert np.abs(F.box_mean(M, winsize, np.float64) - ref).max() < 1e-12
    small = np.random.default_rng(5).standard_normal((5, 9, 11))         # windows larger than the plane
    ref = np.stack([ndi.uniform_filter(m, winsize, mode="nearest") for m in small])
    assert np.abs(F.box_mean(small, winsize, np.float64) - ref).max() < 1e-12


def test_warp_is_map_coordinates_where_in_bounds():
    rng = np.random.default_rng(6)
    R1 = rng.standard_normal((5, 30, 37))
    fy = rng.uniform(-3, 33, (30, 37))
    fx = rng.uniform(-3, 40, (30, 37))
    got, ok = F.warp(R1, fx, fy, np.float64)
    assert 0.5 < ok.mean() < 0.95
    assert (ok == ((fx >= 0) & (fx < 36) & (fy >= 0) & (fy < 29))).all()
    for c in range(5):
        ref = ndi.map_coordinates(R1[c], [fy, fx], order=1)
        assert np.abs(got[c] - ref)[ok].max() < 1e-12


def test_blur_and_resize():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (37, 41)).astype(np.uint8)
    # plane 0: [1/4, 1/2, 1/4] with reflect-101 borders (scipy calls them 'mirror'), no resize
    ref = ndi.correlate1d(ndi.correlate1d(img.astype(np.float64), [.25, .5, .25], 1, mode="mirror"), [.25, .5, .25], 0, mode="mirror")
    assert np.abs(F.plane_image(img, 0, np.float64) - ref).max() < 1e-12
    assert list(np.round(F.blur_taps(1), 6)) == [0.106507, 0.786986, 0.106507] and len(F.blur_taps(2)) == 9
    # halving an even axis averages neighbours; the pixel-centre rule clamps at the ends of an odd one
    a = np.arange(8, dtype=np.float64)[None].repeat(2, 0)
    assert np.allclose(F.resize(a, 2, 4, np.float64), [[.5, 2.5, 4.5, 6.5]] * 2)
    assert np.allclose(F.resize(np.array([[0., 3., 6.]]), 1, 6, np.float64), [[0, .75, 2.25, 3.75, 5.25, 6]])


def test_border_scale_is_the_product_of_both_edges():
    s = F.border_scale(9, 30, np.float64)
    w = {0: .14, 1: .14, 2: .4472, 3: .4472, 4: .4472}
    for y in range(9):
        for x in (0, 1, 2, 4, 5, 15, 24, 25, 29):
            want = w.get(x, 1) * w.get(29 - x, 1) * w.get(y, 1) * w.get(8 - y, 1)
            assert abs(s[y, x] - want) < 1e-15
    assert F.border_scale(40, 40, np.float64)[5:35, 5:35].min() == 1.0


def test_level_rule():
    assert F.n_coarse(120, 160, 2) == 1 and F.plane_size(120, 160, 1) == (60, 80)
    assert F.n_coarse(64, 64, 2) == 1
    assert F.n_coarse(48, 64, 2) == 0
    assert F.n_coarse(128, 132, 3) == 2 and F.plane_size(128, 132, 2) == (32, 33)
    assert F.n_coarse(120, 160, 0) == 0
    assert F.plane_size(67, 71, 1) == (34, 36)          # 33.5 and 35.5 round to even


# ---- ground truth --------------------------------------------------------------------------------------------------------------------
def _truth(H, W, d):
    med, acc = G.ground_truth_figures(H, W, d)
    rec = GOLDEN["ground_truth"]["%dx%d_%d_%d" % (H, W, d[0], d[1])]
    print("%dx%d d=%s: median interior error %.5f px (recorded %.5f), label accuracy %.5f (recorded %.5f)"
          % (H, W, d, med, rec["median_interior_error"], acc, rec["label_interior_accuracy"]))
    assert med <= 0.01 and acc >= 0.999
    assert abs(med - rec["median_interior_error"]) < 1e-4 and abs(acc - rec["label_interior_accuracy"]) < 1e-3


@pytest.mark.parametrize("d", G.SHIFTS, ids=str)
@pytest.mark.parametrize("H,W", G.TWO_PLANE)
def test_known_motion_two_planes(H, W, d):
    _truth(H, W, d)


@pytest.mark.parametrize("H,W", G.ONE_PLANE)
def test_known_motion_one_plane(H, W):
    _truth(H, W, (1, 1))


def test_float32_run_is_close_and_moves_no_label():
    p, q, lp, lq = G.ground_truth_scene(64, 64, (3, -2))
    f64, f32 = F.farneback_flow(p, q), F.farneback_flow(p, q, dtype=np.float32)
    assert np.abs(f64 - f32).max() < 1e-4
    assert (F.update_labels(lq, f64) == F.update_labels(lq, f32)).all()
    assert GOLDEN["sequences"]["float32_vs_float64_pixels"] == 0


def test_restatement_refuses_what_the_contract_excludes():
    z = np.zeros((40, 40), np.uint8)
    for kw in (dict(flags=256), dict(pyr_scale=0.8), dict(winsize=14), dict(poly_n=6)):
        with pytest.raises(ValueError):
            F.farneback_flow(z, z, **kw)


# ---- labels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_update_labels_known_answers(dtype):
    lab = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], dtype=dtype)
    flow = np.zeros((2, 3, 4), np.float32)
    assert (F.update_labels(lab, flow) == lab).all() and F.update_labels(lab, flow).dtype == dtype
    flow[0] = 1                      # take the right-hand neighbour; past the edge -> 0
    assert F.update_labels(lab, flow).tolist() == [[2, 3, 4, 0], [6, 7, 8, 0], [10, 11, 12, 0]]
    flow[0], flow[1] = 0, -1         # the pixel above; negative source row -> 0
    assert F.update_labels(lab, flow).tolist() == [[0, 0, 0, 0], [1, 2, 3, 4], [5, 6, 7, 8]]
    flow[0], flow[1] = 0.5, 0        # ties go to the even column: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 (outside)
    assert F.update_labels(lab, flow).tolist() == [[1, 3, 3, 0], [5, 7, 7, 0], [9, 11, 11, 0]]
    flow[0], flow[1] = -0.5, 0.5     # columns -0.5 -> -0 (inside), 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; rows 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert F.update_labels(lab, flow).tolist() == [[1, 1, 3, 3], [9, 9, 11, 11], [9, 9, 11, 11]]
    flow[0], flow[1] = -0.51, 0      # just past the tie: column -0.51 -> -1 (outside)
    assert F.update_labels(lab, flow)[:, 0].tolist() == [0, 0, 0]
    flow[0] = np.nan
    assert (F.update_labels(lab, flow) == 0).all()
    if dtype == np.int64:
        big = lab.astype(np.int64) * (1 << 40)
        flow[0], flow[1] = 1, 0
        assert F.update_labels(big, flow)[0].tolist() == [2 << 40, 3 << 40, 4 << 40, 0]


def test_rgb_to_gray_in_python_integers():
    corners = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    sample = np.random.default_rng(8).integers(0, 256, (500, 3)).tolist()
    px = np.array(corners + [tuple(s) for s in sample], dtype=np.uint8)
    want = [(4899 * int(r) + 9617 * int(g) + 1868 * int(b) + 8192) >> 14 for r, g, b in px.tolist()]
    assert F.rgb_to_gray(px).tolist() == want and F.rgb_to_gray(px).dtype == np.uint8
    assert want[0] == 0 and want[7] == 255


def test_propagate_labels_is_the_reference_loop():
    pred, gray = F.sequences()
    out = F.propagate_labels(pred[0], gray[0])
    assert (out[0] == F.update_labels(pred[0, 1], F.farneback_flow(gray[0, 0], gray[0, 1]))).all()
    assert (out[2] == F.update_labels(out[1], F.farneback_flow(gray[0, 2], gray[0, 1]))).all()
    with pytest.raises(ValueError):
        F.propagate_labels(pred[0, :1], gray[0, :1])


# ---- the library's plan-time refusals (no device: the planning handle checks the record) ------------------------------------------------
REFUSALS = [(dict(flags=256), "flags 256"), (dict(flags=4), "flags 4"), (dict(pyr_scale=0.8), "pyr_scale 0.8"), (dict(winsize=14), "winsize 14"),
            (dict(winsize=17), "winsize 17"), (dict(poly_n=6), "poly_n 6"), (dict(poly_n=9), "poly_n 9"), (dict(levels=-1), "levels -1"),
            (dict(iterations=0), "iterations 0"), (dict(poly_sigma=0.0), "poly_sigma 0")]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[m for _, m in REFUSALS])
def test_record_refusals(kw, msg):
    import torch
    from robocupvision_amd import _lib as L
    from robocupvision_amd import flow as FL
    z = torch.zeros(1, 40, 48, dtype=torch.uint8)
    with pytest.raises(L.RcvError, match="farneback: .*" + msg):
        FL.farneback_flow(z, z, **kw)


def test_record_workspace_and_surface():
    import torch
    import robocupvision_amd
    from robocupvision_amd import _lib as L
    from robocupvision_amd import flow as FL
    h = L.planner_handle()
    one = FL.FlowRecord(1, 120, 160).workspace_bytes(h)
    # img 2 + R 10 + M 2 x 5 floats per pixel and pair on both planes, the coarse plane's flow 2: 22 x 19200 + 24 x 4800 floats
    assert one == 4 * (22 * 19200 + 24 * 4800)
    assert FL.FlowRecord(64, 120, 160).workspace_bytes(h) == 64 * one
    with pytest.raises(L.RcvError, match="does not fit"):
        FL.FlowRecord(32767, 8192, 8192).workspace_bytes(h)
    with pytest.raises(L.RcvError, match="bytes per pixel"):
        FL.FlowRecord(1, 40, 40, channels=2).workspace_bytes(h)
    with pytest.raises(L.RcvError, match="element size"):
        L.op_workspace(h, L.make_op(L.OP_REMAP_LABELS, n=1, h=4, w=4, inmode=4))
    assert L.OpList([FL.FlowRecord(1, 120, 160, 3).op, L.make_op(L.OP_REMAP_LABELS, n=1, h=4, w=4, inmode=8)]).labels(h) == \
        ["farneback<rgb,n7,2pl>", "remap_labels<i64>"]
    for name in ("farneback_flow", "update_labels", "propagate_labels", "rgb_to_gray", "optFlow", "updateLabels"):
        assert getattr(robocupvision_amd, name) is getattr(FL, name)
    rgb = torch.tensor([[0, 0, 0], [255, 255, 255], [255, 0, 0], [12, 200, 77]], dtype=torch.uint8)
    assert FL.rgb_to_gray(rgb).tolist() == F.rgb_to_gray(rgb.numpy()).tolist()
    with pytest.raises(L.RcvError, match="no CPU path"):
        FL.farneback_flow(torch.zeros(40, 40, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.uint8))
    with pytest.raises(L.RcvError, match="no CPU path"):
        FL.update_labels(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4))
