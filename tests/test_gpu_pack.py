"""GPU: the filter packer itself (RCV_OP_PACK, pack_kernel of csrc/small_kernels.hip) against its numpy restatement
(tests/pack_restatement.py, pinned to the torch operations by tests/test_pack.py) -- the destination buffer, not a convolution behind it.

Index maps, bit for bit, on integer-grid filters (every Winograd halving and every bf16 split exact) for every combination of
(rows_from_d1, flip, layout, scale) that engine.py emits; rounding on random filters; and one launch over a table of eight jobs, as the
engine issues it, against the same jobs packed one at a time."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pack_restatement as R      # noqa: E402
from test_pack import cases      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64
ULP = 2.0 ** -23


def _n_floats(rp, cp, layout):
    return 3 * R._ksteps(layout, rp) * cp * 16 if layout in (3, 4, 5) else (16 if layout == 2 else 4 if layout == 1 else 9) * rp * cp


def _job(rec_case, w, scale=None):
    """(D0, D1, rows_from_d1, flip, rows_pad, cols_pad, layout, w, scale) of a case of tests/test_pack.py."""
    _, rfd1, flip, layout, _, rows, cols, rp_fixed = rec_case
    rp, cp, _ = R.pack_dims(rows, cols, layout)
    D0, D1 = (cols, rows) if rfd1 else (rows, cols)
    return (D0, D1, rfd1, flip, rp_fixed or rp, cp, layout, w, scale)


def _pack_on_device(jobs, aux0=None):
    """One RCV_OP_PACK launch over `jobs`; per job the destination as float32 [taps][rows_pad][cols_pad], resp. the bf16 planes as
    float32 [3][k-steps][cols_pad][32].  Layouts 0 / 1 / 2: dst prefilled with NaN; split layouts: with zeros (engine._zeros); 64 NaN
    guard floats behind every dst must survive."""
    from robocupvision_amd import _lib as L
    h = L.handle(0)
    keep, table, dsts = [], [], []
    for (D0, D1, rfd1, flip, rp, cp, layout, w, scale) in jobs:
        n = _n_floats(rp, cp, layout)
        dst = torch.full((n + GUARD,), float("nan"), device=DEV)
        if layout in (3, 4, 5):
            dst[:n] = 0.0
        wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(DEV)
        sd = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).to(DEV) if scale is not None else None
        assert wd.numel() == D0 * D1 * 9 and (sd is None or sd.numel() >= (D0 if rfd1 else D1))
        j = L.RcvPackJob()
        j.src, j.dst, j.D0, j.D1 = wd.data_ptr(), dst.data_ptr(), D0, D1
        j.rows_from_d1, j.flip, j.rows_pad, j.cols_pad, j.merged = int(rfd1), int(flip), rp, cp, layout
        j.scale = sd.data_ptr() if sd is not None else None
        keep += [wd, sd]
        table.append(j)
        dsts.append((dst, n))
    if aux0 is None:        # as engine.py sizes the grid: the largest job
        aux0 = max((4 if jb[6] in (1, 4) else 9) * jb[4] * jb[5] for jb in jobs)
    dev_table = torch.frombuffer(bytearray(bytes((L.RcvPackJob * len(table))(*table))), dtype=torch.uint8).to(DEV)
    L.OpList([L.make_op(L.OP_PACK, 0, count=len(table), aux0=aux0, p_in=dev_table.data_ptr())]).run(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = []
    for (dst, n), jb in zip(dsts, jobs):
        rp, cp, layout = jb[4], jb[5], jb[6]
        assert bool(torch.isnan(dst[n:]).all()), "the guard floats behind dst were written (layout %d)" % layout
        if layout in (3, 4, 5):
            out.append(dst[:n].view(torch.bfloat16).float().cpu().numpy().reshape(3, R._ksteps(layout, rp), cp, 32))
        else:
            out.append(dst[:n].cpu().numpy().reshape(-1, rp, cp))
    return out


def _restated(jb, dtype):
    D0, D1, rfd1, flip, rp, cp, layout, w, scale = jb
    return R.pack(w, D0, D1, rfd1, flip, rp, cp, layout, scale=scale, dtype=dtype)


def _grid_filter(rng, D0, D1):
    """Multiples of 4 in +-64, a third of them zero."""
    w = (rng.integers(-16, 17, (D0, D1, 3, 3)) * 4).astype(np.float32)
    w[rng.random(w.shape) < 1.0 / 3.0] = 0.0
    return w


def _pow2_scale(rng, n):
    return (np.float32(2.0) ** rng.integers(-3, 4, n).astype(np.float32) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


GROUPS = sorted({(c[0], c[3], c[4]) for c in cases()})


@pytest.mark.parametrize("rec,layout,scaled", GROUPS)
def test_index_maps_bit_for_bit(rec, layout, scaled):
    """Integer-grid filters (multiples of 4 in +-64, a third zero) and scales +-2^k: both Winograd halvings and the bf16 split are
    exact, so every float of dst equals pack(..., dtype=float32) -- every element written (NaN prefill, layouts 0 / 1 / 2), every pad
    zero, the guard untouched -- for every combination and channel pair of tests/test_pack.py, one job per launch."""
    rng = np.random.default_rng(300 + 11 * layout + scaled)
    n = 0
    for c in cases():
        if (c[0], c[3], c[4]) != (rec, layout, scaled):
            continue
        rows, cols = c[5], c[6]
        D0, D1 = (cols, rows) if c[1] else (rows, cols)
        jb = _job(c, _grid_filter(rng, D0, D1), _pow2_scale(rng, cols) if scaled else None)
        got, = _pack_on_device([jb])
        want = _restated(jb, np.float32)
        assert got.shape == want.shape, (c, got.shape, want.shape)
        assert np.array_equal(got, want), (c, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        n += 1
    assert n > 0


@pytest.mark.parametrize("rec,layout,scaled", GROUPS)
def test_rounding_on_random_filters(rec, layout, scaled):
    """Random filters and scales in +-[0.25, 4].  Layouts 0 / 1: bitwise float32(src), resp. the one IEEE product float32(src * scale).
    Layouts 3 / 4 / 5 without a scale: the three planes bitwise the restatement's (the split is exact); with a scale h + m + l in
    float64 within 2^-23 |src * scale| of the float64 product (one fp32 rounding, times 2: the compiler may contract the multiply into
    the first remainder, so the planes are not pinned one by one; a lost low term is 2^-17).  Layout 2: every U entry within
    4 * 2^-23 * (|G| |scale * g| |G|^T) of the float64 restatement (five fp32 roundings on partial sums bounded by the absolute-value
    transform).
    Measured (MI355X, largest over the channel pairs): every bitwise comparison exact; layouts 3 / 4 / 5 with a scale
    0.50 x 2^-23 |src * scale| (the product rounded once to fp32, then split exactly); layout 2 1.08 (conv forward), 1.14 (scaled) and
    1.02 (flipped) x 2^-23 (|G| |scale * g| |G|^T)."""
    rng = np.random.default_rng(400 + 11 * layout + scaled)
    worst = 0.0
    for c in cases():
        if (c[0], c[3], c[4]) != (rec, layout, scaled):
            continue
        rows, cols = c[5], c[6]
        D0, D1 = (cols, rows) if c[1] else (rows, cols)
        w = (rng.standard_normal((D0, D1, 3, 3)) * 0.1).astype(np.float32)
        scale = (rng.uniform(0.25, 4.0, cols) * rng.choice([-1.0, 1.0], cols)).astype(np.float32) if scaled else None
        jb = _job(c, w, scale)
        rp, cp = jb[4], jb[5]
        got, = _pack_on_device([jb])
        if layout in (0, 1) or (layout in (3, 4, 5) and not scaled):
            want = _restated(jb, np.float32)
            assert np.array_equal(got, want), (c, int((got != want).sum()))
            continue
        exact = _restated(jb, np.float64)
        if layout == 2:
            A = np.abs(R.G)
            nine = R.pack(np.abs(w), D0, D1, c[1], c[2], rp, cp, 0, scale=None if scale is None else np.abs(scale), dtype=np.float64)
            bound = np.einsum("ai,ijrc,bj->abrc", A, nine.reshape(3, 3, rp, cp), A).reshape(16, rp, cp)
            err = np.abs(got.astype(np.float64) - exact)
            ok = err <= 4 * ULP * bound
        else:
            assert np.array_equal(R.bf16_rne(got), got)
            value = R.decode_split(exact, layout, rp, cp)          # src * scale in float64, [taps][rows_pad][cols_pad]
            err = np.abs(R.decode_split(got, layout, rp, cp) - value)
            bound = np.abs(value)
            ok = err <= ULP * bound
            # outside the k-index map (beyond the last tap) the planes stay as they were: zero
            ks, kp = R._k_index(layout, 4 if layout == 4 else 9, rp)
            mapped = np.zeros(got.shape[1:], bool)
            mapped[ks[:, :, None], np.arange(cp)[None, None, :], kp[:, :, None]] = True
            assert not got[:, ~mapped].any(), c
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) / ULP)
        assert ok.all(), (c, float((err / np.maximum(bound, 1e-300)).max()) / ULP)
    print(".pack %s layout %d%s: worst error %.3f x 2^-23 x bound" % (rec, layout, " scaled" if scaled else "", worst))


def _table_jobs(rng):
    """Eight jobs of different sizes: layouts 0, 1, 2, 3, 4 and 5 all present, two flipped, two scaled."""
    def job(rfd1, flip, layout, rows, cols, scaled=False, rp_fixed=None):
        D0, D1 = (cols, rows) if rfd1 else (rows, cols)
        w = (rng.standard_normal((D0, D1, 3, 3)) * 0.1).astype(np.float32)
        scale = (rng.uniform(0.25, 4.0, cols) * rng.choice([-1.0, 1.0], cols)).astype(np.float32) if scaled else None
        return _job((None, rfd1, flip, layout, scaled, rows, cols, rp_fixed), w, scale)
    return [job(1, 0, 0, 24, 40, scaled=True), job(0, 0, 1, 32, 16), job(0, 1, 2, 64, 64), job(1, 0, 3, 128, 64),
            job(0, 0, 4, 16, 16, scaled=True), job(1, 0, 5, 32, 64), job(0, 1, 0, 3, 16, rp_fixed=R.CLS_ROWS_PAD), job(1, 0, 0, 3, 8)]


@pytest.mark.parametrize("aux0", ["largest", 1])
def test_a_table_of_several_jobs(aux0):
    """One RCV_OP_PACK over eight jobs (blockIdx.y), as the engine launches it once per forward: every dst bitwise the same job packed
    alone.  i[AUX0] = the largest job, and 1 -- one workgroup per job, whose grid-stride loop must still cover every element."""
    jobs = _table_jobs(np.random.default_rng(9))
    assert {jb[6] for jb in jobs} == {0, 1, 2, 3, 4, 5} and sum(jb[3] for jb in jobs) == 2 and sum(jb[8] is not None for jb in jobs) == 2
    largest = max((4 if jb[6] in (1, 4) else 9) * jb[4] * jb[5] for jb in jobs)
    together = _pack_on_device(jobs, aux0=largest if aux0 == "largest" else 1)
    for k, jb in enumerate(jobs):
        alone, = _pack_on_device([jb])
        assert np.array_equal(together[k], alone), (k, jb[:7], int((together[k] != alone).sum()))
        if jb[6] in (0, 1):
            assert np.array_equal(alone, _restated(jb, np.float32)), (k, jb[:7])
