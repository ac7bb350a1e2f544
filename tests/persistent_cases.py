"""Multi-round cases of the 5x5 classifier family (csrc/conv5.hip) and of the pointwise family (csrc/conv_pw.hip): the shapes at which
a workgroup of conv5_kernel, wgrad5_kernel, pw_kernel and pw_wgrad_kernel takes its loop `for (t = blockIdx.x; t < n; t += gridDim.x)`
three times or more with a ragged last round.  No GPU import: tests/test_plan_census.py checks every row on the 256-CU planning handle,
tests/test_gpu_cls5.py and tests/test_gpu_pw.py parametrize over the tables and guard each case on the real handle.

Planned grid and work count, one function per family, -> (workgroups, work items).  The work items come from the plan query where it
reports them -- i[NPART] with the statistics forced on is the tile count of RCV_OP_PW and RCV_OP_CONV5, i[NSPLIT] the workgroups (along
x) of the two filter gradients -- and the rest is restated from the launchers' rules:
    pw tile            256 pixels, 128 with more than 64 output channels          (pw_launch: 64 * WN)
    pw / conv5 grid    min(tiles, 2 * CUs)
    pw_wgrad chunks    ceil(P / 64); rows = pw_restatement.wgrad_rows             (pw_wgrad_launch)
    5x5 tiles          N * ceil(H / R) * ceil(W / Wt), Wt = 16 if W <= 16 else 32, R = 256 / Wt   (conv5_tiling)
    wgrad5 grid        min(tiles, CUs)
"""
import pw_restatement as PR
from plan_census import copy_op, label_of
from robocupvision_amd import _lib as L

# ------------------------------------------------------------------------------------------------- 5x5 family
# (N, H, W), tile name, tiles.  11 x 121 x 161: 11 * 16 * 6 = 1056 tiles of 8x32 = 512 * 2 + 32 = 256 * 4 + 32;
# 345 x 33 x 16: 345 * 3 * 1 = 1035 tiles of 16x16 = 512 * 2 + 11 = 256 * 4 + 11
C5_PLANES = [((11, 121, 161), "8x32", 1056), ((345, 33, 16), "16x16", 1035)]
C5_CIN = (8, 16)
# (what, (N, H, W), record Cin, record Cout, (label, workgroups, work items on 256 CUs)); the data gradient of a cin-channel layer is
# the record 8 -> cin
CONV5_CASES = [(what, shape, (cin if what == "forward" else 8), (8 if what == "forward" else cin),
                ("conv5_mfma<%d,%s>" % (cin if what == "forward" else 8, tile), 512, tiles))
               for shape, tile, tiles in C5_PLANES for cin in C5_CIN for what in ("forward", "dgrad")]
WGRAD5_CASES = [(shape, cin, ("wgrad5_mfma<%d,%s>" % (cin, tile), 256, tiles)) for shape, tile, tiles in C5_PLANES for cin in C5_CIN]

# ------------------------------------------------------------------------------------------------- pointwise family
PW_BIG = (3, 300, 293)       # 263 700 pixels: 1031 tiles of 256 (the last holds 20 pixels), 4121 chunks of 64
PW_HALF = (3, 150, 293)      # 131 850 pixels: 1031 tiles of 128, 2061 chunks of 64
# (Cin, Cout, (N, H, W), (label, workgroups, tiles)): one per accumulator shape (WM blocks of 16 output channels), (24, 40) with a
# half-filled last block on both sides
PW_CASES = [(16, 8, PW_BIG, ("pw_mfma<1,4>", 512, 1031)), (16, 32, PW_BIG, ("pw_mfma<2,4>", 512, 1031)),
            (24, 40, PW_BIG, ("pw_mfma<4,4>", 512, 1031)), (32, 64, PW_BIG, ("pw_mfma<4,4>", 512, 1031)),
            (64, 128, PW_HALF, ("pw_mfma<8,2>", 512, 1031))]
# name -> (flags, load mode, statistics): the forms of the exact cases (plain loads) and of the random ones
PW_FORMS = {
    "plain": (0, L.LOAD_PLAIN, L.STATS_NONE),
    "folded": (L.F_BIAS | L.F_RELU, L.LOAD_PLAIN, L.STATS_NONE),
    "dgrad": (L.F_TRANSPOSED_SRC | L.F_RESID, L.LOAD_PLAIN, L.STATS_NONE),
    "affine_relu": (0, L.LOAD_AFFINE_RELU, L.STATS_FWD),
    "grad_dec": (L.F_TRANSPOSED_SRC | L.F_RESID, L.LOAD_GRAD_DEC, L.STATS_BWD_DEC),
}
PW_EXACT_FORMS = ("plain", "folded", "dgrad")
PW_RANDOM_CASE, PW_RANDOM_FORMS = PW_CASES[2], ("affine_relu", "grad_dec")
# (Cin, Cout, (N, H, W), (label, rows, chunks)): one per NB (filter blocks per wave) that the default cap of 4 reaches -- 1, 2, 4 --
# and 128 x 128, where the output channels are split over blockIdx.y
PW_WGRAD_CASES = [(8, 8, PW_BIG, ("pw_wgrad_mfma<1,64,1>", 1024, 4121)), (64, 32, PW_BIG, ("pw_wgrad_mfma<2,64,1>", 1024, 4121)),
                  (64, 64, PW_BIG, ("pw_wgrad_mfma<4,64,1>", 512, 4121)), (128, 128, PW_HALF, ("pw_wgrad_mfma<4,64,4>", 256, 2061))]
PW_WGRAD_RANDOM_CASE = PW_WGRAD_CASES[2]
WGRAD5_RANDOM_CASE = WGRAD5_CASES[1]
CONV5_RANDOM_CASES = (CONV5_CASES[2], CONV5_CASES[3])      # 11 x 121 x 161, 16 channels: forward and data gradient

# the reduction's loop edges (pw_reduce_kernel: 16 row lanes, four loads in flight while s + 48 < nsplit) and the forms never launched
PW_REDUCE_NSPLIT = (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1024)
PW_REDUCE_PAIRS = ((8, 8), (24, 40))
WGRAD5_REDUCE_NSPLIT = (1, 2, 255, 256)
WGRAD5_REDUCE_CLASSES = (1, 5, 8)
PW_CAP8_PAIRS = ((64, 64), (128, 64), (128, 128))


# ------------------------------------------------------------------------------------------------- records without operands
def conv5_record(case, **kw):
    what, (N, H, W), cin, cout, _ = case
    return L.make_op(L.OP_CONV5, kw.pop("flags", 0), n=N, h=H, w=W, cin=cin, cout=cout, ho=H, wo=W, stride=1, dil=1, **kw)


def wgrad5_record(case, **kw):
    (N, H, W), cin, _ = case
    return L.make_op(L.OP_WGRAD5, kw.pop("flags", L.F_BIAS), n=N, h=H, w=W, cin=cin, cout=8, ho=H, wo=W, stride=1, dil=1,
                     inmode2=L.LOAD_PLAIN, **kw)


def pw_record(case, form, **kw):
    cin, cout, (N, H, W), _ = case
    flags, mode, stats = PW_FORMS[form]
    return L.make_op(L.OP_PW, flags, n=N, h=H, w=W, cin=cin, cout=cout, inmode=mode, stats=stats, **kw)


def pw_pin(case, form):
    """The case's pin with the label of the form: the data gradient's carries ",t"."""
    label, grid, tiles = case[3]
    return (label[:-1] + ",t>" if PW_FORMS[form][0] & L.F_TRANSPOSED_SRC else label), grid, tiles


def pw_wgrad_record(case, xm=L.LOAD_PLAIN, gm=L.LOAD_PLAIN, **kw):
    cin, cout, (N, H, W), _ = case
    return L.make_op(L.OP_PW_WGRAD, 0, n=N, h=H, w=W, cin=cin, cout=cout, inmode=xm, inmode2=gm, **kw)


# ------------------------------------------------------------------------------------------------- the launchers' rules, restated
def _pixels(op):
    return op.i[L.RCV_I_N] * op.i[L.RCV_I_H] * op.i[L.RCV_I_W]


def pw_tiles(op):
    return -(-_pixels(op) // (128 if op.i[L.RCV_I_COUT] > 64 else 256))


def pw_chunks(op):
    return -(-_pixels(op) // 64)


def c5_tiles(op):
    N, H, W = op.i[L.RCV_I_N], op.i[L.RCV_I_H], op.i[L.RCV_I_W]
    wt = 16 if W <= 16 else 32
    return N * -(-H // (256 // wt)) * -(-W // wt)


def pw_cap_label(cin, cout, cap):
    """The label of an RCV_OP_PW_WGRAD record, pw_wgrad_mfma<NB,64,cosplit>, from the launcher's rule: a workgroup takes all input
    channels and as many blocks of 16 output channels as leave each of its four waves at most `cap` blocks of 16 x 16 of the filter."""
    nbx, nbg = -(-cin // 16), -(-cout // 16)
    nbw = min(max(4 * cap // nbx, 1), nbg)
    per_wave = -(-nbx * nbw // 4)
    nb = 1 if per_wave <= 1 else 2 if per_wave <= 2 else 4 if per_wave <= 4 else 8
    return "pw_wgrad_mfma<%d,64,%d>" % (nb, -(-nbg // nbw))


def _num_cus(h):
    return int(L.load().rcv_num_cus(h))


def _npart(h, op):
    """i[NPART] of a copy of the record with the statistics forced on: the tile count as the plan query reports it."""
    q = copy_op(op)
    if q.i[L.RCV_I_STATS] == L.STATS_NONE:
        q.i[L.RCV_I_STATS] = L.STATS_FWD
    q.p[L.RCV_P_PART] = None
    L.op_workspace(h, q)
    return q.i[L.RCV_I_NPART]


def _nsplit(h, op):
    q = copy_op(op)
    L.op_workspace(h, q)
    return q.i[L.RCV_I_NSPLIT]


def pw_rounds(op, h):
    tiles = _npart(h, op)
    assert tiles == pw_tiles(op), "pw: the query reports %d tiles, the restated rule %d" % (tiles, pw_tiles(op))
    return min(tiles, 2 * _num_cus(h)), tiles


def conv5_rounds(op, h):
    tiles = _npart(h, op)
    assert tiles == c5_tiles(op), "conv5: the query reports %d tiles, the restated rule %d" % (tiles, c5_tiles(op))
    return min(tiles, 2 * _num_cus(h)), tiles


def pw_wgrad_rounds(op, h):
    rows = _nsplit(h, op)
    want = PR.wgrad_rows(_pixels(op), op.i[L.RCV_I_CIN], op.i[L.RCV_I_COUT], _num_cus(h))
    assert rows == want, "pw_wgrad: the query reports %d rows, the restated rule %d" % (rows, want)
    return rows, pw_chunks(op)


def wgrad5_rounds(op, h):
    rows, tiles = _nsplit(h, op), c5_tiles(op)
    assert rows == min(tiles, _num_cus(h)), "wgrad5: the query reports %d rows, the restated rule %d" % (rows, min(tiles, _num_cus(h)))
    return rows, tiles


ROUNDS = {L.OP_PW: pw_rounds, L.OP_CONV5: conv5_rounds, L.OP_PW_WGRAD: pw_wgrad_rounds, L.OP_WGRAD5: wgrad5_rounds}


def multi_round(workgroups, items):
    """The census's rule (plan_census.multi_round): three rounds or more, the last one ragged."""
    return items > 2 * workgroups and items % workgroups != 0


def assert_multi_round(op, h, pinned):
    """The guard of a multi-round GPU case: on the handle `h` the record still loops as its table says.  pinned: (label, workgroups,
    work items) at 256 CUs."""
    cus = _num_cus(h)
    grid, items = ROUNDS[op.kind](op, h)
    label = label_of(h, copy_op(op))
    assert label == pinned[0], "planned on %s, the case was chosen for %s" % (label, pinned[0])
    assert items == pinned[2], "%s: %d work items, the table says %d" % (label, items, pinned[2])
    if cus == 256:
        assert grid == pinned[1], "%s: %d workgroups on 256 CUs, the table says %d" % (label, grid, pinned[1])
    assert multi_round(grid, items), \
        "%s on %d CUs: %d tiles over %d workgroups is no multi-round case any more -- choose a larger shape" % (label, cus, items, grid)
    return grid, items
