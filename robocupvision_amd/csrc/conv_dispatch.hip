// Dispatch of the conv / transposed-conv and filter-gradient records (host code only): shape validation, the plan cache, the kernel
// arguments, and ONE table of kernel families per record kind.  A family is a row (ConvFamily / WgradFamily) defined next to its
// kernels; the order of the rows is the precedence, for the planner and for the filter packer alike.
#include "conv_common.h"
#include "wgrad_common.h"

static const ConvFamily* const kConvFamilies[] = {&kConvnBf3, &kConvBf3, &kConvWino, &kConvFirst, &kConvNarrow, &kConvSmall, &kConvMfma, &kConvDma};
static const WgradFamily* const kWgradFamilies[] = {&kWgradFirst, &kWgradBf3, &kWgradnBf3, &kWgradMfma};
static_assert(sizeof(kConvFamilies) / sizeof(kConvFamilies[0]) == CONV_NUM_FAMILIES && sizeof(kWgradFamilies) / sizeof(kWgradFamilies[0]) == WGRAD_NUM_FAMILIES,
              "one row per CONV_* / WGRAD_* value, in the order of the enum");

// a filter packed in layout 2 (Winograd) or 3..5 (split-bf16) is read by the rows that name the layout and by no other
static const char kWinoRefusal[] = "conv: a filter packed in the Winograd layout needs stride 1 / dilation 1";
static const char kBf3Refusal[] = "conv: a filter packed in a split-bf16 layout needs a record one of the split-bf16 kernels runs";

static int conv_plan(const rcv_handle* h, const rcv_op* op, ConvPlan* pl) {
  const bool transposed = op->kind == RCV_OP_TCONV;
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], Cin = op->i[RCV_I_CIN], Cout = op->i[RCV_I_COUT];
  const int Ho = op->i[RCV_I_HO], Wo = op->i[RCV_I_WO], s = op->i[RCV_I_STRIDE], d = op->i[RCV_I_DIL];
  RCV_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv: empty shape N=%d H=%d W=%d Cin=%d Cout=%d", N, H, W, Cin, Cout);
  RCV_CHECK_ARG(Cout % 4 == 0, "conv: Cout=%d must be a multiple of 4", Cout);
  if (op->i[RCV_I_INMODE] == RCV_LOAD_NCHW) RCV_CHECK_ARG(Cin <= 4, "conv: NCHW input supports Cin<=4 (got %d)", Cin);
  else RCV_CHECK_ARG(Cin % 4 == 0, "conv: Cin=%d must be a multiple of 4 for NHWC operands", Cin);
  int kind = KIND_GATHER;
  if (transposed) {
    RCV_CHECK_ARG(Ho == 2 * H && Wo == 2 * W, "tconv: output must be 2x input (%dx%d -> %dx%d)", H, W, Ho, Wo);
    kind = op->i[RCV_I_AUX0] ? KIND_TMERGED : KIND_TPHASE;     // AUX0 = 1 (or 4: split-bf16): filter is packed in the merged layout
    RCV_CHECK_ARG(kind == KIND_TPHASE || 4 * Cout <= 128, "tconv: merged layout needs Cout <= 32 (got %d)", Cout);
  } else {
    RCV_CHECK_ARG((s == 1 || s == 2) && (d == 1 || d == 2), "conv: stride %d dilation %d unsupported", s, d);
    RCV_CHECK_ARG(Ho == (H - 1) / s + 1 && Wo == (W - 1) / s + 1, "conv: bad output size %dx%d for input %dx%d stride %d", Ho, Wo, H, W, s);
  }
  const int aux = op->i[RCV_I_AUX0];
  const int packed = ((aux >= 3 && aux <= 5) || (aux == 2 && !transposed)) ? aux : 0;     // (a transposed conv has no Winograd layout: 2 is "merged")
  int last = CONV_NUM_FAMILIES - 1;     // a packed filter: the walk ends at the last row that reads its layout
  if (packed) while (last >= 0 && !(kConvFamilies[last]->layouts >> packed & 1)) --last;
  for (int f = 0; f <= last; ++f)
    if (kConvFamilies[f]->supported && kConvFamilies[f]->supported(h, op, kind)) return kConvFamilies[f]->plan(h, op, kind, pl);
  rcv_set_error("%s", packed == 2 ? kWinoRefusal : (packed ? kBf3Refusal : "conv: no kernel family takes the record"));
  return RCV_E_ARG;
}

int rcv_launch_conv(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  ConvPlan pl;
  if (!rcv_plan_get(h, op, &pl)) {
    memset(&pl, 0, sizeof(pl));
    const int rc = conv_plan(h, op, &pl);
    if (rc) return rc;
    pl.dev = h->device;
    rcv_plan_put(h, op, pl);
  }
  const ConvFamily& fam = *kConvFamilies[pl.path];
  if (query) {
    fam.label(pl, op, query->label, sizeof(query->label));
    query->n_part = op->i[RCV_I_STATS] != RCV_STATS_NONE ? pl.n_part : 0;
    query->part_bytes = (size_t)query->n_part * 2 * op->i[RCV_I_COUT] * sizeof(float);
    return RCV_OK;
  }
  ConvArgs a;
  a.in = (const float*)op->p[RCV_P_IN]; a.in_aux = (const float*)op->p[RCV_P_IN_AUX]; a.in_c = (const float*)op->p[RCV_P_IN_C];
  a.w = (const float*)op->p[RCV_P_W]; a.bias = (const float*)op->p[RCV_P_BIAS]; a.out = (float*)op->p[RCV_P_OUT];
  a.resid = (const float*)op->p[RCV_P_RESID]; a.epi_aux = (const float*)op->p[RCV_P_EPI_AUX]; a.epi_c = (const float*)op->p[RCV_P_EPI_C];
  a.part = (float*)op->p[RCV_P_PART];
  a.N = op->i[RCV_I_N]; a.H = op->i[RCV_I_H]; a.W = op->i[RCV_I_W]; a.Ho = op->i[RCV_I_HO]; a.Wo = op->i[RCV_I_WO];
  a.Cin = op->i[RCV_I_CIN]; a.Cout = op->i[RCV_I_COUT]; a.CinP = round_up(a.Cin, 4); a.CoutP = pl.CoutP; a.CoutV = pl.CoutV;
  a.stride = op->i[RCV_I_STRIDE]; a.dil = op->i[RCV_I_DIL];
  a.R = pl.R; a.Wt = pl.Wt; a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y; a.IH = pl.IH; a.IW = pl.IW;
  a.n_pix_tiles = a.N * pl.tiles_x * pl.tiles_y; a.n_co_tiles = pl.n_co_tiles; a.n_sub = pl.n_co_tiles * (pl.kind == KIND_TALL ? 1 : pl.n_phases);
  a.total_tiles = pl.total_tiles; a.nchunks = a.CinP / pl.CK;      // (conv_bf3: CK = 32, Cin % 32 == 0)
  a.in_mode = op->i[RCV_I_INMODE]; a.stats = op->i[RCV_I_STATS]; a.flags = op->flags;
  a.wl_floats = pl.wl_floats; a.xl_floats = pl.xl_floats; a.xk = pl.xk;
  a.xpitch = conv_xpitch(pl.xpitch_ck, pl.kind == KIND_GATHER ? a.stride : 1);
  a.fdWt = make_fastdiv(pl.Wt); a.fdIW = make_fastdiv(pl.IW); a.fdTX = make_fastdiv(pl.tiles_x); a.fdTY = make_fastdiv(pl.tiles_y);
  const uint32_t hints = rcv_stream_hints(h, op);
  a.nt_out = (hints & RCV_F_STREAM_OUT) ? 1 : 0; a.nt_pw = (hints & RCV_F_STREAM_PW) ? 1 : 0;
#ifdef RCV_STAMPS
  a.stamps = (unsigned long long*)op->p[RCV_P_X5];
#endif
  RCV_CHECK_ARG(a.in && a.w && a.out, "conv: null operand");
  RCV_CHECK_ARG(a.in_mode == RCV_LOAD_PLAIN || a.in_mode == RCV_LOAD_NCHW || a.in_c, "conv: load mode %d needs constants", a.in_mode);
  RCV_CHECK_ARG(!(a.in_mode == RCV_LOAD_GRAD_ENC || a.in_mode == RCV_LOAD_GRAD_DEC) || a.in_aux, "conv: gradient load needs aux tensor");
  RCV_CHECK_ARG(!(a.flags & RCV_F_BIAS) || a.bias, "conv: bias flag without bias");
  RCV_CHECK_ARG(!(a.flags & RCV_F_RESID) || a.resid, "conv: resid flag without tensor");
  RCV_CHECK_ARG(a.stats == RCV_STATS_NONE || a.part, "conv: statistics requested without workspace");
  RCV_CHECK_ARG(a.stats == RCV_STATS_NONE || op->i[RCV_I_NPART] == pl.n_part, "conv: workspace rows %d != %d", op->i[RCV_I_NPART], pl.n_part);
  RCV_CHECK_ARG(!(a.stats == RCV_STATS_BWD_ENC || a.stats == RCV_STATS_BWD_DEC) || a.epi_aux, "conv: backward statistics need epi_aux");
  RCV_CHECK_ARG(!(a.stats == RCV_STATS_BWD_ENC || a.stats == RCV_STATS_BWD_DEC) || a.epi_c, "conv: backward statistics need epi_c (scale, shift, mean)");
  return fam.launch(pl, a, s);
}

// The layout the engine packs a record's filter in: the first row that asks for one (force: skip the split-bf16 rows).
int rcv_filter_layout(const rcv_handle* h, const rcv_op* op, int force) {
  for (const ConvFamily* f : kConvFamilies)
    if (const int layout = f->layout ? f->layout(h, op, force) : 0) return layout;
  return 0;
}

static int wgrad_plan(const rcv_handle* h, const rcv_op* op, WPlan* pl) {
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], CA = op->i[RCV_I_CIN], CB = op->i[RCV_I_COUT];
  const int Hp = op->i[RCV_I_HO], Wp = op->i[RCV_I_WO], s = op->i[RCV_I_STRIDE], d = op->i[RCV_I_DIL];
  RCV_CHECK_ARG(N > 0 && H > 0 && W > 0 && CA > 0 && CB > 0, "wgrad: empty shape");
  RCV_CHECK_ARG((s == 1 || s == 2) && (d == 1 || d == 2), "wgrad: stride %d dilation %d unsupported", s, d);
  RCV_CHECK_ARG(Hp == (H - 1) / s + 1 && Wp == (W - 1) / s + 1, "wgrad: pointwise plane %dx%d does not match %dx%d / %d", Hp, Wp, H, W, s);
  RCV_CHECK_ARG(CB % 4 == 0, "wgrad: pointwise channels %d must be a multiple of 4", CB);
  RCV_CHECK_ARG((size_t)N * H * W * CA < (1ull << 31) && (size_t)N * Hp * Wp * CB < (1ull << 31), "wgrad: operand exceeds 2^31 elements (32-bit offsets)");
  if (op->i[RCV_I_INMODE] == RCV_LOAD_NCHW) RCV_CHECK_ARG(CA <= 4, "wgrad: NCHW gathered operand supports <=4 channels");
  else RCV_CHECK_ARG(CA % 4 == 0, "wgrad: gathered channels %d must be a multiple of 4", CA);
  pl->CAP = wgrad_cap(CA); pl->CBP = round_up(CB, 16);
  for (const WgradFamily* f : kWgradFamilies)
    if (f->supported(h, op)) return f->plan(h, op, pl);
  rcv_set_error("wgrad: no kernel family takes the record");
  return RCV_E_ARG;
}

int rcv_launch_wgrad(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  if (op->kind != RCV_OP_WGRAD) {      // the two reduce records
    if (!query) return wgrad_reduce_launch(h, op, s);
    snprintf(query->label, sizeof(query->label), op->kind == RCV_OP_WGRAD_REDUCE_BATCH ? "wgrad_reduce_batch" : "wgrad_reduce");
    return RCV_OK;
  }
  WPlan pl;
  if (!rcv_plan_get(h, op, &pl)) {
    memset(&pl, 0, sizeof(pl));
    const int rc = wgrad_plan(h, op, &pl);
    if (rc) return rc;
    rcv_plan_put(h, op, pl);
  }
  const WgradFamily& fam = *kWgradFamilies[pl.path];
  WgradArgs a;
  a.g_mode = op->i[RCV_I_INMODE]; a.p_mode = op->i[RCV_I_INMODE2];
  const bool g_two = a.g_mode == RCV_LOAD_GRAD_ENC || a.g_mode == RCV_LOAD_GRAD_DEC;
  const bool p_two = a.p_mode == RCV_LOAD_GRAD_ENC || a.p_mode == RCV_LOAD_GRAD_DEC;
  // load-mode refusals belong to the shape of the record: in front of the query return (what the planner accepts, the launch accepts)
  RCV_CHECK_ARG(a.p_mode != RCV_LOAD_NCHW, "wgrad: pointwise operand cannot be NCHW");
  RCV_CHECK_ARG(!(g_two && p_two), "wgrad: at most one operand may be a gradient (two-tensor) load");
  if (query) {
    fam.label(pl, op, query->label, sizeof(query->label));
    query->n_split = pl.nsplit;
    query->part_bytes = (size_t)pl.nsplit * (9 * (size_t)pl.CBP * pl.CAP + pl.CBP) * sizeof(float);
    return RCV_OK;
  }
  a.g = (const float*)op->p[RCV_P_IN]; a.g_aux = (const float*)op->p[RCV_P_IN_AUX]; a.g_c = (const float*)op->p[RCV_P_IN_C];
  a.p = (const float*)op->p[RCV_P_IN2]; a.p_aux = (const float*)op->p[RCV_P_IN2_AUX]; a.p_c = (const float*)op->p[RCV_P_IN2_C];
  a.part = (float*)op->p[RCV_P_PART];
  a.N = op->i[RCV_I_N]; a.H = op->i[RCV_I_H]; a.W = op->i[RCV_I_W]; a.Hp = op->i[RCV_I_HO]; a.Wp = op->i[RCV_I_WO];
  a.CA = op->i[RCV_I_CIN]; a.CB = op->i[RCV_I_COUT]; a.CAP = pl.CAP; a.CBP = pl.CBP;
  a.stride = op->i[RCV_I_STRIDE]; a.dil = op->i[RCV_I_DIL];
  a.R = pl.R; a.Wt = pl.Wt; a.Wt4 = pl.Wt4; a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y;
  a.ntiles = a.N * pl.tiles_x * pl.tiles_y; a.IH = pl.IH; a.IW = pl.IW; a.SP = pl.SP; a.SG = pl.SG;
  a.dbg = op->flags; a.nsplit = pl.nsplit; a.nctiles = pl.nctiles; a.pl_floats = pl.pl_floats; a.gl_floats = pl.gl_floats;
  a.fdWt4 = make_fastdiv(pl.Wt4); a.fdIW = make_fastdiv(pl.IW);
  RCV_CHECK_ARG(a.g && a.p && a.part, "wgrad: null operand");
  RCV_CHECK_ARG(op->i[RCV_I_NSPLIT] == pl.nsplit, "wgrad: workspace splits %d != %d", op->i[RCV_I_NSPLIT], pl.nsplit);
  RCV_CHECK_ARG(a.g_mode == RCV_LOAD_PLAIN || a.g_mode == RCV_LOAD_NCHW || a.g_c, "wgrad: gathered load mode %d needs constants", a.g_mode);
  RCV_CHECK_ARG(a.p_mode == RCV_LOAD_PLAIN || a.p_c, "wgrad: pointwise load mode %d needs constants", a.p_mode);
  RCV_CHECK_ARG(!g_two || a.g_aux, "wgrad: gathered gradient load needs aux");
  RCV_CHECK_ARG(!p_two || a.p_aux, "wgrad: pointwise gradient load needs aux");
  a.part_bias = (op->flags & RCV_F_BIAS) ? a.part + (size_t)pl.nsplit * 9 * pl.CBP * pl.CAP : nullptr;
  return fam.launch(h, pl, a, s);
}
