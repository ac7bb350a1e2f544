// Shared declarations of the convolution kernel families (dispatch: conv_dispatch.hip).
#pragma once
#include "load_xform.h"
#include "bn_sums.h"
#include "stream_hint.h"

enum { KIND_GATHER = 0, KIND_TPHASE = 1, KIND_TMERGED = 2, KIND_TALL = 3 };   // TALL: all four output parities of a transposed conv in one workgroup

struct ConvArgs {
  const float* in;
  const float* in_aux;
  const float* in_c;   // [5][Cin]
  const float* w;      // [taps][CinP][CoutP]
  const float* bias;
  float* out;
  const float* resid;
  const float* epi_aux;
  const float* epi_c;  // [2][Cout]
  float* part;         // [n_part][2][Cout]
  int N, H, W, Cin, Cout, Ho, Wo;
  int CinP, CoutP, CoutV;      // padded rows / cols of the packed filter; number of (virtual) output channels
  int stride, dil;
  int R, Wt, tiles_x, tiles_y, IH, IW;
  int n_pix_tiles, n_co_tiles, n_sub, total_tiles, nchunks;
  int in_mode, stats;
  uint32_t flags;
  int wl_floats, xl_floats;    // LDS carve: filter tile, input tile (then constants, then reduction scratch)
  int xpitch;                  // floats per staged input pixel (see conv_xpitch)
  int xk;                      // conv_dma_kernel: channels per staged input chunk (8 or 16)
  FastDiv fdWt, fdIW;
  FastDiv fdTX, fdTY;          // tiles_x, tiles_y (narrow kernel: tile decode on the scalar unit)
  int nt_out, nt_pw;           // streaming hints (stream_hint.h).  nt_out: the final store of `out` (convs_mfma, convn_bf3, conv_first pick their
                               // STREAM instantiation by it); nt_pw: the epilogue operands resid / epi_aux -- carried, no conv family honours it yet
#ifdef RCV_STAMPS
  unsigned long long* stamps;  // diagnostic build: per wave [12] cycle sums (conv_dma_kernel)
#endif
};

struct TileInfo {
  int n, y0, x0, co0, py, px, oy0, ox0, pt;
};

template <int KIND>
__device__ __forceinline__ TileInfo decode_tile(const ConvArgs& a, int t, int COT) {
  TileInfo ti;
  const int sub = t % a.n_sub;
  int pt = t / a.n_sub;
  ti.pt = pt;
  const int co_tile = sub % a.n_co_tiles, phase = sub / a.n_co_tiles;
  const int tx_i = pt % a.tiles_x;
  pt /= a.tiles_x;
  const int ty_i = pt % a.tiles_y;
  ti.n = pt / a.tiles_y;
  ti.y0 = ty_i * a.R;
  ti.x0 = tx_i * a.Wt;
  ti.co0 = co_tile * COT;
  ti.py = phase >> 1;
  ti.px = phase & 1;
  if (KIND == KIND_GATHER) { ti.oy0 = ti.y0 * a.stride - a.dil; ti.ox0 = ti.x0 * a.stride - a.dil; }
  else { ti.oy0 = ti.y0; ti.ox0 = ti.x0; }
  return ti;
}

// Kernel families in order of precedence: ConvPlan::path is the row of kConvFamilies (conv_dispatch.hip)
enum { CONVN_BF3 = 0, CONV_BF3, CONV_WINO, CONV_FIRST, CONV_NARROW, CONV_SMALL, CONV_MFMA, CONV_DMA, CONV_NUM_FAMILIES };

struct ConvPlan {
  int kind, tile, CK, R, Wt, tiles_x, tiles_y, IH, IW;
  int CoutV, CoutP, n_co_tiles, n_phases, total_tiles, grid;
  size_t lds;
  int wl_floats, xl_floats;
  int path;              // the family that runs the record (CONV_*)
  int n_part;            // statistics rows of a launch: one per pixel tile and parity, or one per workgroup of a persistent kernel
  int xpitch_ck;         // channel count of a staged input pixel (conv_xpitch)
  int xk;                // conv_dma_kernel, conv_wino_kernel: channels per staged input chunk
  int WM, WN, XMAX;      // template selection of the families with several instantiations
  int dev;               // device of the handle the plan belongs to (per-device kernel attributes)
};

// One kernel family: a row of kConvFamilies, defined next to its kernels.  The first row whose `supported` accepts a record plans it
// (`plan` fills every field above but `dev`); the packer asks the same rows, in the same order, through `layout`.
struct ConvFamily {
  const char* name;
  bool (*supported)(const rcv_handle*, const rcv_op*, int kind);   // nullptr: reached through another row's plan
  int (*plan)(const rcv_handle*, const rcv_op*, int kind, ConvPlan*);
  int (*launch)(const ConvPlan&, const ConvArgs&, hipStream_t);
  void (*label)(const ConvPlan&, const rcv_op*, char* buf, size_t n);
  int (*layout)(const rcv_handle*, const rcv_op*, int force);      // filter layout this family asks the packer for (0: none / plain); nullptr where there is none
  unsigned layouts;      // bit L: the family reads a filter packed in layout L = 2..5 (RCV_I_AUX0); such a record runs on one of these rows or not at all
};
extern const ConvFamily kConvnBf3, kConvBf3, kConvWino, kConvFirst, kConvNarrow, kConvSmall, kConvMfma, kConvDma;

// 512-thread launch of a kernel whose grid and dynamic LDS are the plan's (rcv_launch_with_lds)
template <auto KERN>
static int conv_launch_with_lds(const ConvPlan& pl, const ConvArgs& a, hipStream_t s) {
  return rcv_launch_with_lds<KERN>(a, dim3(pl.grid), pl.lds, pl.dev, s);
}

// LDS pitch of a staged input pixel holding CK channels.  The B operand of v_mfma_f32_16x16x4_f32 is read with ds_read_b32 at
// (pixel(l15) * IS * pitch + l4): 16 pixels x 2 channel lanes per 32-lane half must fall on 32 different banks.  Unit-stride pixel
// blocks: pitch = CK + 2 (pitch/2 odd => 16 distinct even banks, + l4 the odd ones); stride-2 blocks: the lane stride is 2*pitch,
// so pitch = CK + 1 (odd).  (CK + 1 everywhere cost 46 % of all LDS cycles in bank conflicts on the unit-stride layers.)
static inline int conv_xpitch(int CK, int pixel_stride) {
  if (const char* ev = RCV_ENV("RCV_XPITCH_PAD")) return CK + atoi(ev);      // experiments build only
  return pixel_stride == 1 ? CK + 2 : CK + 1;
}

static inline void tile_halo(int kind, int R, int Wt, int s, int d, int* IH, int* IW) {
  if (kind == KIND_GATHER) { *IH = (R - 1) * s + 2 * d + 1; *IW = (Wt - 1) * s + 2 * d + 1; }
  else { *IH = R + 1; *IW = Wt + 1; }
}
