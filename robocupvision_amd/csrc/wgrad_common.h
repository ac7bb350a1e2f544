// Shared declarations of the filter-gradient kernel families (dispatch: conv_dispatch.hip).
#pragma once
#include "load_xform.h"

struct WgradArgs {
  const float* g; const float* g_aux; const float* g_c;
  const float* p; const float* p_aux; const float* p_c;
  float* part;        // [nsplit][9][CBP][CAP]
  float* part_bias;   // [nsplit][CBP] or null
  int g_mode, p_mode;
  int N, H, W, Hp, Wp, CA, CB, CAP, CBP;
  int stride, dil;
  int R, Wt, Wt4, tiles_x, tiles_y, ntiles, IH, IW, SP, SG;
  int nsplit, nctiles;
  uint32_t dbg;
  int pl_floats, gl_floats;      // LDS carve: P tile, G tile (then the load constants)
  FastDiv fdWt4, fdIW;
};

// padded gathered-channel count of the partial-filter layout [split][tap][CBP][CAP] (shared by the kernels and RCV_OP_WGRAD_REDUCE)
static inline int wgrad_cap(int CA) { return CA <= 4 ? 4 : round_up(CA, 16); }

// Kernel families in order of precedence: WPlan::path is the row of kWgradFamilies (conv_dispatch.hip: it fills CAP / CBP, `plan` the rest).
// `geom`: the tile width of wgrad_bf3, the tile rows of wgradn_bf3; `tile`: the row of wgrad_mfma's tile table.
enum { WGRAD_FIRST = 0, WGRAD_BF3, WGRADN_BF3, WGRAD_MFMA, WGRAD_NUM_FAMILIES };
struct WPlan { int path; int geom; int nctiles; int tile; int R, Wt, Wt4, tiles_x, tiles_y, IH, IW, SP, SG, nsplit, pl_floats, gl_floats; size_t lds; dim3 grid; int CAP, CBP; };
struct WgradFamily {      // one row, defined next to its kernels; the first row whose `supported` accepts a record plans it
  const char* name;
  bool (*supported)(const rcv_handle*, const rcv_op*);
  int (*plan)(const rcv_handle*, const rcv_op*, WPlan*);
  int (*launch)(const rcv_handle*, const WPlan&, const WgradArgs&, hipStream_t);
  void (*label)(const WPlan&, const rcv_op*, char* buf, size_t n);
};
extern const WgradFamily kWgradFirst, kWgradBf3, kWgradnBf3, kWgradMfma;
int wgrad_reduce_launch(const rcv_handle* h, const rcv_op* op, hipStream_t s);      // RCV_OP_WGRAD_REDUCE[_BATCH] (wgrad_mfma.hip)
