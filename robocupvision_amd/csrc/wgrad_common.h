// Shared declarations of the filter-gradient kernels (wgrad_mfma.hip: matrix cores; wgrad_first.hip: first layer on the vector ALU).
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

// first-layer kernel (wgrad_first.hip)
bool wgrad_first_supported(const rcv_op* op);
int wgrad_first_nsplit(const rcv_handle* h, const rcv_op* op);
int wgrad_first_launch(const rcv_handle* h, const WgradArgs& a, hipStream_t s);

// wide stride-1 layers on the bf16 matrix pipe (wgrad_bf3.hip)
bool wgrad_bf3_supported(const rcv_handle* h, const rcv_op* op);
void wgrad_bf3_geometry(const rcv_handle* h, const rcv_op* op, int* tw, int* tiles_x, int* tiles_y, int* nsplit, int* nctiles);
int wgrad_bf3_launch(const rcv_handle* h, const WgradArgs& a, int tw, hipStream_t s);

// narrow layers on the bf16 matrix pipe (wgradn_bf3.hip)
bool wgradn_bf3_supported(const rcv_handle* h, const rcv_op* op);
void wgradn_bf3_geometry(const rcv_handle* h, const rcv_op* op, int* th, int* tiles_x, int* tiles_y, int* ngroups);
int wgradn_bf3_launch(const rcv_handle* h, const WgradArgs& a, int th, int ngroups, hipStream_t s);
