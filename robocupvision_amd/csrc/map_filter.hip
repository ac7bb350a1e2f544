// RCV_OP_MAP_FILTER (rcv_map_filter): cleaning a class map between "class map" and "objects / metrics / targets" -- the windowed
// majority vote the reference leaves switched off (labelExtraction.py:70-89 __filterMask, off at :46) and the morphology it leaves
// commented (test.py:41, cv2.morphologyEx(imgPred, cv2.MORPH_CLOSE, np.ones((3,3))) in front of connectedComponents), DESIGN §4.21.
//
// One kernel: per pixel the class counts h[c] of its k x k window (in-image pixels only; a void pixel counts in no class) and the
// number n of in-image pixels of the window, then one integer decision rule (rcv.h RCV_MF_*).
//
//   stage     the workgroup's MF_TH x MF_TW tile plus its halo as bytes in LDS: a class as its byte, void and outside as 255 (int64 maps
//             are narrowed on load); the bit-map rules stage the bit byte masked with the class set, outside as 0
//   rows      horizontal window sums of every staged row, the eight class counts packed one per byte lane: a pixel adds 1 << 8c, a
//             lane holds at most 15 here ...
//   columns   ... and at most 15 * 15 = 225 after the vertical sums, so no carry ever crosses a lane (this is why k stops at 15).  A
//             thread owns one column and MF_ROWS consecutive rows of the tile and slides the window down: add the entering row sum,
//             subtract the leaving one (every lane of the sum holds at least what leaves it: no borrow either)
//   decide    the rule, on h, n and the pixel's own value read from the map itself (an unchanged pixel keeps ALL its bits: a byte
//             >= C, -100, a value beyond 32 bits)
//
// Maps of at most 4 classes count in 32 bits (the upper four lanes do not exist).  Integer arithmetic only; the optional changed
// counter is added to with integer atomics (one per workgroup), so it does not depend on the order.  No workspace.
#include "rcv_internal.h"

namespace {

constexpr int MF_TH = RCV_MAP_FILTER_TILE_H, MF_TW = RCV_MAP_FILTER_TILE_W;
constexpr int MF_THREADS = 256;
constexpr int MF_MAXK = 15;
constexpr int MF_ROWS = MF_TH * MF_TW / MF_THREADS;      // rows of the tile one thread decides
constexpr int MF_SH = MF_TH + MF_MAXK - 1;               // staged rows
constexpr int MF_SP = 80;                                // staged row pitch in bytes (>= MF_TW + MF_MAXK - 1, a multiple of 4)
static_assert(MF_TW == 64 && MF_ROWS * MF_THREADS == MF_TH * MF_TW && MF_SP >= MF_TW + MF_MAXK - 1, "tile geometry");

struct MfArgs {
  const void* in;        // the windowed input: the class map, or the bit map of the *_FINISH rules
  const void* orig;      // the map the decision reads the pixel's own value from (== in unless a *_FINISH rule)
  void* out;
  int* changed;          // int32[N] or nullptr
  int N, H, W, C, k, rule, set, a0, a1;
  int tiles_x, tiles;    // tiles per row of tiles, tiles per image
};

template <typename CT>
__device__ __forceinline__ CT mf_one(int v) { return v < (int)sizeof(CT) ? (CT)1 << (8 * v) : (CT)0; }

// bit c of the byte -> 1 in lane c
__device__ __forceinline__ uint32_t mf_spread(uint32_t b, uint32_t) {
  const uint32_t x = (b * 0x01010101u) & 0x08040201u;
  return ((x + 0x7f7f7f7fu) >> 7) & 0x01010101u;
}
__device__ __forceinline__ unsigned long long mf_spread(uint32_t b, unsigned long long) {
  const unsigned long long x = ((unsigned long long)b * 0x0101010101010101ull) & 0x8040201008040201ull;
  return ((x + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

template <typename CT>
__device__ __forceinline__ int mf_lane(CT h, int c) { return (int)((h >> (8 * c)) & 0xff); }

// grid N * tiles x MF_THREADS.  EB: element bytes of the map (1 = uint8, 8 = int64); CT: the packed counts (32 bits up to 4 classes)
template <int EB, typename CT>
__global__ __launch_bounds__(MF_THREADS) void map_filter_kernel(MfArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_in[MF_SH * MF_SP];
  __shared__ __attribute__((aligned(16))) CT s_h[MF_SH * MF_TW];
  __shared__ int s_changed;
  const int tid = threadIdx.x;
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int y0 = ty * MF_TH, x0 = tx * MF_TW;
  const int k = a.k, r0 = k >> 1, r1 = k - 1 - r0;
  const int rows_s = MF_TH + k - 1;
  const bool bits = a.rule == RCV_MF_OPEN_FINISH || a.rule == RCV_MF_CLOSE_FINISH;
  const size_t plane = (size_t)a.H * a.W;
  if (tid == 0) s_changed = 0;

  // stage (the pitch's padding columns are staged as outside: nothing reads them)
  for (int i = tid; i < rows_s * MF_SP; i += MF_THREADS) {
    const int row = i / MF_SP, col = i - row * MF_SP;
    const int gy = y0 - r0 + row, gx = x0 - r0 + col;
    uint32_t b = bits ? 0u : 255u;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const size_t at = img * plane + (size_t)gy * a.W + gx;
      if (bits) {
        b = (uint32_t)((const uint8_t*)a.in)[at] & (uint32_t)a.set;
      } else if (EB == 1) {
        const uint32_t v = ((const uint8_t*)a.in)[at];
        b = v < (uint32_t)a.C ? v : 255u;
      } else {
        const long long v = ((const long long*)a.in)[at];
        b = (v >= 0 && v < a.C) ? (uint32_t)v : 255u;
      }
    }
    s_in[i] = (uint8_t)b;
  }
  __syncthreads();

  // rows: s_h[row][x] = the window sum of staged columns x .. x + k - 1
  for (int i = tid; i < rows_s * MF_TW; i += MF_THREADS) {
    const uint8_t* p = s_in + (i >> 6) * MF_SP + (i & 63);
    CT s = 0;
    if (bits) {
      for (int j = 0; j < k; ++j) s += mf_spread((uint32_t)p[j], (CT)0);
    } else {
      for (int j = 0; j < k; ++j) s += mf_one<CT>(p[j]);
    }
    s_h[i] = s;
  }
  __syncthreads();

  // columns + decide
  const int lx = tid & 63, ly0 = (tid >> 6) * MF_ROWS;
  const int x = x0 + lx;
  int n_changed = 0;
  if (x < a.W && y0 + ly0 < a.H) {
    const int ncols = min(a.W - 1, x + r1) - max(0, x - r0) + 1;
    const CT* hp = s_h + ly0 * MF_TW + lx;
    CT h = 0;
    for (int j = 0; j < k; ++j) h += hp[j * MF_TW];
    const int rows = min(MF_ROWS, a.H - y0 - ly0);
    for (int r = 0; r < rows; ++r) {
      const int y = y0 + ly0 + r;
      if (r) h += hp[(r - 1 + k) * MF_TW] - hp[(r - 1) * MF_TW];
      const int n = (min(a.H - 1, y + r1) - max(0, y - r0) + 1) * ncols;
      const size_t at = img * plane + (size_t)y * a.W + x;
      const long long raw = EB == 1 ? (long long)((const uint8_t*)a.orig)[at] : ((const long long*)a.orig)[at];
      const bool isc = raw >= 0 && raw < a.C;
      const int v = isc ? (int)raw : 0;
      const bool in_set = isc && ((a.set >> v) & 1);
      long long o = raw;
      switch (a.rule) {
        case RCV_MF_MAJORITY: {      // set = fill_void, a0 = min_major, a1 = min_own
          int m = 0, first = 0;
          for (int c = 0; c < a.C; ++c) {
            const int hc = mf_lane(h, c);
            if (hc > m) { m = hc; first = c; }
          }
          const int own = isc ? mf_lane(h, v) : 0;
          if ((isc || a.set) && (m >= a.a0 || (isc && own < a.a1))) o = first;
          break;
        }
        case RCV_MF_ERODE:           // a0 = fill
          if (in_set && mf_lane(h, v) < n) o = a.a0;
          break;
        case RCV_MF_ERODE_BITS:
          o = (in_set && mf_lane(h, v) == n) ? (1 << v) : 0;
          break;
        case RCV_MF_DILATE_BITS: {
          int bset = 0;
          for (int c = 0; c < a.C; ++c) bset |= mf_lane(h, c) ? (1 << c) : 0;
          o = bset & a.set;
          break;
        }
        case RCV_MF_OPEN_FINISH:     // a0 = fill
          if (in_set && mf_lane(h, v) == 0) o = a.a0;
          break;
        default: {                   // RCV_MF_CLOSE_FINISH: a1 = over (bit 8 = void)
          const bool claim = ((a.a1 >> (isc ? v : 8)) & 1) != 0;
          for (int c = 0; c < a.C; ++c)
            if (((a.set >> c) & 1) && mf_lane(h, c) == n && (claim || (isc && v == c))) { o = c; break; }
          break;
        }
      }
      if (a.rule == RCV_MF_ERODE_BITS || a.rule == RCV_MF_DILATE_BITS) {
        ((uint8_t*)a.out)[at] = (uint8_t)o;
      } else {
        if (EB == 1) ((uint8_t*)a.out)[at] = (uint8_t)o;
        else ((long long*)a.out)[at] = o;
        n_changed += o != raw ? 1 : 0;
      }
    }
  }
  if (a.changed) {      // (the same in every thread)
    if (n_changed) atomicAdd(&s_changed, n_changed);
    __syncthreads();
    if (tid == 0 && s_changed) atomicAdd(a.changed + img, s_changed);
  }
}

static const char* const MF_RULE_NAMES[6] = {"majority", "erode", "erode_bits", "dilate_bits", "open_finish", "close_finish"};

}  // namespace

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_MAP_FILTER).  Record:
//   i: N, H, W; COUT = C (1..8); COUNT = k (1..15); INMODE = element bytes of the map (1 = uint8, 8 = int64); INMODE2 = 1 when p[IN] is
//      a bit map (the *_FINISH rules, and only they); AUX0 = rule; AUX1 = class set S (majority: fill_void 0 / 1); STRIDE = fill
//      (majority: min_major); DIL = over set O, bit 8 = void (majority: min_own)
//   p: IN = the windowed input [N][H][W], IN2 = the original map of the *_FINISH rules, OUT = result [N][H][W] (not p[IN]),
//      X0 = changed int32[N] or NULL (added to)
// Every refusal that depends on the record sits in front of the query return; the two about pointers apply where the pointers are set.
// --------------------------------------------------------------------------------------------
int rcv_launch_map_filter(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "map_filter";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_COUT], k = op->i[RCV_I_COUNT];
  const int eb = op->i[RCV_I_INMODE], in_bits = op->i[RCV_I_INMODE2], rule = op->i[RCV_I_AUX0];
  const int set = op->i[RCV_I_AUX1], a0 = op->i[RCV_I_STRIDE], a1 = op->i[RCV_I_DIL];
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(rule >= RCV_MF_MAJORITY && rule <= RCV_MF_CLOSE_FINISH, "%s: rule %d unknown (0..5)", what, rule);
  const char* name = MF_RULE_NAMES[rule];
  const bool morph = rule >= RCV_MF_ERODE_BITS, finish = rule >= RCV_MF_OPEN_FINISH;
  RCV_CHECK_ARG(k >= 1 && k <= MF_MAXK, "%s: window %d unsupported (1..%d)", what, k, MF_MAXK);
  RCV_CHECK_ARG(!morph || (k & 1), "%s: rule %s takes odd windows only (got %d)", what, name, k);
  RCV_CHECK_ARG(C >= 1 && C <= 8, "%s: %d classes unsupported (1..8)", what, C);
  RCV_CHECK_ARG(eb == 1 || eb == 8, "%s: class map element size %d unsupported (1 = uint8, 8 = int64)", what, eb);
  RCV_CHECK_ARG(in_bits == (finish ? 1 : 0), "%s: rule %s reads %s (i[INMODE2] = %d, got %d)", what, name,
                finish ? "a bit map beside the original map" : "the class map alone", finish ? 1 : 0, in_bits);
  if (rule == RCV_MF_MAJORITY) {
    RCV_CHECK_ARG(a0 >= 1, "%s: min_major %d must be >= 1", what, a0);
    RCV_CHECK_ARG(a1 >= 0, "%s: min_own %d must be >= 0", what, a1);
    RCV_CHECK_ARG(set == 0 || set == 1, "%s: fill_void %d must be 0 or 1", what, set);
  } else {
    RCV_CHECK_ARG(set >= 0 && (set >> C) == 0, "%s: class set 0x%x names a class >= %d", what, set, C);
    if (rule == RCV_MF_ERODE || rule == RCV_MF_OPEN_FINISH)
      RCV_CHECK_ARG(eb == 8 || (a0 >= 0 && a0 <= 255), "%s: fill %d does not fit a uint8 map (0..255)", what, a0);
    if (rule == RCV_MF_CLOSE_FINISH)
      RCV_CHECK_ARG(a1 >= 0 && ((a1 & 0xff) >> C) == 0 && (a1 >> 9) == 0, "%s: over set 0x%x names a class >= %d (bit 8 = void)", what, a1, C);
  }
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: batch %d of %dx%d planes out of range", what, N, H, W);
  const int tiles_x = ceil_div(W, MF_TW), tiles_y = ceil_div(H, MF_TH);
  RCV_CHECK_ARG((double)N * tiles_x * tiles_y < 2147483647.0, "%s: batch %d of %dx%d planes has too many tiles for one grid", what, N, H, W);
  RCV_CHECK_ARG(!op->p[RCV_P_IN] || op->p[RCV_P_IN] != op->p[RCV_P_OUT], "%s: the filter cannot run in place (halo pixels are read after their neighbours are written)", what);
  RCV_CHECK_ARG(!finish || !op->p[RCV_P_IN] || op->p[RCV_P_IN2], "%s: rule %s needs the original map in p[IN2]", what, name);
  RCV_CHECK_ARG(!finish || !op->p[RCV_P_IN2] || op->p[RCV_P_IN2] != op->p[RCV_P_OUT], "%s: the result cannot overwrite the original map", what);
  if (query) {
    snprintf(query->label, sizeof(query->label), "map_filter<%s,%s,k%d,%s>", name, eb == 1 ? "u8" : "i64", k, C <= 4 ? "c4" : "c8");
    query->n_part = 0;
    query->n_split = 0;
    query->part_bytes = 0;
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_OUT], "%s: null operand", what);
  const bool wide_out = eb == 8 && rule != RCV_MF_ERODE_BITS && rule != RCV_MF_DILATE_BITS;
  RCV_CHECK_ARG(eb == 1 || (((uintptr_t)(finish ? op->p[RCV_P_IN2] : op->p[RCV_P_IN]) & 7) == 0 && (!wide_out || ((uintptr_t)op->p[RCV_P_OUT] & 7) == 0)),
                "%s: int64 map not 8-byte aligned", what);
  RCV_CHECK_ARG(((uintptr_t)op->p[RCV_P_X0] & 3) == 0, "%s: changed counter not 4-byte aligned", what);
  MfArgs a;
  a.in = op->p[RCV_P_IN]; a.orig = finish ? op->p[RCV_P_IN2] : op->p[RCV_P_IN]; a.out = op->p[RCV_P_OUT]; a.changed = (int*)op->p[RCV_P_X0];
  a.N = N; a.H = H; a.W = W; a.C = C; a.k = k; a.rule = rule; a.set = set; a.a0 = a0; a.a1 = a1;
  a.tiles_x = tiles_x; a.tiles = tiles_x * tiles_y;
  const dim3 grid((unsigned)(N * a.tiles)), block(MF_THREADS);
  if (C <= 4) {
    if (eb == 1) hipLaunchKernelGGL((map_filter_kernel<1, uint32_t>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((map_filter_kernel<8, uint32_t>), grid, block, 0, s, a);
  } else {
    if (eb == 1) hipLaunchKernelGGL((map_filter_kernel<1, unsigned long long>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((map_filter_kernel<8, unsigned long long>), grid, block, 0, s, a);
  }
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
