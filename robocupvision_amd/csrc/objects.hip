// RCV_OP_OBJECTS: the objects of a class map -- per image and class 1..C-1 the largest 8-connected components with their bounding box,
// pixel area, component number and doubled box centre (test.py:43-67; the per-class area rules of DBConvert.py:47-102), DESIGN §4.9.
//
//   init -> merge -> count -> plane -> rank -> box/area stats     the stages of objdet_stages.h over N single planes
//   select     one wave per (image, class): walks the class's contiguous component entries; |A| and amax, |Q|, then the top `cap` by
//              (area descending, rank ascending); writes the rows, their zero fill and the four counts
//
// Two forms with identical output bytes, chosen by the SHAPE of the record alone (obj_route_lds; measured):
//   general    seven launches, union-find parents in global memory: any plane the contract admits
//   lds        one launch, one 1024-thread workgroup per image: class words, parents and the tile tables live in LDS, the stages are
//              separated by workgroup barriers, merging uses LDS atomicMin; rank-of-root and the component table stay in the global
//              workspace (an isolated-pixel plane has more components than LDS can hold stats for)
//
// Integer atomics only (min / max / add into the component table: order-free); select is a pure function of that table.
#include <math.h>
#include "objdet_stages.h"

namespace {

constexpr int OBJ_MAXM = 16;
constexpr int OBJ_LDS_THREADS = 1024;
constexpr int OBJ_LDS_TILES = OBJ_LDS_THREADS / OD_TILE;   // tiles the lds form handles per pass
// the lds form keeps 20 bytes per 2x2 block (class word + four parents) and 64 per tile in LDS: 30 tiles = 7680 blocks (a 120 x 256
// plane) is the largest multiple of OBJ_LDS_TILES that fits 160 KiB
constexpr int OBJ_LDS_MAX_BLOCKS = 7680;
// batches from this size on take the lds form when the plane fits: measured (scripts/bench_objects.py) it loses to the general
// form at 1..32 images of 120x160 (one workgroup per image leaves the chip idle and is bound by the merge's dependent LDS atomics) and
// wins at 64, 128 and 256, where the general form's global atomics contend
constexpr int OBJ_LDS_MIN_N = 64;

struct ObjSel {
  double ratio[OD_MAXC];   // [c] fp64 as given
  int min_area[OD_MAXC];
  int cap[OD_MAXC];
  int M;
};

struct ObjWs {
  uint32_t* cls;    // [N][NB] four class bytes per 2x2 block          (general form only)
  int* L;           // [N][QP] union-find parent (plane-local q)       (general form only)
  int* R;           // [N][QP] rank of a root among the roots of its class
  int* comp;        // [N * QP][8] component table, gid = plane * QP + class base + rank
  int* tcnt;        // [N][tiles][8] roots per class and tile          (general form only)
  int* toff;        // [N][tiles][8] exclusive offsets of the tiles    (general form only)
  int* pc;          // [N][16] components per class, [8..15] gid base  (general form only)
};

static inline size_t obj_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t obj_layout(const OdGeo& g, char* base, ObjWs* w) {
  const size_t P = (size_t)g.N;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += obj_align(bytes); return p; };
  char* r = take(P * g.QP * 4);
  char* cp = take(P * g.QP * 32);
  char* cl = take(P * g.NB * 4);
  char* l = take(P * g.QP * 4);
  char* tc = take(P * g.tiles * 8 * 4);
  char* to = take(P * g.tiles * 8 * 4);
  char* pc = take(P * 16 * 4);
  if (w) {
    w->cls = (uint32_t*)cl; w->L = (int*)l; w->R = (int*)r; w->comp = (int*)cp; w->tcnt = (int*)tc; w->toff = (int*)to; w->pc = (int*)pc;
  }
  return off;
}

__device__ __forceinline__ unsigned long long obj_wave_max64(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}

// select, one wave: e0 = the n contiguous component entries of one (image, class) in rank order.  Entry j qualifies for A when
// area > min_area, for Q when also (double)area >= (double)amax * ratio; the key (area << 32) | (0x7fffffff - j) orders Q by area
// descending, rank ascending, and is unique per entry.  Round r takes the largest key below round r-1's: `emit` <= 16 passes over
// the entries (the first 64 stay in registers), nothing depends on the order in which the table was filled.  L2 = true reads the
// table past this CU's vector cache (the lds form: the table was finished by atomics in L2 within the same launch).
template <bool L2>
__device__ __forceinline__ int obj_entry(const int* p) { return L2 ? od_ld(p) : *p; }

template <bool L2>
__device__ __forceinline__ void obj_select(const int* __restrict__ e0, int n, int min_area, double ratio, int cap, int M,
                                           int* __restrict__ rows, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int a_first = lane < n ? obj_entry<L2>(e0 + (size_t)lane * 8 + CAREA) : 0;      // areas are >= 1: 0 never qualifies
  int nA = 0, amax = 0;
  if (a_first > min_area) { nA = 1; amax = a_first; }
  for (int j = lane + 64; j < n; j += 64) {
    const int a = obj_entry<L2>(e0 + (size_t)j * 8 + CAREA);
    if (a > min_area) { ++nA; amax = max(amax, a); }
  }
  nA = od_wave_sum(nA);
  amax = od_wave_max(amax);
  const double lim = (double)amax * ratio;
  const bool q_first = a_first > min_area && (double)a_first >= lim;
  int nQ = q_first ? 1 : 0;
  for (int j = lane + 64; j < n; j += 64) {
    const int a = obj_entry<L2>(e0 + (size_t)j * 8 + CAREA);
    nQ += (a > min_area && (double)a >= lim) ? 1 : 0;
  }
  nQ = od_wave_sum(nQ);
  const int emit = min(nQ, cap);
  const unsigned long long k_first = q_first ? (((unsigned long long)(uint32_t)a_first << 32) | (uint32_t)(0x7fffffff - lane)) : 0ull;
  unsigned long long prev = ~0ull, mine = 0ull;
  for (int r = 0; r < emit; ++r) {
    unsigned long long best = k_first < prev ? k_first : 0ull;
    for (int j = lane + 64; j < n; j += 64) {
      const int a = obj_entry<L2>(e0 + (size_t)j * 8 + CAREA);
      if (a > min_area && (double)a >= lim) {
        const unsigned long long k = ((unsigned long long)(uint32_t)a << 32) | (uint32_t)(0x7fffffff - j);
        if (k < prev && k > best) best = k;
      }
    }
    best = obj_wave_max64(best);
    prev = best;
    if (lane == r) mine = best;
  }
  if (lane < M) {
    int4 lo = make_int4(0, 0, 0, 0), hi = make_int4(0, 0, 0, 0);
    if (lane < emit) {
      const int rank = 0x7fffffff - (int)(uint32_t)mine;
      const int* e = e0 + (size_t)rank * 8;
      const int4 bb = make_int4(obj_entry<L2>(e + CX0), obj_entry<L2>(e + CX1), obj_entry<L2>(e + CY0), obj_entry<L2>(e + CY1));
      const int w = bb.y - bb.x + 1, h = bb.w - bb.z + 1;
      lo = make_int4(bb.x, bb.z, w, h);
      hi = make_int4((int)(mine >> 32), rank, 2 * bb.x + w, 2 * bb.z + h);
    }
    *reinterpret_cast<int4*>(rows + (size_t)lane * 8) = lo;
    *reinterpret_cast<int4*>(rows + (size_t)lane * 8 + 4) = hi;
  }
  if (lane == 0) *reinterpret_cast<int4*>(counts) = make_int4(n, nA, nQ, emit);
}

// ------------------------------------------------------------------------------------------------------------------------------
// general form: grid (tiles, N) x OD_TILE for the per-block stages
__global__ __launch_bounds__(OD_TILE) void obj_init_kernel(const void* __restrict__ src, OdGeo g, uint32_t* __restrict__ cls,
                                                           int* __restrict__ L) {
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  if (b >= g.NB) return;
  od_init_block(g, src, g.pbytes, pl, b, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP);
}

__global__ __launch_bounds__(OD_TILE) void obj_merge_kernel(OdGeo g, const uint32_t* __restrict__ cls, int* L) {
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  if (b >= g.NB) return;
  od_merge_block(g, b, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP);
}

__global__ __launch_bounds__(OD_TILE) void obj_count_kernel(OdGeo g, const uint32_t* __restrict__ cls, int* L, int* __restrict__ tcnt) {
  __shared__ int wc[OD_TILE / 64][OD_MAXC];
  const int pl = blockIdx.y;
  od_count_tile(g, blockIdx.x * OD_TILE + threadIdx.x, blockIdx.x, threadIdx.x, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP,
                tcnt + (size_t)pl * g.tiles * OD_MAXC, wc);
}

// grid N x 256
__global__ __launch_bounds__(256) void obj_plane_kernel(OdGeo g, const int* __restrict__ tcnt, int* __restrict__ toff, int* __restrict__ pc) {
  __shared__ int sh[16];
  __shared__ int tot[OD_MAXC];
  const int pl = blockIdx.x;
  od_plane_scan<256>(g, tcnt + (size_t)pl * g.tiles * OD_MAXC, toff + (size_t)pl * g.tiles * OD_MAXC, pc + pl * 16, nullptr, 0, sh, tot);
}

__global__ __launch_bounds__(OD_TILE) void obj_rank_kernel(OdGeo g, const uint32_t* __restrict__ cls, const int* __restrict__ L,
                                                           const int* __restrict__ toff, const int* __restrict__ pc, int* __restrict__ R,
                                                           int* __restrict__ comp) {
  __shared__ int wc[OD_TILE / 64][OD_MAXC];
  const int pl = blockIdx.y;
  od_rank_tile(g, blockIdx.x * OD_TILE + threadIdx.x, blockIdx.x, threadIdx.x, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP,
               toff + (size_t)pl * g.tiles * OD_MAXC, pc + pl * 16, R + (size_t)pl * g.QP, comp + (size_t)pl * g.QP * 8, wc);
}

__global__ __launch_bounds__(OD_TILE) void obj_stats_kernel(OdGeo g, const uint32_t* __restrict__ cls, const int* __restrict__ L,
                                                            const int* __restrict__ R, const int* __restrict__ pc, int* comp) {
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  const bool in = b < g.NB;
  const uint32_t cw = in ? cls[(size_t)pl * g.NB + b] : 0u;
  const size_t pbase = (size_t)pl * g.QP;
  int4 l = make_int4(0, 0, 0, 0);
  if (cw) l = *reinterpret_cast<const int4*>(L + pbase + 4 * b);
  const int lv[4] = {l.x, l.y, l.z, l.w};
  od_stats_boxes(g, in, b, cw, lv, pbase, R + pbase, pc + pl * 16, comp);
}

// grid N * (C-1) x 64
__global__ __launch_bounds__(64) void obj_select_kernel(OdGeo g, ObjSel sel, const int* __restrict__ pc, const int* __restrict__ comp,
                                                        int* __restrict__ rows, int* __restrict__ counts) {
  const int pl = blockIdx.x / (g.C - 1), c = blockIdx.x % (g.C - 1) + 1;
  const size_t oc = (size_t)pl * (g.C - 1) + c - 1;
  obj_select<false>(comp + ((size_t)pl * g.QP + pc[pl * 16 + 8 + c]) * 8, pc[pl * 16 + c], sel.min_area[c], sel.ratio[c], sel.cap[c], sel.M,
             rows + oc * sel.M * 8, counts + oc * 4);
}

// ------------------------------------------------------------------------------------------------------------------------------
// lds form: grid N x 1024.  Dynamic LDS, every carve a multiple of 16 bytes: L[QP] | cls[round4(NB)] | tcnt[T][8] | toff[T][8] | wc[16][8] |
// pc[16] | sh[16] | tot[8], T = tiles rounded up to OBJ_LDS_TILES (a pass handles OBJ_LDS_TILES tiles, the last one may run past
// `tiles`: those threads have b >= NB and write zero counts into the padding).  Every thread runs every pass (the tile bodies hold
// barriers).
__host__ __device__ inline int obj_lds_tiles(int tiles) { return (tiles + OBJ_LDS_TILES - 1) / OBJ_LDS_TILES * OBJ_LDS_TILES; }
__host__ __device__ inline size_t obj_lds_bytes(int NB, int tiles) {
  return (size_t)NB * 16 + (size_t)((NB + 3) & ~3) * 4 + (size_t)obj_lds_tiles(tiles) * 64 + (size_t)(16 * OD_MAXC + 16 + 16 + OD_MAXC) * 4;
}

__global__ __launch_bounds__(OBJ_LDS_THREADS) void obj_lds_kernel(const void* __restrict__ src, OdGeo g, ObjSel sel, int* __restrict__ Rg,
                                                                  int* compg, int* __restrict__ rows, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char obj_sh[];
  const int T = obj_lds_tiles(g.tiles);
  int* L = reinterpret_cast<int*>(obj_sh);
  uint32_t* cls = reinterpret_cast<uint32_t*>(L + g.QP);
  int* tcnt = reinterpret_cast<int*>(cls + ((g.NB + 3) & ~3));
  int* toff = tcnt + T * OD_MAXC;
  int (*wc)[OD_MAXC] = reinterpret_cast<int (*)[OD_MAXC]>(toff + T * OD_MAXC);
  int* pc = toff + T * OD_MAXC + 16 * OD_MAXC;
  int* sh = pc + 16;
  int* tot = sh + 16;
  const int pl = blockIdx.x;
  const int tsub = threadIdx.x / OD_TILE, tl = threadIdx.x % OD_TILE;
  const size_t pbase = (size_t)pl * g.QP;
  int* R = Rg + pbase;

  for (int b = threadIdx.x; b < g.NB; b += OBJ_LDS_THREADS) od_init_block(g, src, g.pbytes, pl, b, cls, L);
  __syncthreads();
  for (int b = threadIdx.x; b < g.NB; b += OBJ_LDS_THREADS) od_merge_block(g, b, cls, L);
  __syncthreads();
  for (int t0 = 0; t0 < g.tiles; t0 += OBJ_LDS_TILES) {
    const int tile = t0 + tsub;
    od_count_tile(g, tile * OD_TILE + tl, tile, tl, cls, L, tcnt, wc + tsub * (OD_TILE / 64));
    __syncthreads();      // wc is reused by the next pass
  }
  od_plane_scan<OBJ_LDS_THREADS>(g, tcnt, toff, pc, nullptr, 0, sh, tot);
  __syncthreads();
  for (int t0 = 0; t0 < g.tiles; t0 += OBJ_LDS_TILES) {
    const int tile = t0 + tsub;
    od_rank_tile(g, tile * OD_TILE + tl, tile, tl, cls, L, toff, pc, R, compg + pbase * 8, wc + tsub * (OD_TILE / 64));
    __syncthreads();
  }
  // (R and the initialised table entries were written with plain stores by other waves of this workgroup: the barrier above waits
  // for them -- the vector cache writes through, so the atomics of stats, which work in L2, find the entries initialised)
  for (int t0 = 0; t0 < g.tiles; t0 += OBJ_LDS_TILES) {
    const int b = (t0 + tsub) * OD_TILE + tl;
    const bool in = b < g.NB;
    const uint32_t cw = in ? cls[b] : 0u;
    int4 l = make_int4(0, 0, 0, 0);
    if (cw) l = *reinterpret_cast<const int4*>(L + 4 * b);
    const int lv[4] = {l.x, l.y, l.z, l.w};
    od_stats_boxes(g, in, b, cw, lv, pbase, R, pc, compg);
  }
  __syncthreads();      // the table is finished, by atomics in L2: select reads it there
  const int c = (int)(threadIdx.x >> 6) + 1;
  if (c < g.C) {
    const size_t oc = (size_t)pl * (g.C - 1) + c - 1;
    obj_select<true>(compg + (pbase + pc[8 + c]) * 8, pc[c], sel.min_area[c], sel.ratio[c], sel.cap[c], sel.M, rows + oc * sel.M * 8,
               counts + oc * 4);
  }
}

// the form a record takes: its shape alone decides (i[AUX0]: 0 = this rule, 1 = general, 2 = lds, for tests and the A/B timing)
static bool obj_route_lds(int N, int NB, int force) {
  if (force) return force == 2;
  return NB <= OBJ_LDS_MAX_BLOCKS && N >= OBJ_LDS_MIN_N;
}

}  // namespace

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_OBJECTS).  Record:
//   i: N, H, W; COUT = C (2..8); COUNT = M (1..16); INMODE = element bytes of the class map (1 = uint8, 8 = int64); AUX0 = form
//      (0 = the library's choice, 1 = general, 2 = lds); NPART = workspace size in 256-byte units (filled by the query)
//   p: IN = class map [N][H][W], OUT = rows int32 [N][C-1][M][8], X0 = counts int32 [N][C-1][4] (both overwritten), PART = workspace,
//      X1 = HOST double[C-1] min_ratio, X2 = HOST int32[C-1] min_area, X3 = HOST int32[C-1] cap, read when the record is enqueued
// Every refusal that depends on the shape of the record (the per-class rules included) sits in front of the query return.
// --------------------------------------------------------------------------------------------
int rcv_launch_objects(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "objects";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_COUT], M = op->i[RCV_I_COUNT];
  const int eb = op->i[RCV_I_INMODE], force = op->i[RCV_I_AUX0];
  RCV_CHECK_ARG(C >= 2 && C <= OD_MAXC, "%s: %d classes unsupported (2..%d)", what, C, OD_MAXC);
  RCV_CHECK_ARG(M >= 1 && M <= OBJ_MAXM, "%s: max_objects %d unsupported (1..%d)", what, M, OBJ_MAXM);
  RCV_CHECK_ARG(eb == 1 || eb == 8, "%s: class map element size %d unsupported (1 = uint8, 8 = int64)", what, eb);
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(force >= 0 && force <= 2, "%s: form %d unknown (0 = the library's choice, 1 = general, 2 = lds)", what, force);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && N <= 32767 && H <= 8192 && W <= 8192, "%s: batch %d of %dx%d planes out of range", what,
                N, H, W);
  const long long NBl = (long long)((H + 1) / 2) * ((W + 1) / 2);
  RCV_CHECK_ARG(NBl <= OD_MAX_BLOCKS, "%s: a %dx%d plane is too large (at most %d 2x2 blocks)", what, H, W, OD_MAX_BLOCKS);
  RCV_CHECK_ARG((double)N * 4.0 * (double)NBl < 2147483647.0, "%s: batch %d of %dx%d planes too large for 32-bit component ids", what, N, H, W);
  RCV_CHECK_ARG(force != 2 || NBl <= OBJ_LDS_MAX_BLOCKS, "%s: a %dx%d plane does not fit the lds form (at most %d 2x2 blocks)", what, H, W,
                OBJ_LDS_MAX_BLOCKS);
  const double* ratio = (const double*)op->p[RCV_P_X1];
  const int32_t* min_area = (const int32_t*)op->p[RCV_P_X2];
  const int32_t* cap = (const int32_t*)op->p[RCV_P_X3];
  RCV_CHECK_ARG(ratio && min_area && cap, "%s: per-class rules (p[X1] min_ratio: host double[C-1], p[X2] min_area, p[X3] cap: host int32[C-1]) missing",
                what);
  ObjSel sel;
  memset(&sel, 0, sizeof(sel));
  sel.M = M;
  for (int c = 1; c < C; ++c) {
    RCV_CHECK_ARG(min_area[c - 1] >= 0, "%s: min_area of class %d (%d) must be >= 0", what, c, min_area[c - 1]);
    RCV_CHECK_ARG(isfinite(ratio[c - 1]) && ratio[c - 1] >= 0.0 && ratio[c - 1] <= 1.0, "%s: min_ratio of class %d (%g) must be in [0, 1]", what,
                  c, ratio[c - 1]);
    RCV_CHECK_ARG(cap[c - 1] >= 0 && cap[c - 1] <= M, "%s: cap of class %d (%d) must be in [0, max_objects = %d]", what, c, cap[c - 1], M);
    sel.ratio[c] = ratio[c - 1]; sel.min_area[c] = min_area[c - 1]; sel.cap[c] = cap[c - 1];
  }
  OdGeo g;
  memset(&g, 0, sizeof(g));
  g.N = N; g.H = H; g.W = W; g.C = C; g.Wb = (W + 1) / 2; g.NB = (int)NBl; g.QP = 4 * g.NB; g.tiles = ceil_div(g.NB, OD_TILE);
  g.pbytes = eb; g.tbytes = eb;
  const bool lds = obj_route_lds(N, g.NB, force);
  const size_t bytes = obj_layout(g, nullptr, nullptr);
  RCV_CHECK_ARG(bytes / 256 < 2147483647ull, "%s: workspace too large", what);
  if (query) {
    snprintf(query->label, sizeof(query->label), "objects<%s%s>", eb == 1 ? "u8" : "i64", lds ? ",lds" : "");
    query->n_part = (int)(bytes / 256);
    query->part_bytes = bytes;
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_OUT] && op->p[RCV_P_X0], "%s: null operand", what);
  RCV_CHECK_ARG((((uintptr_t)op->p[RCV_P_OUT] | (uintptr_t)op->p[RCV_P_X0]) & 15) == 0, "%s: rows / counts not 16-byte aligned", what);
  RCV_CHECK_ARG(op->p[RCV_P_PART] && ((uintptr_t)op->p[RCV_P_PART] & 255) == 0, "%s: workspace missing or not 256-byte aligned", what);
  RCV_CHECK_ARG(op->i[RCV_I_NPART] == (int)(bytes / 256), "%s: workspace of %d x 256 bytes given, %zu expected (rcv_op_workspace)", what,
                op->i[RCV_I_NPART], bytes / 256);
  ObjWs w;
  obj_layout(g, (char*)op->p[RCV_P_PART], &w);
  int* rows = (int*)op->p[RCV_P_OUT];
  int* counts = (int*)op->p[RCV_P_X0];
  if (lds) {
    const size_t sh = obj_lds_bytes(g.NB, g.tiles);
    RCV_CHECK_ARG(sh <= (size_t)h->max_lds, "%s: the lds form needs %zu bytes of LDS, %d available", what, sh, h->max_lds);
    static size_t configured[RCV_MAX_DEVICES];
    RCV_ENSURE_LDS(obj_lds_kernel, sh, h->device, configured);
    hipLaunchKernelGGL(obj_lds_kernel, dim3(N), dim3(OBJ_LDS_THREADS), sh, s, op->p[RCV_P_IN], g, sel, w.R, w.comp, rows, counts);
    RCV_HIP(hipGetLastError());
    return RCV_OK;
  }
  const dim3 grid(g.tiles, N);
  hipLaunchKernelGGL(obj_init_kernel, grid, dim3(OD_TILE), 0, s, op->p[RCV_P_IN], g, w.cls, w.L);
  hipLaunchKernelGGL(obj_merge_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L);
  hipLaunchKernelGGL(obj_count_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.tcnt);
  hipLaunchKernelGGL(obj_plane_kernel, dim3(N), dim3(256), 0, s, g, w.tcnt, w.toff, w.pc);
  hipLaunchKernelGGL(obj_rank_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.toff, w.pc, w.R, w.comp);
  hipLaunchKernelGGL(obj_stats_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.R, w.pc, w.comp);
  hipLaunchKernelGGL(obj_select_kernel, dim3(N * (C - 1)), dim3(64), 0, s, g, sel, w.pc, w.comp, rows, counts);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
