// The labelling stages shared by RCV_OP_OBJECT_MATCH (objdet.hip) and RCV_OP_OBJECTS (objects.hip), DESIGN §4.3 / §4.9:
//
//   init -> merge -> count -> plane -> rank -> box/area stats
//
// Every stage is a __device__ body over ONE 2x2 block (or one tile of OD_TILE blocks, or one plane) of ONE plane, with plane-local
// pointers; the __global__ wrappers of the two translation units choose the plane (objdet.hip: 2N planes, pred / target interleaved;
// objects.hip: N planes) and where the union-find parents live (global memory, or LDS in the single-launch kernel of objects.hip).
// What only the matcher needs (the target planes, the pair hash table, the candidate lists) stays in objdet.hip.
#pragma once
#include "rcv_internal.h"

namespace {

constexpr int OD_TILE = 256;    // 2x2 blocks per tile of the per-block stages
constexpr int OD_MAXC = 8;
constexpr int OD_MAX_BLOCKS = 1 << 17;   // 2x2 blocks per plane (a 512 x 1024 plane); bounds the matcher's LDS (24 B per 64 blocks)

struct OdGeo {
  int N, H, W, C, Wb, NB, QP, tiles;   // NB = 2x2 blocks per plane, QP = 4 * NB (block-major pixel slots), tiles = ceil(NB / OD_TILE)
  int pbytes, tbytes;                  // element size of pred / target: 1 (uint8) or 8 (int64)
  uint32_t hmask;                      // pair hash capacity - 1
};

// component table entry (int[8] per gid): bounding box first (one 16-byte load), then area and the candidate list of a pred component
enum { CX0 = 0, CX1, CY0, CY1, CAREA, CCNT, COFF, CCUR };

__device__ __forceinline__ int od_cls(uint32_t cw, int i) { return (int)((cw >> (8 * i)) & 255u); }

// index of the first pixel of block word cw with the class of pixel i
__device__ __forceinline__ int od_rep(uint32_t cw, int i) {
  const int c = od_cls(cw, i);
  int j = 0;
  while (od_cls(cw, j) != c) ++j;
  return j;
}

__device__ __forceinline__ int od_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int od_find_live(const int* L, int a) {     // during the merge: parents change under our feet
  int b = od_ld(L + a);
  while (b != a) { a = b; b = od_ld(L + a); }
  return a;
}

// Playne & Hawick's lock-free union: link the larger root under the smaller; a failed link (the root got a parent meanwhile)
// continues from that parent.  Labels only decrease and always point inside the component, so the loop ends.
__device__ void od_union(int* L, int a, int b) {
  while (true) {
    a = od_find_live(L, a);
    b = od_find_live(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + b, a);
    if (old == b) return;
    b = old;
  }
}

__device__ __forceinline__ int od_popc_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int od_wave_min(int v) {
  for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int od_wave_max(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int od_wave_sum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exclusive scan of one int per thread over the workgroup (blockDim.x a multiple of 64, at most 1024); sh = 16 ints of LDS
__device__ int od_block_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wv] = x;
  __syncthreads();
  int before = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const int s = sh[w];
    if (w < wv) before += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return before + x - v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// 1 init, block b of a plane: class of every pixel, label = the first pixel of its class inside the block.  src = image n of a class
// map of `bytes` per element
__device__ __forceinline__ void od_init_block(const OdGeo& g, const void* __restrict__ src, int bytes, int n, int b,
                                              uint32_t* __restrict__ cls, int* __restrict__ L) {
  const int by = b / g.Wb, bx = b - by * g.Wb;
  uint32_t cw = 0;
  for (int i = 0; i < 4; ++i) {
    const int y = 2 * by + (i >> 1), x = 2 * bx + (i & 1);
    if (y >= g.H || x >= g.W) continue;
    const size_t idx = ((size_t)n * g.H + y) * g.W + x;
    const long long v = bytes == 1 ? (long long)((const uint8_t*)src)[idx] : (long long)((const int64_t*)src)[idx];
    if (v >= 1 && v < g.C) cw |= (uint32_t)v << (8 * i);
  }
  cls[b] = cw;
  int4 l;
  l.x = 4 * b + od_rep(cw, 0); l.y = 4 * b + od_rep(cw, 1); l.z = 4 * b + od_rep(cw, 2); l.w = 4 * b + od_rep(cw, 3);
  *reinterpret_cast<int4*>(L + 4 * b) = l;
}

// 2 merge, block b: the raster-backward neighbours (left, up-left, up, up-right) of every pixel cover every 8-neighbour edge once; edges
// inside the block were joined by init
__device__ __forceinline__ void od_merge_block(const OdGeo& g, int b, const uint32_t* __restrict__ cp, int* Lp) {
  const uint32_t cw = cp[b];
  if (!cw) return;
  const int by = b / g.Wb, bx = b - by * g.Wb;
  const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
  for (int i = 0; i < 4; ++i) {
    const int c = od_cls(cw, i);
    if (!c) continue;
    const int y = 2 * by + (i >> 1), x = 2 * bx + (i & 1);
    const int rep = 4 * b + od_rep(cw, i);
    for (int e = 0; e < 4; ++e) {
      const int ny = y + dy[e], nx = x + dx[e];
      if (ny < 0 || nx < 0 || nx >= g.W) continue;
      const int nb = (ny >> 1) * g.Wb + (nx >> 1);
      if (nb == b) continue;
      const int ni = (ny & 1) * 2 + (nx & 1);
      if (od_cls(cp[nb], ni) != c) continue;
      od_union(Lp, rep, 4 * nb + ni);
    }
  }
}

// 3 count, one tile (the OD_TILE threads tl = 0..OD_TILE-1 of block b = tile * OD_TILE + tl; wc = this tile's [OD_TILE / 64][OD_MAXC]
// ints of LDS): path compression; roots per class in this tile -> tcnt[tile].  Holds a workgroup barrier: every thread of the
// workgroup calls it the same number of times
__device__ __forceinline__ void od_count_tile(const OdGeo& g, int b, int tile, int tl, const uint32_t* __restrict__ cp, int* Lp,
                                              int* __restrict__ tcnt, int (*wc)[OD_MAXC]) {
  const int lane = tl & 63, wv = tl >> 6;
  const uint32_t cw = b < g.NB ? cp[b] : 0u;
  uint32_t roots = 0;   // bit c: this block holds the root of a class-c component (at most one per class)
  if (cw) {
    int4 l = *reinterpret_cast<const int4*>(Lp + 4 * b);
    int lv[4] = {l.x, l.y, l.z, l.w};
    for (int i = 0; i < 4; ++i) {
      const int c = od_cls(cw, i);
      if (!c) continue;
      int a = lv[i];
      while (true) { const int p = Lp[a]; if (p == a) break; a = p; }
      lv[i] = a;
      if (a == 4 * b + i) roots |= 1u << c;
    }
    *reinterpret_cast<int4*>(Lp + 4 * b) = make_int4(lv[0], lv[1], lv[2], lv[3]);
  }
  for (int c = 1; c < g.C; ++c) {
    const uint64_t m = __ballot((roots >> c) & 1u);
    if (lane == 0) wc[wv][c] = __popcll(m);
  }
  __syncthreads();
  if (tl < OD_MAXC) {
    const int c = tl;
    int s = 0;
    if (c >= 1 && c < g.C)
      for (int w = 0; w < OD_TILE / 64; ++w) s += wc[w][c];
    tcnt[(size_t)tile * OD_MAXC + c] = s;
  }
}

// 4 plane, the whole workgroup (NT threads) on one plane: tile offsets per class (scan), components per class -> pc[c], their gid base
// inside the plane -> pc[8 + c].  sh = 16, tot = OD_MAXC ints of LDS.  cnt != nullptr: the class's count also goes to cnt[(c - 1) * row]
template <int NT>
__device__ __forceinline__ void od_plane_scan(const OdGeo& g, const int* __restrict__ tcnt, int* __restrict__ toff, int* __restrict__ pc,
                                              int* __restrict__ cnt, int row, int* sh, int* tot) {
  for (int c = 1; c < g.C; ++c) {
    int carry = 0;
    for (int t0 = 0; t0 < g.tiles; t0 += NT) {
      const int t = t0 + threadIdx.x;
      const size_t at = (size_t)t * OD_MAXC + c;
      const int v = t < g.tiles ? tcnt[at] : 0;
      int total;
      const int ex = od_block_scan(v, sh, &total);
      if (t < g.tiles) toff[at] = carry + ex;
      carry += total;
    }
    if (threadIdx.x == 0) tot[c] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int base = 0;
    for (int c = 1; c < g.C; ++c) {
      pc[c] = tot[c];
      pc[8 + c] = base;
      base += tot[c];
      if (cnt) cnt[(size_t)(c - 1) * row] = tot[c];
    }
  }
}

// 5 rank, one tile (threads and wc as in count): R[root] = rank in block order among the roots of its class; the component's table
// entry (comp = the plane's first entry) is initialised.  Holds a workgroup barrier
__device__ __forceinline__ void od_rank_tile(const OdGeo& g, int b, int tile, int tl, const uint32_t* __restrict__ cp,
                                             const int* __restrict__ Lp, const int* __restrict__ toff, const int* __restrict__ pc,
                                             int* __restrict__ R, int* __restrict__ comp, int (*wc)[OD_MAXC]) {
  const int lane = tl & 63, wv = tl >> 6;
  const uint32_t cw = b < g.NB ? cp[b] : 0u;
  int rootq[OD_MAXC];
  uint32_t roots = 0;
  if (cw) {
    const int4 l = *reinterpret_cast<const int4*>(Lp + 4 * b);
    const int lv[4] = {l.x, l.y, l.z, l.w};
    for (int i = 0; i < 4; ++i) {
      const int c = od_cls(cw, i);
      if (c && lv[i] == 4 * b + i) { roots |= 1u << c; rootq[c] = 4 * b + i; }
    }
  }
  int below[OD_MAXC];
  for (int c = 1; c < g.C; ++c) {
    const uint64_t m = __ballot((roots >> c) & 1u);
    below[c] = od_popc_below(m);
    if (lane == 0) wc[wv][c] = __popcll(m);
  }
  __syncthreads();
  for (int c = 1; c < g.C; ++c) {
    if (!((roots >> c) & 1u)) continue;
    int rank = toff[(size_t)tile * OD_MAXC + c] + below[c];
    for (int w = 0; w < wv; ++w) rank += wc[w][c];
    R[rootq[c]] = rank;
    int* e = comp + ((size_t)pc[8 + c] + rank) * 8;
    *reinterpret_cast<int4*>(e) = make_int4(0x7fffffff, -1, 0x7fffffff, -1);
    *reinterpret_cast<int4*>(e + 4) = make_int4(0, 0, 0, 0);
  }
}

// area + bounding box of one group of pixels into its component; when every active lane of the wave hits the same component the wave
// reduces first and one lane does the atomics (a large blob would otherwise serialise thousands of atomics on one address)
__device__ void od_add_box(bool act, int gid, int area, int x0, int x1, int y0, int y1, int* comp) {
  const uint64_t am = __ballot(act);
  if (!am) return;
  const int lead = __ffsll((unsigned long long)am) - 1;
  const int lg = __shfl(gid, lead, 64);
  if (__ballot(act && gid == lg) == am) {
    const int a = od_wave_sum(act ? area : 0);
    const int ax0 = od_wave_min(act ? x0 : 0x7fffffff), ax1 = od_wave_max(act ? x1 : -1);
    const int ay0 = od_wave_min(act ? y0 : 0x7fffffff), ay1 = od_wave_max(act ? y1 : -1);
    if ((int)(threadIdx.x & 63) == lead) {
      int* e = comp + (size_t)lg * 8;
      atomicMin(e + CX0, ax0); atomicMax(e + CX1, ax1); atomicMin(e + CY0, ay0); atomicMax(e + CY1, ay1); atomicAdd(e + CAREA, a);
    }
  } else if (act) {
    int* e = comp + (size_t)gid * 8;
    atomicMin(e + CX0, x0); atomicMax(e + CX1, x1); atomicMin(e + CY0, y0); atomicMax(e + CY1, y1); atomicAdd(e + CAREA, area);
  }
}

// 6 stats (boxes), block b (`in` = b < NB, cw = its class word or 0, lv = its four compressed labels): area + bounding box per
// component into comp[gid], gid = gbase + pc[8 + c] + R[root].  Every thread of a wave runs the (uniform) slot loop, so the wave-level
// aggregation sees all lanes
__device__ __forceinline__ void od_stats_boxes(const OdGeo& g, bool in, int b, uint32_t cw, const int* lv, size_t gbase,
                                               const int* __restrict__ R, const int* __restrict__ pc, int* comp) {
  const int by = in ? b / g.Wb : 0, bx = in ? b - by * g.Wb : 0;
  // slot i: the pixels of the class of pixel i, when pixel i is the first of its class in the block
  for (int i = 0; i < 4; ++i) {
    const int c = od_cls(cw, i);
    const bool act = c != 0 && od_rep(cw, i) == i;
    int gid = 0, area = 0, x0 = 0x7fffffff, x1 = -1, y0 = 0x7fffffff, y1 = -1;
    if (act) {
      gid = (int)(gbase + pc[8 + c] + R[lv[i]]);
      for (int j = i; j < 4; ++j) {
        if (od_cls(cw, j) != c) continue;
        const int y = 2 * by + (j >> 1), x = 2 * bx + (j & 1);
        ++area; x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
      }
    }
    od_add_box(act, gid, area, x0, x1, y0, y1, comp);
  }
}

}  // namespace
