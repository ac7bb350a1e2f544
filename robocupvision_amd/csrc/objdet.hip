// RCV_OP_OBJECT_MATCH: the object-detection precision / recall counts of the reference's validation (test.py:28-89, getPrecRecall),
// for every image, every class 1..C-1 and K threshold pairs at once, on the device.
//
// Planes: plane 2n is image n of `pred`, plane 2n+1 image n of `target`; a pixel's class is its value when 1 <= v < C, else 0 (no plane).
// Pixels are addressed in BLOCK-MAJOR order, q = block * 4 + (y & 1) * 2 + (x & 1) with block = (y >> 1) * ceil(W/2) + (x >> 1).
//
//   1 init      class of every pixel, label = the first pixel of its class inside its 2x2 block (same-class pixels of one block are
//               8-adjacent); clears the pair hash table
//   2 merge     lock-free union-find over the 8-neighbour edges that leave the block, union toward the smaller index (atomicMin):
//               every component ends with its root at its smallest q, i.e. in its first block
//   3 count     path compression; roots of every class per tile of 256 blocks
//   4 plane     per plane: tile offsets per class (scan), components per class, their gid base; nPred / nTrue into the output
//   5 rank      rank of every root among the roots of its class in block order (= the component order of the contract)
//   6 stats     area + bounding box per component (integer atomics, aggregated per wave when the wave hits one component), and the
//               overlap pixels per (pred component, target component) pair into an integer hash table (aggregated per 2x2 block)
//   7-9 group   pairs per pred component (count, per-plane scan, scatter); the scatter evaluates the K IoU tests in fp64 once
//  10 match     one wave per (image, class, threshold, criterion): the greedy walk over the preds in rank order, "used" bitmask in LDS
//
// Integer atomics only; every output is a pure function of the inputs (the hash-table layout depends on scheduling, but the matcher
// takes the MINIMUM qualifying rank of a candidate list, so the order of the lists does not matter).  No host synchronisation.
#include <math.h>
#include "objdet_stages.h"

namespace {

constexpr int OD_MAXK = 8;
constexpr int OD_NO_MATCH = 0x7fffffff;

struct OdThr {
  double t[OD_MAXK];   // IoU thresholds, fp64 as given
  int s[OD_MAXK];      // distance thresholds as integer limits on s = dX^2 + dY^2 (X = x0 + x1 + 1): pass iff s <= s[k]
};

struct OdWs {
  uint64_t* hkey;   // [cap] pair key (pred gid + 1) << 32 | target gid; 0 = empty
  int* hcnt;        // [cap] overlap pixels of the pair
  uint32_t* cls;    // [2N][NB] four class bytes per 2x2 block
  int* L;           // [2N][QP] union-find parent (plane-local q)
  int* R;           // [2N][QP] rank of a root among the roots of its class
  int* comp;        // [2N * QP][8] component table, gid = plane * QP + class base + rank
  int* tcnt;        // [2N][tiles][8] roots per class and tile
  int* toff;        // [2N][tiles][8] exclusive offsets of the tiles per class
  int* pc;          // [2N][16] components per class, [8..15] their gid base inside the plane
  int2* cand;       // [N][QP] candidate lists: (target gid, bit k = IoU test k passes)
};

__host__ __device__ inline int round4(int a) { return (a + 3) & ~3; }
static inline size_t od_align(size_t b) { return (b + 255) & ~(size_t)255; }

// bytes of the workspace and (base != nullptr) the region pointers
static size_t od_layout(const OdGeo& g, uint64_t cap, char* base, OdWs* w) {
  const size_t P = (size_t)2 * g.N;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += od_align(bytes); return p; };
  char* hk = take(cap * 12);      // keys then counts: one contiguous region, cleared as one
  char* cl = take(P * g.NB * 4);
  char* l = take(P * g.QP * 4);
  char* r = take(P * g.QP * 4);
  char* cp = take(P * g.QP * 32);
  char* tc = take(P * g.tiles * 8 * 4);
  char* to = take(P * g.tiles * 8 * 4);
  char* pc = take(P * 16 * 4);
  char* cd = take((size_t)g.N * g.QP * 8);
  if (w) {
    w->hkey = (uint64_t*)hk; w->hcnt = (int*)(hk + cap * 8); w->cls = (uint32_t*)cl; w->L = (int*)l; w->R = (int*)r;
    w->comp = (int*)cp; w->tcnt = (int*)tc; w->toff = (int*)to; w->pc = (int*)pc; w->cand = (int2*)cd;
  }
  return off;
}

__device__ __forceinline__ uint32_t od_hash(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (uint32_t)k;
}

__device__ void od_insert(uint64_t* keys, int* cnt, uint32_t hmask, uint64_t key, int v) {
  uint32_t slot = od_hash(key) & hmask;
  while (true) {
    const uint64_t cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) break;
    if (cur == 0) {
      const uint64_t prev = atomicCAS((unsigned long long*)(keys + slot), 0ull, (unsigned long long)key);
      if (prev == 0 || prev == key) break;
    }
    slot = (slot + 1) & hmask;   // load factor <= 1/2 (capacity sized by the pair bound): a free slot always exists
  }
  atomicAdd(cnt + slot, v);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Stages 1-6 are the bodies of objdet_stages.h over 2N planes (plane 2n = pred, 2n + 1 = target of image n).
// 1 init: grid (tiles, 2N) x OD_TILE, one thread per 2x2 block; clears the pair hash table
__global__ __launch_bounds__(OD_TILE) void od_init_kernel(const void* __restrict__ pred, const void* __restrict__ target, OdGeo g,
                                                          uint32_t* __restrict__ cls, int* __restrict__ L, uint4* __restrict__ hclear,
                                                          size_t hwords) {
  const size_t tid = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * OD_TILE + threadIdx.x;
  const size_t nthr = (size_t)gridDim.x * gridDim.y * OD_TILE;
  for (size_t i = tid; i < hwords; i += nthr) hclear[i] = make_uint4(0u, 0u, 0u, 0u);
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  if (b >= g.NB) return;
  const bool tgt = pl & 1;
  od_init_block(g, tgt ? target : pred, tgt ? g.tbytes : g.pbytes, pl >> 1, b, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP);
}

// 2 merge
__global__ __launch_bounds__(OD_TILE) void od_merge_kernel(OdGeo g, const uint32_t* __restrict__ cls, int* L) {
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  if (b >= g.NB) return;
  od_merge_block(g, b, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP);
}

// 3 count
__global__ __launch_bounds__(OD_TILE) void od_count_kernel(OdGeo g, const uint32_t* __restrict__ cls, int* L, int* __restrict__ tcnt) {
  __shared__ int wc[OD_TILE / 64][OD_MAXC];
  const int pl = blockIdx.y;
  od_count_tile(g, blockIdx.x * OD_TILE + threadIdx.x, blockIdx.x, threadIdx.x, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP,
                tcnt + (size_t)pl * g.tiles * OD_MAXC, wc);
}

// 4 plane: grid 2N x 256; nPred / nTrue into the output
__global__ __launch_bounds__(256) void od_plane_kernel(OdGeo g, int K, const int* __restrict__ tcnt, int* __restrict__ toff,
                                                       int* __restrict__ pc, int* __restrict__ counts) {
  __shared__ int sh[16];
  __shared__ int tot[OD_MAXC];
  const int pl = blockIdx.x, row = 2 + 2 * K;
  od_plane_scan<256>(g, tcnt + (size_t)pl * g.tiles * OD_MAXC, toff + (size_t)pl * g.tiles * OD_MAXC, pc + pl * 16,
                     counts + (size_t)(pl >> 1) * (g.C - 1) * row + (pl & 1), row, sh, tot);
}

// 5 rank
__global__ __launch_bounds__(OD_TILE) void od_rank_kernel(OdGeo g, const uint32_t* __restrict__ cls, const int* __restrict__ L,
                                                          const int* __restrict__ toff, const int* __restrict__ pc, int* __restrict__ R,
                                                          int* __restrict__ comp) {
  __shared__ int wc[OD_TILE / 64][OD_MAXC];
  const int pl = blockIdx.y;
  od_rank_tile(g, blockIdx.x * OD_TILE + threadIdx.x, blockIdx.x, threadIdx.x, cls + (size_t)pl * g.NB, L + (size_t)pl * g.QP,
               toff + (size_t)pl * g.tiles * OD_MAXC, pc + pl * 16, R + (size_t)pl * g.QP, comp + (size_t)pl * g.QP * 8, wc);
}

__device__ void od_add_pair(bool act, uint64_t key, int v, uint64_t* keys, int* cnt, uint32_t hmask) {
  const uint64_t am = __ballot(act);
  if (!am) return;
  const int lead = __ffsll((unsigned long long)am) - 1;
  const uint64_t lk = __shfl(key, lead, 64);
  if (__ballot(act && key == lk) == am) {
    const int s = od_wave_sum(act ? v : 0);
    if ((int)(threadIdx.x & 63) == lead) od_insert(keys, cnt, hmask, lk, s);
  } else if (act) {
    od_insert(keys, cnt, hmask, key, v);
  }
}

// 6 stats: grid (tiles, 2N); area + bounding box per component, and the overlap pixels per (pred component, target component) pair into
// an integer hash table (aggregated per 2x2 block)
__global__ __launch_bounds__(OD_TILE) void od_stats_kernel(OdGeo g, const uint32_t* __restrict__ cls, const int* __restrict__ L,
                                                           const int* __restrict__ R, const int* __restrict__ pc, int* comp, uint64_t* hkey,
                                                           int* hcnt) {
  const int pl = blockIdx.y, b = blockIdx.x * OD_TILE + threadIdx.x;
  const bool in = b < g.NB;
  const uint32_t cw = in ? cls[(size_t)pl * g.NB + b] : 0u;
  const size_t pbase = (size_t)pl * g.QP;
  int4 l = make_int4(0, 0, 0, 0);
  if (cw) l = *reinterpret_cast<const int4*>(L + pbase + 4 * b);
  const int lv[4] = {l.x, l.y, l.z, l.w};
  od_stats_boxes(g, in, b, cw, lv, pbase, R + pbase, pc + pl * 16, comp);
  if (pl & 1) return;        // (uniform per workgroup) pairs are counted from the pred planes
  const uint32_t tw = in ? cls[(size_t)(pl + 1) * g.NB + b] : 0u;
  uint32_t both = 0;         // class bytes of the pixels where pred == target (>= 1)
  for (int i = 0; i < 4; ++i)
    if (od_cls(cw, i) && od_cls(cw, i) == od_cls(tw, i)) both |= (uint32_t)od_cls(cw, i) << (8 * i);
  int4 tl = make_int4(0, 0, 0, 0);
  if (both) tl = *reinterpret_cast<const int4*>(L + pbase + g.QP + 4 * b);
  const int tv[4] = {tl.x, tl.y, tl.z, tl.w};
  for (int i = 0; i < 4; ++i) {
    const int c = od_cls(both, i);
    const bool act = c != 0 && od_rep(both, i) == i;
    uint64_t key = 0;
    int v = 0;
    if (act) {
      const int pg = (int)(pbase + pc[pl * 16 + 8 + c] + R[pbase + lv[i]]);
      const int tg = (int)(pbase + g.QP + pc[(pl + 1) * 16 + 8 + c] + R[pbase + g.QP + tv[i]]);
      key = ((uint64_t)(pg + 1) << 32) | (uint32_t)tg;
      for (int j = i; j < 4; ++j) v += od_cls(both, j) == c;
    }
    od_add_pair(act, key, v, hkey, hcnt, g.hmask);
  }
}

// 7 group: candidates per pred component
__global__ void od_group_kernel(const uint64_t* __restrict__ hkey, uint32_t cap, int* comp) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
    const uint64_t k = hkey[s];
    if (k) atomicAdd(comp + (size_t)((k >> 32) - 1) * 8 + CCNT, 1);
  }
}

// 8 candidate offsets: grid N x 1024, exclusive scan over the components of pred plane 2n (gid order); image n owns cand[n*QP ..)
__global__ __launch_bounds__(1024) void od_cand_scan_kernel(OdGeo g, const int* __restrict__ pc, int* comp) {
  __shared__ int sh[16];
  const int pl = 2 * blockIdx.x;
  int ncomp = 0;
  for (int c = 1; c < g.C; ++c) ncomp += pc[pl * 16 + c];
  int* e0 = comp + (size_t)pl * g.QP * 8;
  int carry = blockIdx.x * g.QP;
  for (int j0 = 0; j0 < ncomp; j0 += 1024) {
    const int j = j0 + threadIdx.x;
    const int v = j < ncomp ? e0[(size_t)j * 8 + CCNT] : 0;
    int total;
    const int ex = od_block_scan(v, sh, &total);
    if (j < ncomp) e0[(size_t)j * 8 + COFF] = carry + ex;
    carry += total;
  }
}

// 9 scatter: (target gid, IoU test bits) into the pred component's list; inter / union in fp64 as numpy's true division
__global__ void od_scatter_kernel(const uint64_t* __restrict__ hkey, const int* __restrict__ hcnt, uint32_t cap, int K, OdThr thr, int* comp,
                                  int2* __restrict__ cand) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
    const uint64_t k = hkey[s];
    if (!k) continue;
    const int pg = (int)((k >> 32) - 1), tg = (int)(uint32_t)k;
    const int inter = hcnt[s];
    int* pe = comp + (size_t)pg * 8;
    const int uni = pe[CAREA] + comp[(size_t)tg * 8 + CAREA] - inter;
    const double iou = (double)inter / (double)uni;
    int mask = 0;
    for (int q = 0; q < K; ++q) mask |= (iou > thr.t[q]) ? (1 << q) : 0;
    const int pos = pe[COFF] + atomicAdd(pe + CCUR, 1);
    cand[pos] = make_int2(tg, mask);
  }
}

// words of the matcher's used bitmask: 2 per 64 blocks (a class has at most one component per block), rounded to 16 bytes
__host__ __device__ inline int od_used_words(int nb) { return round4((nb + 63) >> 6 << 1); }

// 10 match: one 64-lane workgroup per (image, class, k, criterion).  LDS: used bits (2 words per 64 targets, bits >= nt preset) and,
// for the distance criterion, the bounding box of the centres of every 64 consecutive targets (skips whole chunks per pred).
__global__ __launch_bounds__(64) void od_match_kernel(OdGeo g, int K, OdThr thr, const int* __restrict__ pc, const int* __restrict__ comp,
                                                      const int2* __restrict__ cand, int* __restrict__ counts) {
  extern __shared__ uint32_t od_sh[];
  const int lane = threadIdx.x;
  int id = blockIdx.x;
  const int crit = id & 1;
  id >>= 1;
  const int k = id % K;
  id /= K;
  const int c = id % (g.C - 1) + 1, n = id / (g.C - 1);
  const int pp = 2 * n, tp = 2 * n + 1;
  const int np = pc[pp * 16 + c], nt = pc[tp * 16 + c];
  const size_t pg0 = (size_t)pp * g.QP + pc[pp * 16 + 8 + c], tg0 = (size_t)tp * g.QP + pc[tp * 16 + 8 + c];
  const int nch = (nt + 63) >> 6;
  const int S = thr.s[k];
  uint32_t* used = od_sh;
  int4* box = reinterpret_cast<int4*>(od_sh + od_used_words(g.NB));
  int* out = counts + ((size_t)n * (g.C - 1) + c - 1) * (2 + 2 * K) + 2 + crit * K + k;
  if (np == 0 || nt == 0 || (crit == 1 && S < 0)) {
    if (lane == 0) *out = 0;
    return;
  }
  for (int w = lane; w < 2 * nch; w += 64) {
    const int lo = w * 32;
    used[w] = nt >= lo + 32 ? 0u : (nt <= lo ? ~0u : (~0u << (nt - lo)));
  }
  if (crit == 1) {
    for (int ch = 0; ch < nch; ++ch) {
      const int t = ch * 64 + lane;
      int X0 = 0x7fffffff, X1 = -1, Y0 = 0x7fffffff, Y1 = -1;
      if (t < nt) {
        const int4 bb = *reinterpret_cast<const int4*>(comp + (tg0 + t) * 8);
        X0 = X1 = bb.x + bb.y + 1;
        Y0 = Y1 = bb.z + bb.w + 1;
      }
      X0 = od_wave_min(X0); X1 = od_wave_max(X1); Y0 = od_wave_min(Y0); Y1 = od_wave_max(Y1);
      if (lane == 0) box[ch] = make_int4(X0, X1, Y0, Y1);
    }
  }
  __syncthreads();
  int count = 0;
  for (int p0 = 0; p0 < np; p0 += 64) {
    int4 pb = make_int4(0, 0, 0, 0), pa = make_int4(0, 0, 0, 0);
    if (p0 + lane < np) {
      const int* e = comp + (pg0 + p0 + lane) * 8;
      pb = *reinterpret_cast<const int4*>(e);
      pa = *reinterpret_cast<const int4*>(e + 4);
    }
    const int px = pb.x + pb.y + 1, py = pb.z + pb.w + 1;
    const int nloc = min(64, np - p0);
    for (int i = 0; i < nloc; ++i) {
      int best = OD_NO_MATCH;
      if (crit == 0) {
        const int cnt = __shfl(pa.y, i, 64), off = __shfl(pa.z, i, 64);
        for (int e0 = 0; e0 < cnt; e0 += 64) {
          if (e0 + lane < cnt) {
            const int2 v = cand[off + e0 + lane];
            const int tr = v.x - (int)tg0;
            if (((v.y >> k) & 1) && !((used[tr >> 5] >> (tr & 31)) & 1u)) best = min(best, tr);
          }
        }
        best = od_wave_min(best);
      } else {
        const int PX = __shfl(px, i, 64), PY = __shfl(py, i, 64);
        for (int g0 = 0; g0 < nch && best == OD_NO_MATCH; g0 += 64) {
          const int ch = g0 + lane;
          bool hit = false;
          if (ch < nch && (used[2 * ch] & used[2 * ch + 1]) != ~0u) {
            const int4 bx = box[ch];
            const long long ddx = max(0, max(bx.x - PX, PX - bx.y)), ddy = max(0, max(bx.z - PY, PY - bx.w));
            hit = ddx * ddx + ddy * ddy <= (long long)S;
          }
          uint64_t m = __ballot(hit);
          while (m) {
            const int chs = g0 + __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int t = chs * 64 + lane;
            bool ok = false;
            if (t < nt && !((used[t >> 5] >> (t & 31)) & 1u)) {
              const int4 bb = *reinterpret_cast<const int4*>(comp + (tg0 + t) * 8);
              const long long ex = bb.x + bb.y + 1 - PX, ey = bb.z + bb.w + 1 - PY;
              ok = ex * ex + ey * ey <= (long long)S;
            }
            const uint64_t mm = __ballot(ok);
            if (mm) { best = chs * 64 + __ffsll((unsigned long long)mm) - 1; break; }
          }
        }
      }
      if (best != OD_NO_MATCH) {
        if (lane == 0) used[best >> 5] |= 1u << (best & 31);
        ++count;
      }
      __syncthreads();
    }
  }
  if (lane == 0) *out = count;
}

// S = max{ s >= 0 : sqrt(s / 4.0) < d } with the correctly rounded host sqrt (-1: no s qualifies), clamped to smax (the largest s the
// plane can produce: every s <= smax then passes)
static int od_dist_limit(double d, long long smax) {
  if (!(d > 0.0)) return -1;
  if (d * d > (double)smax) return (int)smax;
  long long s = (long long)(4.0 * d * d);
  while (s >= 0 && !(sqrt((double)s / 4.0) < d)) --s;
  while (sqrt((double)(s + 1) / 4.0) < d) ++s;
  return (int)(s < smax ? s : smax);
}

}  // namespace

// --------------------------------------------------------------------------------------------
// launcher (RCV_OP_OBJECT_MATCH).  Record:
//   i: N, H, W; COUT = C (2..8); COUNT = K (1..8); INMODE / INMODE2 = element bytes of pred / target (1 = uint8, 8 = int64);
//      NPART = workspace size in 256-byte units (filled by the query)
//   p: IN = pred [N][H][W], IN2 = target [N][H][W], OUT = counts int32 [N][C-1][2+2K] (overwritten), PART = workspace,
//      X0 / X1 = HOST double[K] IoU / distance thresholds, read when the record is enqueued
// Every refusal that depends on the shape of the record (thresholds included) sits in front of the query return.
// --------------------------------------------------------------------------------------------
int rcv_launch_objdet(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  const char* what = "object_match";
  const int N = op->i[RCV_I_N], H = op->i[RCV_I_H], W = op->i[RCV_I_W], C = op->i[RCV_I_COUT], K = op->i[RCV_I_COUNT];
  const int pb = op->i[RCV_I_INMODE], tb = op->i[RCV_I_INMODE2];
  RCV_CHECK_ARG(C >= 2 && C <= OD_MAXC, "%s: %d classes unsupported (2..%d)", what, C, OD_MAXC);
  RCV_CHECK_ARG(K >= 1 && K <= OD_MAXK, "%s: %d threshold pairs unsupported (1..%d)", what, K, OD_MAXK);
  RCV_CHECK_ARG(pb == 1 || pb == 8, "%s: pred element size %d unsupported (1 = uint8, 8 = int64)", what, pb);
  RCV_CHECK_ARG(tb == 1 || tb == 8, "%s: target element size %d unsupported (1 = uint8, 8 = int64)", what, tb);
  RCV_CHECK_ARG((op->flags & ~RCV_F_SIDE_STREAM) == 0, "%s: flags 0x%x unsupported", what, op->flags & ~RCV_F_SIDE_STREAM);
  RCV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && N <= 32767 && H <= 8192 && W <= 8192, "%s: batch %d of %dx%d planes out of range", what,
                N, H, W);
  const long long NBl = (long long)((H + 1) / 2) * ((W + 1) / 2);
  RCV_CHECK_ARG(NBl <= OD_MAX_BLOCKS, "%s: a %dx%d plane is too large (at most %d 2x2 blocks)", what, H, W, OD_MAX_BLOCKS);
  RCV_CHECK_ARG(2.0 * N * 4.0 * (double)NBl < 2147483647.0, "%s: batch %d of %dx%d planes too large for 32-bit component ids", what, N, H, W);
  const double* it = (const double*)op->p[RCV_P_X0];
  const double* dt = (const double*)op->p[RCV_P_X1];
  RCV_CHECK_ARG(it && dt, "%s: threshold arrays (p[X0] IoU, p[X1] distance: host double[K]) missing", what);
  for (int k = 0; k < K; ++k) {
    RCV_CHECK_ARG(isfinite(it[k]) && it[k] >= 0.0, "%s: IoU threshold %d (%g) must be finite and >= 0", what, k, it[k]);
    RCV_CHECK_ARG(isfinite(dt[k]), "%s: distance threshold %d (%g) must be finite", what, k, dt[k]);
  }
  OdGeo g;
  g.N = N; g.H = H; g.W = W; g.C = C; g.Wb = (W + 1) / 2; g.NB = (int)NBl; g.QP = 4 * g.NB; g.tiles = ceil_div(g.NB, OD_TILE);
  g.pbytes = pb; g.tbytes = tb;
  // distinct (pred, target) pairs <= (2x2 block, class) groups of the pred planes: N * NB * min(4, C-1); capacity >= twice that
  const uint64_t pairs = (uint64_t)N * g.NB * (uint64_t)(C - 1 < 4 ? C - 1 : 4);
  uint64_t cap = 64;
  while (cap < 2 * pairs) cap <<= 1;
  g.hmask = (uint32_t)(cap - 1);
  const size_t bytes = od_layout(g, cap, nullptr, nullptr);
  RCV_CHECK_ARG(bytes / 256 < 2147483647ull, "%s: workspace too large", what);
  if (query) {
    snprintf(query->label, sizeof(query->label), "object_match<%s,%s>", pb == 1 ? "u8" : "i64", tb == 1 ? "u8" : "i64");
    query->n_part = (int)(bytes / 256);
    query->part_bytes = bytes;
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN] && op->p[RCV_P_IN2] && op->p[RCV_P_OUT], "%s: null operand", what);
  RCV_CHECK_ARG(op->p[RCV_P_PART] && ((uintptr_t)op->p[RCV_P_PART] & 255) == 0, "%s: workspace missing or not 256-byte aligned", what);
  RCV_CHECK_ARG(op->i[RCV_I_NPART] == (int)(bytes / 256), "%s: workspace of %d x 256 bytes given, %zu expected (rcv_op_workspace)", what,
                op->i[RCV_I_NPART], bytes / 256);
  OdThr thr;
  memset(&thr, 0, sizeof(thr));
  const long long smax = 4LL * ((long long)(W - 1) * (W - 1) + (long long)(H - 1) * (H - 1));
  for (int k = 0; k < K; ++k) { thr.t[k] = it[k]; thr.s[k] = od_dist_limit(dt[k], smax); }
  OdWs w;
  od_layout(g, cap, (char*)op->p[RCV_P_PART], &w);
  int* counts = (int*)op->p[RCV_P_OUT];
  const dim3 grid(g.tiles, 2 * N);
  hipLaunchKernelGGL(od_init_kernel, grid, dim3(OD_TILE), 0, s, op->p[RCV_P_IN], op->p[RCV_P_IN2], g, w.cls, w.L, (uint4*)w.hkey,
                     (size_t)(cap * 12 / 16));
  hipLaunchKernelGGL(od_merge_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L);
  hipLaunchKernelGGL(od_count_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.tcnt);
  hipLaunchKernelGGL(od_plane_kernel, dim3(2 * N), dim3(256), 0, s, g, K, w.tcnt, w.toff, w.pc, counts);
  hipLaunchKernelGGL(od_rank_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.toff, w.pc, w.R, w.comp);
  hipLaunchKernelGGL(od_stats_kernel, grid, dim3(OD_TILE), 0, s, g, w.cls, w.L, w.R, w.pc, w.comp, w.hkey, w.hcnt);
  size_t sg = (cap + 255) / 256;
  if (sg > (size_t)h->num_cus * 8) sg = (size_t)h->num_cus * 8;
  hipLaunchKernelGGL(od_group_kernel, dim3((unsigned)sg), dim3(256), 0, s, w.hkey, (uint32_t)cap, w.comp);
  hipLaunchKernelGGL(od_cand_scan_kernel, dim3(N), dim3(1024), 0, s, g, w.pc, w.comp);
  hipLaunchKernelGGL(od_scatter_kernel, dim3((unsigned)sg), dim3(256), 0, s, w.hkey, w.hcnt, (uint32_t)cap, K, thr, w.comp, w.cand);
  const size_t lds = (size_t)od_used_words(g.NB) * 4 + (size_t)((g.NB + 63) >> 6) * 16;
  hipLaunchKernelGGL(od_match_kernel, dim3(N * (C - 1) * K * 2), dim3(64), lds, s, g, K, thr, w.pc, w.comp, w.cand, counts);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
