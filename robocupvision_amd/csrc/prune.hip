// RCV_OP_PRUNE: the three magnitude-pruning mask builders of the reference (model.py:45-57 pruneModelNew, :621-642 pruneModel,
// :644-672 pruneModel2) for every weight tensor of a model in ONE launch, one workgroup per tensor.
//
// The reference asks the device for two or three scalars per tensor (`float(torch.sum(...))`, and two more per step of pruneModel's
// threshold search): ~100 host round trips per model.  Here a workgroup owns a tensor from the first pass to the last: every
// quantity that decides something is an integer count, a maximum, or a float64 sum taken in a fixed order, so the result does not
// depend on how the workgroups are scheduled, and nothing is reduced across workgroups.  The largest weight tensor of any net in
// this project is below 150 k floats: it stays in L2 over the few passes a rule needs.  20-70 workgroups leave most of the chip
// idle; the op runs once per prune round, and what it removes is host syncs, not device time.
//
// A tensor may start at any 4-byte boundary (the engine lays the parameters out back to back in one flat buffer), so the counting
// passes peel to 16-byte alignment before they read float4s.  The two float64 passes of rule 1 and every pass that writes are plain
// index-strided loops: their order must not depend on the address.
#include "rcv_internal.h"

namespace {

constexpr int PRUNE_THREADS = 1024;
constexpr int PRUNE_WAVES = PRUNE_THREADS / 64;

__device__ __forceinline__ uint32_t key_of(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// f(value) for every element of w[0..n), each exactly once, in no particular order: float4 reads behind a scalar head of <= 3
// elements (up to the first 16-byte boundary) and ahead of a scalar tail of <= 3
template <typename F>
__device__ __forceinline__ void for_each_value(const float* w, uint32_t n, F f) {
  uint32_t head = (uint32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(w) & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const uint32_t n4 = (n - head) >> 2;
  const float4* w4 = reinterpret_cast<const float4*>(w + head);
  for (uint32_t i = threadIdx.x; i < n4; i += PRUNE_THREADS) {
    const float4 v = w4[i];
    f(v.x); f(v.y); f(v.z); f(v.w);
  }
  if (threadIdx.x < head) f(w[threadIdx.x]);
  for (uint32_t i = head + 4u * n4 + threadIdx.x; i < n; i += PRUNE_THREADS) f(w[i]);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                   // lane 0 holds the sum
}

// Sums of a and b over the workgroup, returned to every thread.  buf: 2 * PRUNE_WAVES words; two barriers, so the buffer can be
// reused by the next call at once.
__device__ __forceinline__ void block_sum2(uint32_t& a, uint32_t& b, uint32_t* buf) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  a = wave_sum(a); b = wave_sum(b);
  if (lane == 0) { buf[wv] = a; buf[PRUNE_WAVES + wv] = b; }
  __syncthreads();
  uint32_t sa = 0, sb = 0;
  for (int k = 0; k < PRUNE_WAVES; ++k) { sa += buf[k]; sb += buf[PRUNE_WAVES + k]; }
  __syncthreads();
  a = sa; b = sb;
}

// Sum of v over the workgroup in a fixed binary tree, returned to every thread.  buf: PRUNE_THREADS doubles.
__device__ __forceinline__ double block_sum_d(double v, double* buf) {
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int s = PRUNE_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) buf[threadIdx.x] += buf[threadIdx.x + s];
    __syncthreads();
  }
  const double r = buf[0];
  __syncthreads();
  return r;
}

// #(|w| < thresh) and #(w != 0): the two numbers of the reference's `Pruned %f%%` line
__device__ __forceinline__ void count_below_nonzero(const float* w, uint32_t n, float thresh, uint32_t& below, uint32_t& nonzero, uint32_t* buf) {
  uint32_t cb = 0, nz = 0;
  for_each_value(w, n, [&](float v) { cb += fabsf(v) < thresh ? 1u : 0u; nz += v != 0.f ? 1u : 0u; });
  block_sum2(cb, nz, buf);
  below = cb; nonzero = nz;
}

// param[|param| < thresh] = 0; mask = |param| < thresh afterwards (for thresh > 0 that is the same set; for thresh <= 0 it is empty)
__device__ __forceinline__ void zero_below(float* w, uint8_t* mask, uint32_t n, float thresh) {
  for (uint32_t i = threadIdx.x; i < n; i += PRUNE_THREADS) {
    const bool below = fabsf(w[i]) < thresh;
    if (below) w[i] = 0.f;
    mask[i] = below ? 1 : 0;
  }
}

__global__ __launch_bounds__(PRUNE_THREADS) void prune_kernel(rcv_prune_job* __restrict__ jobs, int rule) {
  __shared__ double s_d[PRUNE_THREADS];
  __shared__ uint32_t s_u[2 * PRUNE_WAVES];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_sel[3];                 // radix select: chosen digit, its count, rank left inside it
  __shared__ uint32_t s_tie[2][PRUNE_WAVES];

  rcv_prune_job* job = jobs + blockIdx.x;
  float* w = job->w;
  uint8_t* mask = job->mask;
  const int64_t n64 = job->n;
  const int64_t amount64 = job->amount;
  auto finish = [&](float thresh, int64_t r0, int64_t r1, int64_t r2, int64_t status) {
    if (threadIdx.x == 0) {
      job->thresh = thresh;
      job->result[0] = r0; job->result[1] = r1; job->result[2] = r2; job->result[3] = status;
    }
  };
  // what rcv_prune_check refuses never touches memory here either (every test below is uniform over the workgroup)
  const bool bad = w == nullptr || mask == nullptr || (reinterpret_cast<uintptr_t>(w) & 3u) != 0 || n64 < 1 || n64 >= ((int64_t)1 << 31) ||
                   (rule == RCV_PRUNE_STD_SEARCH && n64 < 2) || (rule == RCV_PRUNE_SMALLEST_K && (amount64 < 0 || amount64 > n64)) ||
                   rule < RCV_PRUNE_MAX_RATIO || rule > RCV_PRUNE_SMALLEST_K;
  if (bad) { finish(0.f, 0, 0, 0, RCV_PRUNE_ST_BAD_JOB); return; }
  const uint32_t n = (uint32_t)n64;

  if (rule == RCV_PRUNE_MAX_RATIO) {
    // thresh = torch.max(torch.abs(param)) * ratio: a maximum is order free; NaN is outside the contract (fmaxf drops it)
    float mx = 0.f;
    for_each_value(w, n, [&](float v) { mx = fmaxf(mx, fabsf(v)); });
    uint32_t a = __float_as_uint(mx);                 // non-negative floats order as their bit patterns
    for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_down(a, o, 64));
    if ((threadIdx.x & 63) == 0) s_u[threadIdx.x >> 6] = a;
    __syncthreads();
    a = 0;
    for (int k = 0; k < PRUNE_WAVES; ++k) a = max(a, s_u[k]);
    __syncthreads();
    const float thresh = __fmul_rn(__uint_as_float(a), job->ratio);
    uint32_t below, nonzero;
    count_below_nonzero(w, n, thresh, below, nonzero, s_u);
    zero_below(w, mask, n, thresh);
    finish(thresh, below, nonzero, 0, RCV_PRUNE_ST_OK);
    return;
  }

  if (rule == RCV_PRUNE_STD_SEARCH) {
    // param.std(): unbiased, mean and squared deviations in float64, two passes, thread t owning the indices t (mod 1024) and a
    // fixed tree over the threads -- the order depends on nothing but n
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += PRUNE_THREADS) acc += (double)w[i];
    const double mean = block_sum_d(acc, s_d) / (double)n;
    acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += PRUNE_THREADS) { const double d = (double)w[i] - mean; acc += d * d; }
    const double ssq = block_sum_d(acc, s_d);
    float thresh = (float)sqrt(ssq / (double)(n - 1));
    const double lower = job->lower, upper = job->upper;
    const float up = 1.025f, down = 0.975f;           // `thresh *= 1.025` on a 0-dim fp32 tensor: an fp32 multiply by fp32(1.025)
    uint32_t below = 0, nonzero = 0;
    int it = 0;
    int64_t status = RCV_PRUNE_ST_NO_END;
    for (; it < RCV_PRUNE_MAX_ITER; ++it) {           // every quantity in the loop is uniform over the workgroup
      count_below_nonzero(w, n, thresh, below, nonzero, s_u);
      if (nonzero == 0) { status = RCV_PRUNE_ST_ALL_ZERO; break; }
      const double num = (double)below / (double)nonzero * 100.0;
      if (num < lower) thresh = __fmul_rn(thresh, up);
      else if (num > upper) thresh = __fmul_rn(thresh, down);
      else { status = RCV_PRUNE_ST_OK; break; }
    }
    if (status == RCV_PRUNE_ST_OK) zero_below(w, mask, n, thresh);
    finish(thresh, below, nonzero, it, status);
    return;
  }

  // RCV_PRUNE_SMALLEST_K: the amount-th smallest key (|w| as its bit pattern: monotone for non-NaN floats) by radix select, top
  // digit first; every round keeps the prefix found so far and the rank left inside it
  const uint32_t amount = (uint32_t)amount64;
  uint32_t nz = 0, dummy = 0;
  for_each_value(w, n, [&](float v) { nz += key_of(v) != 0u ? 1u : 0u; });
  block_sum2(nz, dummy, s_u);
  uint32_t T = 0, need = 0;                            // need = how many of the elements with key == T go
  if (amount > 0) {
    uint32_t prefix = 0, prefix_mask = 0, rank = amount;     // rank is 1-based among the elements that match the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
      __syncthreads();
      for_each_value(w, n, [&](float v) {
        const uint32_t k = key_of(v);
        if ((k & prefix_mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
      });
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t seen = 0, d = 0;
        for (; d < 255u; ++d) {                        // rank <= #matching elements, so the walk ends inside the table
          if (seen + s_hist[d] >= rank) break;
          seen += s_hist[d];
        }
        s_sel[0] = d; s_sel[1] = s_hist[d]; s_sel[2] = rank - seen;
      }
      __syncthreads();
      prefix |= s_sel[0] << shift;
      prefix_mask |= 255u << shift;
      rank = s_sel[2];
      __syncthreads();
    }
    T = prefix; need = rank;
  }
  // zero key < T everywhere and, among key == T, the `need` lowest flat indices: chunks of 1024 consecutive elements in index
  // order, an exclusive count of the ties ahead of every element (ballot inside the wave, wave totals through LDS)
  uint32_t ties_before = 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int par = 0;
  for (uint32_t base = 0; base < n; base += PRUNE_THREADS, par ^= 1) {
    const uint32_t i = base + threadIdx.x;
    const bool in = i < n;
    const float v = in ? w[i] : 0.f;
    const uint32_t k = key_of(v);
    const bool tie = in && amount > 0 && k == T;
    const unsigned long long b = __ballot(tie);
    if (lane == 0) s_tie[par][wv] = (uint32_t)__popcll(b);
    __syncthreads();                                   // (the other half of s_tie is written next round: one barrier per chunk)
    uint32_t ahead = ties_before, total = 0;
    for (int q = 0; q < PRUNE_WAVES; ++q) { const uint32_t c = s_tie[par][q]; if (q < wv) ahead += c; total += c; }
    ahead += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    ties_before += total;
    if (in) {
      const bool zero = amount > 0 && (k < T || (tie && ahead < need));
      if (zero) w[i] = 0.f;
      mask[i] = (zero || k == 0u) ? 1 : 0;             // indices.append(param == 0.0): weights that were zero already are in the mask
    }
  }
  finish(__uint_as_float(T), amount, nz, 0, RCV_PRUNE_ST_OK);
}

}  // namespace

int rcv_launch_prune(const rcv_handle* h, const rcv_op* op, hipStream_t s, OpQuery* query) {
  (void)h;
  const int count = op->i[RCV_I_COUNT], rule = op->i[RCV_I_AUX0];
  RCV_CHECK_ARG(rule >= RCV_PRUNE_MAX_RATIO && rule <= RCV_PRUNE_SMALLEST_K, "prune: rule %d unknown (0 = pruneModelNew, 1 = pruneModel, 2 = pruneModel2)", rule);
  RCV_CHECK_ARG(count > 0 && count <= 65535, "prune: %d jobs (1..65535)", count);
  if (query) {
    query->n_part = 0; query->n_split = 0; query->part_bytes = 0;
    snprintf(query->label, sizeof(query->label), "prune<%d>", rule);
    return RCV_OK;
  }
  RCV_CHECK_ARG(op->p[RCV_P_IN], "prune: null job table");
  hipLaunchKernelGGL(prune_kernel, dim3(count), dim3(PRUNE_THREADS), 0, s, (rcv_prune_job*)op->p[RCV_P_IN], rule);
  RCV_HIP(hipGetLastError());
  return RCV_OK;
}
