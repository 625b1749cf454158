// Isoenergetic (Houdayer) cluster moves on resumable chains (include/asp.h section 4, DESIGN.md §4.13,
// law "ASP-ICM-1"): two chains of a handle flip one connected component of the sites on which their
// current configurations differ — the seed site from one Philox draw, the component by a
// level-synchronous search on the graph of A induced on the differing sites, the energy change of the
// flip as the sum of the annealer's own fixed-point proposal energies (§4.4-4.5) over the component.
// A workgroup per pair — or, for the small models of a batch (asp_sa_chains_cluster_move_batch), a
// wavefront per pair —; everything after the row sums is integer arithmetic, and the component is a
// set, so no traversal or reduction order can change a result.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "asp_common.hpp"
#include "sa_device.hpp"
#include "sa_internal.hpp"

namespace {

using namespace asp::dev;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kSharedRow = 64;  // a longer row of A is walked by the whole wavefront
constexpr size_t kStaticLds = 2048;  // what the kernel declares beside the planes (scan scratch, sums), rounded up

struct ClusterArgs {
  const uint32_t *row_ptr;  // [K + 1] rows of A over ORIGINAL indices (csr of plan->host)
  const uint32_t *col;      // ascending in a row
  const double *val;
  const double *field;      // [K], original order
  uint64_t *x_cur, *x_best;       // [R][W]
  long long *e_cur, *e_best;      // [R]
  const uint32_t *pairs;          // [2 P], validated on the host
  uint32_t *hbm_planes;           // HBM form: [P][3][2 W] words (d | member | frontier); else unused
  uint64_t *back;  // n | size << 32 [P], Q [P], tracked_current of (a, b) [2 P]: what the host reads back
  uint64_t seed;
  double scale;  // 2^S
  uint32_t num_spins, words, num_pairs, sweeps_done, draw;
};

// The same for ONE pair: what a workgroup (or a wavefront) needs for its move, wherever it comes from —
// made from ClusterArgs and the pair's index by the single call's kernel, a row of the uploaded table
// in a batch (one row per (item, pair); the rows of a launch class are contiguous).
struct ClusterRow {
  const uint32_t *row_ptr, *col;
  const double *val, *field;
  uint64_t *x_cur, *x_best;
  long long *e_cur, *e_best;
  uint32_t *hbm_planes;  // HBM form: THIS pair's [3][2 W] words; else unused
  uint64_t *back;  // n | size << 32 [back_count], Q [back_count], tracked_current of (a, b) [2 back_count]
  uint64_t seed;
  double scale;
  uint32_t num_spins, words, slot_a, slot_b, sweeps_done, draw;
  uint32_t back_at, back_count;  // the pair's place in `back`
};

__device__ __forceinline__ ClusterRow row_of(const ClusterArgs &a, uint32_t pair) {
  return ClusterRow{a.row_ptr, a.col, a.val, a.field, a.x_cur, a.x_best, a.e_cur, a.e_best,
                    a.hbm_planes ? a.hbm_planes + static_cast<uint64_t>(pair) * 6u * a.words : nullptr,
                    a.back, a.seed, a.scale, a.num_spins, a.words, a.pairs[2u * pair], a.pairs[2u * pair + 1u],
                    a.sweeps_done, a.draw, pair, a.num_pairs};
}

// What the host reads back for the pair (one thread).
__device__ __forceinline__ void report(const ClusterRow &a, uint32_t n, uint32_t size, long long Q, long long ea,
                                       long long eb) {
  const uint64_t T = a.back_count;
  a.back[a.back_at] = static_cast<uint64_t>(n) | (static_cast<uint64_t>(size) << 32);
  a.back[T + a.back_at] = static_cast<uint64_t>(Q);
  a.back[2ull * T + 2u * a.back_at] = static_cast<uint64_t>(ea);
  a.back[2ull * T + 2u * a.back_at + 1u] = static_cast<uint64_t>(eb);
}

// The three bit planes as 32-bit words (spin i: word i >> 5, bit i & 31 — the low and the high half
// of the configuration's 64-bit word).  LDS: plain accesses and workgroup-scope atomics.  HBM: every
// access is an agent-scope atomic, so a word that another wavefront changed with an atomic OR (done
// in the L2) is never read from a stale line of this CU's vector cache.
template <bool HBM>
struct Planes {
  uint32_t *base;
  __device__ __forceinline__ uint32_t load(uint32_t at) const {
    if constexpr (HBM) return __hip_atomic_load(base + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base[at];
  }
  __device__ __forceinline__ void store(uint32_t at, uint32_t v) const {
    if constexpr (HBM) {
      __hip_atomic_store(base + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      base[at] = v;
    }
  }
  __device__ __forceinline__ uint32_t fetch_or(uint32_t at, uint32_t v) const {
    return __hip_atomic_fetch_or(base + at, v, __ATOMIC_RELAXED,
                                 HBM ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ uint32_t take(uint32_t at) const {
    return __hip_atomic_exchange(base + at, 0u, __ATOMIC_RELAXED,
                                 HBM ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// q_i of step 4 for a member i of the component: the fixed-point proposal energy of site i in replica a
// against the sites with d = 0 (a neighbour with d = 1 belongs to the component itself).
template <typename P>
__device__ __forceinline__ long long member_energy(const ClusterRow &a, const P &planes, uint32_t D,
                                                   const uint64_t *xa, uint32_t i) {
  double acc = 0.0;
  const uint32_t begin = a.row_ptr[i], end = a.row_ptr[i + 1u];
  uint32_t k = begin;
  // four entries at a time: their loads are in flight together, the sum keeps the column order
  for (; k + 4u <= end; k += 4u) {
    uint32_t j[4], dw[4];
    double v[4];
    uint64_t x[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      j[t] = a.col[k + t];
      v[t] = a.val[k + t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      x[t] = xa[j[t] >> 6];
      dw[t] = planes.load(D + (j[t] >> 5));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (((dw[t] >> (j[t] & 31u)) & 1u) != 0u) continue;
      acc = __builtin_fma(v[t], ((x[t] >> (j[t] & 63u)) & 1ull) != 0ull ? 1.0 : -1.0, acc);
    }
  }
  for (; k < end; ++k) {
    const uint32_t j = a.col[k];
    if (((planes.load(D + (j >> 5)) >> (j & 31u)) & 1u) != 0u) continue;
    const bool up = ((xa[j >> 6] >> (j & 63u)) & 1ull) != 0ull;
    acc = __builtin_fma(a.val[k], up ? 1.0 : -1.0, acc);
  }
  const double g = __dadd_rn(acc, a.field[i]);
  const bool up = ((xa[i >> 6] >> (i & 63u)) & 1ull) != 0ull;
  const double de = __dmul_rn(up ? -2.0 : 2.0, g);
  // rint(dE * 2^S): |dE * 2^S| < 2^51
  return __double_as_longlong(__dadd_rn(__dmul_rn(de, a.scale), 0x1.8p52)) - 0x4338000000000000ll;
}

// Steps 1-6 of ASP-ICM-1 for the pair of row `a`, by a whole workgroup (the single call's kernel and
// the two workgroup classes of a batch); lds_planes: the dynamic LDS (unused in the HBM form).
template <bool HBM>
__device__ __forceinline__ void cluster_move_pair(const ClusterRow &a, uint64_t *lds_planes) {
  __shared__ uint32_t s_scan[kThreads];
  __shared__ unsigned long long s_q;
  __shared__ uint32_t s_size;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t K = a.num_spins, W = a.words, W2 = 2u * W;
  const uint32_t sa = a.slot_a, sb = a.slot_b;
  uint64_t *xa = a.x_cur + static_cast<uint64_t>(sa) * W;
  uint64_t *xb = a.x_cur + static_cast<uint64_t>(sb) * W;
  const Planes<HBM> planes{HBM ? a.hbm_planes : reinterpret_cast<uint32_t *>(lds_planes)};
  const uint32_t D = 0u, M = W2, F = 2u * W2;  // word offsets of d, member, frontier
  if (tid == 0) {
    s_q = 0ull;
    s_size = 0u;
  }

  // ---- step 1: d = x_a xor x_b; thread t owns the words [t per, (t + 1) per) ----
  const uint64_t tail = (K & 63u) ? (1ull << (K & 63u)) - 1ull : ~0ull;
  const uint32_t per = (W + kThreads - 1u) / kThreads;
  const uint32_t first = tid * per < W ? tid * per : W;
  const uint32_t last = first + per < W ? first + per : W;
  uint32_t mine = 0;
  for (uint32_t w = first; w < last; ++w) {
    uint64_t d = xa[w] ^ xb[w];
    if (w + 1u == W) d &= tail;
    planes.store(D + 2u * w, static_cast<uint32_t>(d));
    planes.store(D + 2u * w + 1u, static_cast<uint32_t>(d >> 32));
    planes.store(M + 2u * w, 0u);
    planes.store(M + 2u * w + 1u, 0u);
    planes.store(F + 2u * w, 0u);
    planes.store(F + 2u * w + 1u, 0u);
    mine += static_cast<uint32_t>(__popcll(d));
  }
  s_scan[tid] = mine;
  __syncthreads();
  for (uint32_t step = 1; step < kThreads; step <<= 1) {
    const uint32_t add = tid >= step ? s_scan[tid - step] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  const uint32_t n = s_scan[kThreads - 1u];
  if (n == 0u) {  // (uniform) identical replicas: nothing changes for the pair
    if (tid == 0) report(a, 0u, 0u, 0ll, a.e_cur[sa], a.e_cur[sb]);
    return;
  }

  // ---- step 2: the U-th differing site, U = floor(v n / 2^32) ----
  const Philox4 rnd = philox4x32_10(sa, a.sweeps_done, 0xFFFFFFFBu, a.draw, static_cast<uint32_t>(a.seed),
                                    static_cast<uint32_t>(a.seed >> 32));
  const uint32_t U = __umulhi(rnd.w[0], n);
  const uint32_t before = s_scan[tid] - mine;
  if (U >= before && U < before + mine) {  // exactly one thread
    uint32_t skip = U - before;
    for (uint32_t w = first; w < last; ++w) {
      uint64_t d = static_cast<uint64_t>(planes.load(D + 2u * w)) |
                   (static_cast<uint64_t>(planes.load(D + 2u * w + 1u)) << 32);
      const uint32_t here = static_cast<uint32_t>(__popcll(d));
      if (skip >= here) {
        skip -= here;
        continue;
      }
      for (; skip != 0u; --skip) d &= d - 1ull;
      const uint32_t i0 = w * 64u + static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(d)) - 1);
      planes.store(M + (i0 >> 5), 1u << (i0 & 31u));
      planes.store(F + (i0 >> 5), 1u << (i0 & 31u));
      break;
    }
  }
  __syncthreads();

  // ---- step 3: the component, level by level; a round takes the frontier's bits and sets the next ----
  auto visit = [&](uint32_t j) -> uint32_t {
    const uint32_t wj = j >> 5, bj = 1u << (j & 31u);
    if ((planes.load(D + wj) & bj) == 0u) return 0u;
    if ((planes.load(M + wj) & bj) != 0u) return 0u;
    if ((planes.fetch_or(M + wj, bj) & bj) != 0u) return 0u;  // (somebody else was first)
    planes.fetch_or(F + wj, bj);
    return 1u;
  };
  for (;;) {
    uint32_t added = 0;
    for (uint32_t base = wave * 64u; base < W2; base += kThreads) {  // (uniform over the wavefront)
      const uint32_t w = base + lane;
      uint32_t f = 0;
      if (w < W2 && planes.load(F + w) != 0u) f = planes.take(F + w);
      uint32_t shared_rows = 0;
      while (f != 0u) {
        const uint32_t bit = static_cast<uint32_t>(__ffs(f) - 1);
        f &= f - 1u;
        const uint32_t i = w * 32u + bit;
        const uint32_t begin = a.row_ptr[i], end = a.row_ptr[i + 1u];
        if (end - begin > kSharedRow) {
          shared_rows |= 1u << bit;
          continue;
        }
        uint32_t k = begin;
      for (; k + 4u <= end; k += 4u) {  // (four columns in flight together)
        const uint32_t j0 = a.col[k], j1 = a.col[k + 1u], j2 = a.col[k + 2u], j3 = a.col[k + 3u];
        added |= visit(j0) | visit(j1) | visit(j2) | visit(j3);
      }
      for (; k < end; ++k) added |= visit(a.col[k]);
      }
      // long rows, one at a time: the lanes stride the row
      uint64_t waiting = __ballot(shared_rows != 0u);
      while (waiting != 0ull) {
        const int leader = __ffsll(static_cast<unsigned long long>(waiting)) - 1;
        const uint32_t theirs = __shfl(shared_rows, leader);
        const uint32_t bit = static_cast<uint32_t>(__ffs(theirs) - 1);
        if (static_cast<int>(lane) == leader) shared_rows &= shared_rows - 1u;
        const uint32_t i = (base + static_cast<uint32_t>(leader)) * 32u + bit;
        const uint32_t begin = a.row_ptr[i], end = a.row_ptr[i + 1u];
        for (uint32_t k = begin + lane; k < end; k += 64u) added |= visit(a.col[k]);
        waiting = __ballot(shared_rows != 0u);
      }
    }
    if (__syncthreads_or(static_cast<int>(added)) == 0) break;
  }

  // ---- step 4: Q = sum over the component of the fixed-point proposal energies ----
  long long q_sum = 0;
  uint32_t members = 0;
  for (uint32_t i = tid; i < K; i += kThreads) {
    if (((planes.load(M + (i >> 5)) >> (i & 31u)) & 1u) == 0u) continue;
    members += 1u;
    q_sum += member_energy(a, planes, D, xa, i);
  }
  for (int offset = 32; offset != 0; offset >>= 1) {
    q_sum += __shfl_xor(q_sum, offset);
    members += __shfl_xor(members, offset);
  }
  if (lane == 0 && members != 0u) {
    atomicAdd(&s_q, static_cast<unsigned long long>(q_sum));
    atomicAdd(&s_size, members);
  }
  // (every thread reads the tracked energies before thread 0 replaces them)
  const long long ea_old = a.e_cur[sa], eb_old = a.e_cur[sb];
  const long long best_a = a.e_best[sa], best_b = a.e_best[sb];
  __syncthreads();
  const long long Q = static_cast<long long>(s_q);
  const long long ea = ea_old + Q, eb = eb_old - Q;
  const bool improves_a = ea < best_a, improves_b = eb < best_b;

  // ---- steps 5 and 6: flip the component in both chains; a strictly lower tracked energy is the best ----
  uint64_t *best_xa = a.x_best + static_cast<uint64_t>(sa) * W;
  uint64_t *best_xb = a.x_best + static_cast<uint64_t>(sb) * W;
  for (uint32_t w = tid; w < W; w += kThreads) {
    const uint64_t m = static_cast<uint64_t>(planes.load(M + 2u * w)) |
                       (static_cast<uint64_t>(planes.load(M + 2u * w + 1u)) << 32);
    const uint64_t na = xa[w] ^ m, nb = xb[w] ^ m;
    if (m != 0ull) {
      xa[w] = na;
      xb[w] = nb;
    }
    if (improves_a) best_xa[w] = na;
    if (improves_b) best_xb[w] = nb;
  }
  if (tid == 0) {
    a.e_cur[sa] = ea;
    a.e_cur[sb] = eb;
    if (improves_a) a.e_best[sa] = ea;
    if (improves_b) a.e_best[sb] = eb;
    report(a, n, s_size, Q, ea, eb);
  }
}

// The single call: pair blockIdx.x of the handle.
template <bool HBM>
__global__ __launch_bounds__(kThreads) void k_cluster_move(ClusterArgs a) {
  extern __shared__ uint64_t lds_planes[];
  const ClusterRow row = row_of(a, blockIdx.x);
  cluster_move_pair<HBM>(row, lds_planes);
}

// The two workgroup classes of a batch: row blockIdx.x of the class's part of the table.
template <bool HBM>
__global__ __launch_bounds__(kThreads) void k_cluster_move_rows(const ClusterRow *rows) {
  extern __shared__ uint64_t lds_planes[];
  const ClusterRow row = rows[blockIdx.x];
  cluster_move_pair<HBM>(row, lds_planes);
}

// ---- the packed form: a WAVEFRONT per pair, for handles of at most kPackedWords words (2048 spins) ----
// The three planes of a pair are 3 x 64 words of static LDS, lane l owns plane word l (lanes from 2 W on
// own nothing).  The four wavefronts of a workgroup run different pairs, with different numbers of search
// rounds, and some return early, so after a wavefront has taken its pair NOTHING here may wait for the
// workgroup: no __syncthreads, no workgroup barrier of any kind.  What one lane writes to the planes and
// another reads is ordered by the wavefront's own program order (wave_order below); every access of a
// plane word is an LDS atomic or an atomic load / store, so none is kept in a register across it.
constexpr uint32_t kPackedWords = 32;
constexpr uint32_t kPackedPairs = kThreads / 64u;

struct WavePlanes {
  uint32_t *base;
  __device__ __forceinline__ uint32_t load(uint32_t at) const {
    return __hip_atomic_load(base + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  __device__ __forceinline__ void store(uint32_t at, uint32_t v) const {
    __hip_atomic_store(base + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  __device__ __forceinline__ uint32_t fetch_or(uint32_t at, uint32_t v) const {
    return __hip_atomic_fetch_or(base + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  __device__ __forceinline__ uint32_t take(uint32_t at) const {
    return __hip_atomic_exchange(base + at, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
};

// LDS operations of a wavefront complete in the order they were issued: all that is needed between one
// lane's writes and another lane's reads is that the compiler keeps that order.
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void k_cluster_move_packed(const ClusterRow *rows, uint32_t count) {
  __shared__ uint32_t s_planes[kPackedPairs][3u * 64u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // (the wavefront's index as a scalar: the row is then read with scalar loads)
  const uint32_t at = __builtin_amdgcn_readfirstlane(blockIdx.x * kPackedPairs + wave);
  if (at >= count) return;  // (uniform over the wavefront) no pair for this wavefront of the last workgroup
  const ClusterRow a = rows[at];
  const uint32_t K = a.num_spins, W = a.words, W2 = 2u * W;  // W2 <= 64
  const uint32_t sa = a.slot_a, sb = a.slot_b;
  uint64_t *xa = a.x_cur + static_cast<uint64_t>(sa) * W;
  uint64_t *xb = a.x_cur + static_cast<uint64_t>(sb) * W;
  const WavePlanes planes{s_planes[wave]};
  const uint32_t D = 0u, M = 64u, F = 128u;  // word offsets of d, member, frontier

  // ---- step 1: d = x_a xor x_b, lane l the 32-bit word l; n by a prefix sum over the wavefront ----
  uint32_t d = 0;
  if (lane < W2) {
    const uint64_t both = xa[lane >> 1] ^ xb[lane >> 1];
    d = static_cast<uint32_t>(both >> (32u * (lane & 1u)));
    const uint32_t from = 32u * lane;  // (bits from num_spins on cleared)
    if (K < from + 32u) d &= K > from ? (1u << (K - from)) - 1u : 0u;
  }
  planes.store(D + lane, d);
  planes.store(M + lane, 0u);
  planes.store(F + lane, 0u);
  const uint32_t mine = static_cast<uint32_t>(__popc(d));
  uint32_t upto = mine;  // inclusive
  for (uint32_t step = 1; step < 64u; step <<= 1) {
    const uint32_t below = __shfl_up(upto, step);
    if (lane >= step) upto += below;
  }
  const uint32_t n = __shfl(upto, 63);
  if (n == 0u) {  // (uniform) identical replicas: nothing changes for the pair
    if (lane == 0) report(a, 0u, 0u, 0ll, a.e_cur[sa], a.e_cur[sb]);
    return;
  }

  // ---- step 2: the U-th differing site, U = floor(v n / 2^32) ----
  const Philox4 rnd = philox4x32_10(sa, a.sweeps_done, 0xFFFFFFFBu, a.draw, static_cast<uint32_t>(a.seed),
                                    static_cast<uint32_t>(a.seed >> 32));
  const uint32_t U = __umulhi(rnd.w[0], n);
  const uint32_t before = upto - mine;
  if (U >= before && U < before + mine) {  // exactly one lane
    uint32_t rest = d;
    for (uint32_t skip = U - before; skip != 0u; --skip) rest &= rest - 1u;
    const uint32_t bit = 1u << (__ffs(rest) - 1);
    planes.store(M + lane, bit);
    planes.store(F + lane, bit);
  }

  // ---- step 3: the component, level by level; at most |C| + 1 rounds ----
  auto visit = [&](uint32_t j) -> uint32_t {
    const uint32_t wj = j >> 5, bj = 1u << (j & 31u);
    if ((planes.load(D + wj) & bj) == 0u) return 0u;
    if ((planes.load(M + wj) & bj) != 0u) return 0u;
    if ((planes.fetch_or(M + wj, bj) & bj) != 0u) return 0u;  // (somebody else was first)
    planes.fetch_or(F + wj, bj);
    return 1u;
  };
  for (;;) {
    wave_order();
    uint32_t added = 0;
    uint32_t f = planes.take(F + lane);  // (every lane takes its word before any lane sets a bit)
    wave_order();
    uint32_t shared_rows = 0;
    while (f != 0u) {
      const uint32_t bit = static_cast<uint32_t>(__ffs(f) - 1);
      f &= f - 1u;
      const uint32_t i = lane * 32u + bit;
      const uint32_t begin = a.row_ptr[i], end = a.row_ptr[i + 1u];
      if (end - begin > kSharedRow) {
        shared_rows |= 1u << bit;
        continue;
      }
      uint32_t k = begin;
      for (; k + 4u <= end; k += 4u) {  // (four columns in flight together)
        const uint32_t j0 = a.col[k], j1 = a.col[k + 1u], j2 = a.col[k + 2u], j3 = a.col[k + 3u];
        added |= visit(j0) | visit(j1) | visit(j2) | visit(j3);
      }
      for (; k < end; ++k) added |= visit(a.col[k]);
    }
    // long rows, one at a time: the lanes stride the row
    uint64_t waiting = __ballot(shared_rows != 0u);
    while (waiting != 0ull) {
      const int leader = __ffsll(static_cast<unsigned long long>(waiting)) - 1;
      const uint32_t theirs = __shfl(shared_rows, leader);
      const uint32_t bit = static_cast<uint32_t>(__ffs(theirs) - 1);
      if (static_cast<int>(lane) == leader) shared_rows &= shared_rows - 1u;
      const uint32_t i = static_cast<uint32_t>(leader) * 32u + bit;
      const uint32_t begin = a.row_ptr[i], end = a.row_ptr[i + 1u];
      for (uint32_t k = begin + lane; k < end; k += 64u) added |= visit(a.col[k]);
      waiting = __ballot(shared_rows != 0u);
    }
    if (__ballot(added != 0u) == 0ull) break;
  }
  wave_order();

  // ---- step 4: Q and |C|, the lanes stride the sites; no atomics on a sum ----
  long long q_sum = 0;
  uint32_t members = 0;
  for (uint32_t i = lane; i < K; i += 64u) {
    if (((planes.load(M + (i >> 5)) >> (i & 31u)) & 1u) == 0u) continue;
    members += 1u;
    q_sum += member_energy(a, planes, D, xa, i);
  }
  for (int offset = 32; offset != 0; offset >>= 1) {
    q_sum += __shfl_xor(q_sum, offset);
    members += __shfl_xor(members, offset);
  }
  // (every lane has read what it needs of x_a before the reduction above ends, so before any lane flips;
  // and reads the tracked energies before lane 0 replaces them)
  const long long Q = q_sum;
  const long long ea = a.e_cur[sa] + Q, eb = a.e_cur[sb] - Q;
  const bool improves_a = ea < a.e_best[sa], improves_b = eb < a.e_best[sb];
  wave_order();

  // ---- steps 5 and 6: lane l the 64-bit word l ----
  if (lane < W) {
    const uint64_t m = static_cast<uint64_t>(planes.load(M + 2u * lane)) |
                       (static_cast<uint64_t>(planes.load(M + 2u * lane + 1u)) << 32);
    const uint64_t na = xa[lane] ^ m, nb = xb[lane] ^ m;
    if (m != 0ull) {
      xa[lane] = na;
      xb[lane] = nb;
    }
    if (improves_a) a.x_best[static_cast<uint64_t>(sa) * W + lane] = na;
    if (improves_b) a.x_best[static_cast<uint64_t>(sb) * W + lane] = nb;
  }
  if (lane == 0) {
    a.e_cur[sa] = ea;
    a.e_cur[sb] = eb;
    if (improves_a) a.e_best[sa] = ea;
    if (improves_b) a.e_best[sb] = eb;
    report(a, n, members, Q, ea, eb);
  }
}

thread_local float g_cluster_ms = 0.0f;
thread_local float g_cluster_batch_ms = 0.0f;

// pairs[0 .. 2 P) of a handle of R chains: every slot below R and named at most once.  `where`: what the
// message begins with ("" or "item 3: ").
int check_pairs(const uint32_t *pairs, uint32_t P, uint32_t R, const char *where) {
  std::vector<uint32_t> named(R, 0xFFFFFFFFu);  // the entry of `pairs` that names the slot
  for (uint64_t k = 0; k < 2ull * P; ++k) {
    const uint32_t slot = pairs[k];
    if (slot >= R) {
      return asp::set_error(ASP_ERR_INVALID, "%spairs[%llu] = %u is not one of the %u chains", where,
                            static_cast<unsigned long long>(k), slot, R);
    }
    if (named[slot] != 0xFFFFFFFFu) {
      return asp::set_error(ASP_ERR_INVALID, "%spairs[%u] and pairs[%llu] name the same chain %u", where,
                            named[slot], static_cast<unsigned long long>(k), slot);
    }
    named[slot] = static_cast<uint32_t>(k);
  }
  return ASP_OK;
}

}  // namespace

namespace asp {

// Rows of A over original indices and the field in original order, uploaded on a plan's first move
// (or first device tree, csrc/greedy_tree.hip).
int ensure_rows(asp_sa_plan *p) {
  if (p->cluster_row_ptr.ptr) return ASP_OK;
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  const uint64_t nnz = static_cast<uint64_t>(L.a_ptr[K]);
  if (nnz > 0xFFFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 1 couplings");
  std::vector<uint32_t> row_ptr(K + 1), col(nnz);
  std::vector<double> field(K);
  for (uint64_t i = 0; i <= K; ++i) row_ptr[i] = static_cast<uint32_t>(L.a_ptr[i]);
  for (uint64_t k = 0; k < nnz; ++k) col[k] = static_cast<uint32_t>(L.a_col[k]);
  for (uint64_t i = 0; i < K; ++i) field[i] = L.field_pos[L.pos_of_spin[i]];
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);  // (the staging vectors live until the copies are done)
  asp::DeviceBuffer<uint32_t> d_row_ptr;
  ASP_TRY(asp::upload_vector(d_row_ptr, row_ptr, s));
  ASP_TRY(asp::upload_vector(p->cluster_col, col, s));
  ASP_TRY(asp::upload_vector(p->cluster_val, L.a_val, s));
  ASP_TRY(asp::upload_vector(p->cluster_field, field, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  std::swap(p->cluster_row_ptr.ptr, d_row_ptr.ptr);  // (set last: what marks the rows as uploaded)
  std::swap(p->cluster_row_ptr.count, d_row_ptr.count);
  return ASP_OK;
}

}  // namespace asp

extern "C" {

int asp_sa_chains_set_cluster_planes(asp_sa_chains *c, int where) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  c->cluster_planes = where < 0 ? 0 : (where > 2 ? 2 : where);
  return ASP_OK;
}

float asp_sa_chains_cluster_move_last_ms(void) { return g_cluster_ms; }

int asp_sa_chains_cluster_move(asp_sa_chains *c, uint32_t const *pairs, uint32_t num_pairs, uint32_t draw,
                               uint32_t *out_differing, uint32_t *out_size, int64_t *out_delta) {
  asp_clear_error();
  g_cluster_ms = 0.0f;
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (num_pairs && !pairs) return asp::set_error(ASP_ERR_INVALID, "null pairs");
  const uint32_t R = c->repetitions, P = num_pairs;
  ASP_TRY(check_pairs(pairs, P, R, ""));
  asp_sa_plan *p = c->plan;
  if (P == 0 || R == 0) return ASP_OK;
  if (p->host.num_spins == 0) {  // no spins: no site differs
    for (uint32_t k = 0; k < P; ++k) {
      if (out_differing) out_differing[k] = 0u;
      if (out_size) out_size[k] = 0u;
      if (out_delta) out_delta[k] = 0;
    }
    return ASP_OK;
  }
  ASP_TRY(asp::bind_device());
  ASP_TRY(asp::ensure_rows(p));
  const uint32_t W = c->words;
  const size_t plane_bytes = 3ull * 8ull * W;
  const bool fits = plane_bytes + kStaticLds <= p->max_lds;
  if (c->cluster_planes == 1 && !fits) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%zu B of LDS needed for the planes, %zu B available",
                          plane_bytes + kStaticLds, p->max_lds);
  }
  const bool hbm = c->cluster_planes == 2 || !fits;
  // what comes back in one copy: n | size << 32 [P], Q [P], tracked_current of the pairs' slots [2 P]
  const uint64_t back_words = 4ull * P;
  std::vector<uint64_t> h_back(back_words, 0);
  asp::DeviceBuffer<uint64_t> d_back;
  asp::DeviceBuffer<uint32_t> d_pairs;
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);
  ASP_TRY(d_back.alloc(back_words));
  ASP_TRY(d_pairs.alloc(2ull * P));
  if (hbm) ASP_TRY(p->cluster_scratch.ensure(static_cast<uint64_t>(P) * 6ull * W));
  ASP_TRY(d_pairs.upload(pairs, 2ull * P, s));
  const ClusterArgs args{p->cluster_row_ptr.ptr, p->cluster_col.ptr, p->cluster_val.ptr, p->cluster_field.ptr,
                         c->x_cur.ptr,           c->x_best.ptr,      c->e_cur.ptr,       c->e_best.ptr,
                         d_pairs.ptr,            hbm ? p->cluster_scratch.ptr : nullptr,  d_back.ptr,
                         c->seed,                std::ldexp(1.0, p->host.energy_scale_exp),
                         static_cast<uint32_t>(p->host.num_spins), W, P, c->sweeps_done, draw};
  ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
  if (hbm) {
    hipLaunchKernelGGL(k_cluster_move<true>, dim3(P), dim3(kThreads), 0, s, args);
  } else {
    if (plane_bytes > 48u * 1024u) {
      ASP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cluster_move<false>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(plane_bytes)));
    }
    hipLaunchKernelGGL(k_cluster_move<false>, dim3(P), dim3(kThreads), plane_bytes, s, args);
  }
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(p->ev[3], s));
  ASP_TRY(d_back.download(h_back.data(), back_words, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  ASP_HIP_TRY(hipEventElapsedTime(&g_cluster_ms, p->ev[0], p->ev[3]));
  for (uint32_t k = 0; k < P; ++k) {
    if (out_differing) out_differing[k] = static_cast<uint32_t>(h_back[k]);
    if (out_size) out_size[k] = static_cast<uint32_t>(h_back[k] >> 32);
    if (out_delta) out_delta[k] = static_cast<int64_t>(h_back[P + k]);
    c->h_e_cur[pairs[2u * k]] = static_cast<int64_t>(h_back[2ull * P + 2u * k]);
    c->h_e_cur[pairs[2u * k + 1u]] = static_cast<int64_t>(h_back[2ull * P + 2u * k + 1u]);
  }
  return ASP_OK;
}

float asp_sa_chains_cluster_move_batch_last_ms(void) { return g_cluster_batch_ms; }

int asp_sa_chains_cluster_move_batch(asp_sa_chains_cluster_item const *items, uint32_t count) {
  asp_clear_error();
  g_cluster_batch_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before any device work and before any output is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_cluster_item &it = items[i];
    if (it.flags & ~ASP_CLUSTER_NO_PACKED) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    }
    if (!it.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    if (it.num_pairs && !it.pairs) return asp::set_error(ASP_ERR_INVALID, "item %u: null pairs", i);
    char where[32];
    std::snprintf(where, sizeof(where), "item %u: ", i);
    ASP_TRY(check_pairs(it.pairs, it.num_pairs, it.chains->repetitions, where));
  }
  {
    std::vector<asp_sa_chains *> handles(count);
    for (uint32_t i = 0; i < count; ++i) handles[i] = items[i].chains;
    ASP_TRY(asp::check_distinct_plans(handles));
  }
  // ---- the items that run, their places in the back buffer (item after item, pair after pair) and
  // their launch classes: 0 packed (a wavefront per pair), 1 a workgroup with the planes in LDS, 2 in HBM ----
  struct Live {
    uint32_t item, klass;
    uint64_t at;  // the first pair's place in the back buffer
  };
  std::vector<Live> live;
  uint64_t total = 0;
  uint64_t in_class[3] = {0, 0, 0};
  size_t lds_bytes = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_cluster_item &it = items[i];
    const asp_sa_chains *c = it.chains;
    if (it.num_pairs == 0 || c->repetitions == 0 || c->plan->host.num_spins == 0) continue;
    const size_t plane_bytes = 3ull * 8ull * c->words;
    const bool fits = plane_bytes + kStaticLds <= c->plan->max_lds;
    uint32_t klass;
    if (c->words <= kPackedWords && !(it.flags & ASP_CLUSTER_NO_PACKED)) {
      klass = 0;
    } else if (c->cluster_planes == 1 && !fits) {
      return asp::set_error(ASP_ERR_TOO_LARGE, "item %u: %zu B of LDS needed for the planes, %zu B available", i,
                            plane_bytes + kStaticLds, c->plan->max_lds);
    } else if (c->cluster_planes == 2 || !fits) {
      klass = 2;
    } else {
      klass = 1;
      lds_bytes = std::max(lds_bytes, plane_bytes);
    }
    live.push_back(Live{i, klass, total});
    in_class[klass] += it.num_pairs;
    total += it.num_pairs;
  }
  if (total > 0x7FFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^31 - 1 pairs in one batch");
  // what comes back in one copy: n | size << 32 [total], Q [total], tracked_current of the pairs' slots [2 total]
  const uint64_t back_words = 4ull * total;
  std::vector<uint64_t> h_back(back_words, 0);
  if (total != 0) {
    ASP_TRY(asp::bind_device());
    for (const Live &l : live) ASP_TRY(asp::ensure_rows(items[l.item].chains->plan));
    asp::DeviceBuffer<ClusterRow> d_rows;
    asp::DeviceBuffer<uint64_t> d_back;
    asp::EventPool events;
    hipEvent_t begin = nullptr, end = nullptr;
    asp::ScopedStream batch;
    ASP_TRY(batch.acquire());
    hipStream_t s = batch.stream;
    ASP_TRY(events.make(&begin, true));
    ASP_TRY(events.make(&end, true));
    ASP_TRY(d_rows.alloc(total));
    ASP_TRY(d_back.alloc(back_words));
    // the table: the rows of class 0, then of class 1, then of class 2
    const uint64_t first_of[3] = {0, in_class[0], in_class[0] + in_class[1]};
    uint64_t next[3] = {first_of[0], first_of[1], first_of[2]};
    std::vector<ClusterRow> rows(total);
    for (const Live &l : live) {
      const asp_sa_chains_cluster_item &it = items[l.item];
      asp_sa_chains *c = it.chains;
      asp_sa_plan *p = c->plan;
      const uint32_t W = c->words;
      if (l.klass == 2) ASP_TRY(p->cluster_scratch.ensure(static_cast<uint64_t>(it.num_pairs) * 6ull * W));
      for (uint32_t k = 0; k < it.num_pairs; ++k) {
        rows[next[l.klass]++] = ClusterRow{
            p->cluster_row_ptr.ptr, p->cluster_col.ptr, p->cluster_val.ptr, p->cluster_field.ptr,
            c->x_cur.ptr, c->x_best.ptr, c->e_cur.ptr, c->e_best.ptr,
            l.klass == 2 ? p->cluster_scratch.ptr + static_cast<uint64_t>(k) * 6ull * W : nullptr,
            d_back.ptr, c->seed, std::ldexp(1.0, p->host.energy_scale_exp),
            static_cast<uint32_t>(p->host.num_spins), W, it.pairs[2u * k], it.pairs[2u * k + 1u],
            c->sweeps_done, it.draw, static_cast<uint32_t>(l.at + k), static_cast<uint32_t>(total)};
      }
    }
    asp::StreamFence fence(s);  // (declared after the buffers: waited for before they go)
    // the batch stream runs after what is pending on the plans' streams
    // (a stream with nothing pending — the usual case: every entry point waits for its stream — needs no event)
    for (const Live &l : live) {
      asp_sa_plan *p = items[l.item].chains->plan;
      const hipError_t pending = hipStreamQuery(p->stream);
      if (pending == hipSuccess) continue;
      if (pending != hipErrorNotReady) ASP_HIP_TRY(pending);
      ASP_HIP_TRY(hipEventRecord(p->ev[0], p->stream));
      ASP_HIP_TRY(hipStreamWaitEvent(s, p->ev[0], 0));
    }
    ASP_TRY(d_rows.upload(rows.data(), total, s));
    ASP_HIP_TRY(hipEventRecord(begin, s));
    if (in_class[0] != 0) {
      const uint32_t n = static_cast<uint32_t>(in_class[0]);
      hipLaunchKernelGGL(k_cluster_move_packed, dim3((n + kPackedPairs - 1u) / kPackedPairs), dim3(kThreads), 0, s,
                         d_rows.ptr + first_of[0], n);
      ASP_HIP_TRY(hipGetLastError());
    }
    if (in_class[1] != 0) {
      if (lds_bytes > 48u * 1024u) {
        ASP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cluster_move_rows<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
      }
      hipLaunchKernelGGL(k_cluster_move_rows<false>, dim3(static_cast<uint32_t>(in_class[1])), dim3(kThreads),
                         lds_bytes, s, d_rows.ptr + first_of[1]);
      ASP_HIP_TRY(hipGetLastError());
    }
    if (in_class[2] != 0) {
      hipLaunchKernelGGL(k_cluster_move_rows<true>, dim3(static_cast<uint32_t>(in_class[2])), dim3(kThreads), 0, s,
                         d_rows.ptr + first_of[2]);
      ASP_HIP_TRY(hipGetLastError());
    }
    ASP_HIP_TRY(hipEventRecord(end, s));
    ASP_TRY(d_back.download(h_back.data(), back_words, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
    ASP_HIP_TRY(hipEventElapsedTime(&g_cluster_batch_ms, begin, end));
  }
  // ---- the handles' host mirrors and the outputs ----
  for (const Live &l : live) {
    const asp_sa_chains_cluster_item &it = items[l.item];
    asp_sa_chains *c = it.chains;
    for (uint32_t k = 0; k < it.num_pairs; ++k) {
      const uint64_t r = l.at + k;
      if (it.out_differing) it.out_differing[k] = static_cast<uint32_t>(h_back[r]);
      if (it.out_size) it.out_size[k] = static_cast<uint32_t>(h_back[r] >> 32);
      if (it.out_delta) it.out_delta[k] = static_cast<int64_t>(h_back[total + r]);
      c->h_e_cur[it.pairs[2u * k]] = static_cast<int64_t>(h_back[2ull * total + 2u * r]);
      c->h_e_cur[it.pairs[2u * k + 1u]] = static_cast<int64_t>(h_back[2ull * total + 2u * r + 1u]);
    }
  }
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_cluster_item &it = items[i];
    if (it.chains->repetitions != 0 && it.chains->plan->host.num_spins != 0) continue;
    // no chains or no spins: nothing runs; no site differs
    for (uint32_t k = 0; k < it.num_pairs; ++k) {
      if (it.out_differing) it.out_differing[k] = 0u;
      if (it.out_size) it.out_size[k] = 0u;
      if (it.out_delta) it.out_delta[k] = 0;
    }
  }
  return ASP_OK;
}

}  // extern "C"
