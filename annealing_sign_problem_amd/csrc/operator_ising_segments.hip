// The coupling build of many clusters in one call (specification ASP-ISING-SEG-1), on
// gfx950: asp_operator_ising_csr over every segment of a concatenated table, in shared launches.
// For segment g the result is, bit for bit, what asp_operator_ising_csr returns for its keys and
// amplitudes alone: J = 0.5 * (M + M^T), M_ij = (H_ij |psi_j|) |psi_i| over the states of the segment,
// duplicates summed in connection order from 0, an entry pruned iff the sum is 0.
//
// HBM layout: offsets u64[S+1]; keys u64[T], psi f64[T] (segments concatenated, each ascending);
//   row_segment u32[T] (k_row_segments); ONE open-addressing hash over all T entries
//   {fingerprint:32 | global index+1:32}, u64[2^s >= 2T], hashed with a per-segment salt (the rule of
//   operator_local_energy.hip), so that a state present in every segment does not form one probe chain;
//   row_nnz u32[T] -> indptr i64[T+1] by ONE device scan over all rows; out col i32[nnz] (position
//   within the segment), val f64[nnz].
// Mapping: one wavefront per table row, four rows per workgroup; what a row shares (salt, begin, end of
//   its segment) is wavefront-uniform and sits in SGPRs.
//   k_ising_rows_seg<EMIT>   operators with unique targets: lanes over the bonds in chunks of 64, at most
//                            three transitions per lane, both matrix elements of a pair from the bond's 4x4
//                            matrix (k_ising_rows), the lookup restricted to the row's own segment; the
//                            row's entries rank-sorted in per-wavefront LDS.
//   k_merge_rows_seg         rows that may reach a state twice (symmetry-adapted bases, single-site
//                            flips): the row's entries of the device connection list, columns through
//                            the hash, duplicates summed in connection order -> Mhat, row r's distinct
//                            columns sorted IN the row's own range of the connection list (no scan).
//   k_sym_rows_seg<EMIT>     Mhat_jr by bisection in global row begin + j, prune; counts the entries
//                            without a mirror and records the first segment that has one.
// No atomics on floating-point data, no dependency between workgroups; the CAS insertion runs at load
// factor <= 1/2.  Host synchronisations per call: two (unique targets) or three, whatever S is.
// Traffic: 20 B/row in, 8 B/row + 12 B/non-zero out; the probes hit the L2-resident table.
#include <algorithm>
#include <vector>

#include "asp_common.hpp"
#include "operator_internal.hpp"

namespace {

using asp::Bond;
using asp::DeviceBuffer;
using asp::mix64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// (segment_of, segment_salt and the probe are those of operator_local_energy.hip)
__device__ __forceinline__ uint64_t segment_of(const uint64_t *__restrict__ offsets, uint64_t num_segments,
                                               uint64_t i) {
  uint64_t lo = 0, hi = num_segments;  // offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (offsets[mid] <= i) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

__device__ __forceinline__ uint64_t segment_salt(uint64_t segment) { return mix64(segment + 1ull); }

// row -> segment for every table entry, and the entry into the salted hash.
__global__ __launch_bounds__(kThreads) void k_row_segments(const uint64_t *__restrict__ keys, uint64_t total,
                                                          const uint64_t *__restrict__ offsets,
                                                          uint64_t num_segments,
                                                          uint32_t *__restrict__ row_segment,
                                                          unsigned long long *__restrict__ slots,
                                                          uint64_t mask) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= total) return;
  const uint64_t g = segment_of(offsets, num_segments, i);
  row_segment[i] = static_cast<uint32_t>(g);
  const uint64_t h = mix64(keys[i] ^ segment_salt(g));
  const unsigned long long entry = (h & 0xFFFFFFFF00000000ull) | (i + 1);
  uint64_t at = h & mask;
  while (atomicCAS(&slots[at], 0ull, entry) != 0ull) at = (at + 1) & mask;
}

struct Table {
  const uint64_t *keys;
  const double *psi;
  const uint64_t *offsets;  // u64[S + 1]
  const uint32_t *row_segment;
  const unsigned long long *slots;
  uint64_t mask;
  uint64_t total;  // T
};

struct Segment {
  uint64_t salt, begin, end;
};

__device__ __forceinline__ Segment segment_of_row(const Table &t, uint64_t r) {
  const uint32_t g = t.row_segment[r];
  return Segment{segment_salt(g), t.offsets[g], t.offsets[g + 1]};
}

// Global index of `needle` among the keys of the segment, or -1.
__device__ __forceinline__ int64_t find_in_segment(const Table &t, const Segment &s, uint64_t needle) {
  const uint64_t h = mix64(needle ^ s.salt);
  const uint32_t fingerprint = static_cast<uint32_t>(h >> 32);
  for (uint64_t at = h & t.mask;; at = (at + 1) & t.mask) {
    const unsigned long long slot = t.slots[at];
    if (slot == 0) return -1;
    if (static_cast<uint32_t>(slot >> 32) != fingerprint) continue;
    const uint64_t idx = static_cast<uint32_t>(slot) - 1u;
    if (idx >= s.begin && idx < s.end && t.keys[idx] == needle) return static_cast<int64_t>(idx);
  }
}

__device__ __forceinline__ uint32_t wave_exclusive_scan_u32(uint32_t v, uint32_t lane, uint32_t *total) {
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= static_cast<uint32_t>(d)) incl += up;
  }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}

// ---------------------------------------------------------------------------
// operators with unique targets: the pair-fused pass
// ---------------------------------------------------------------------------

struct RowsArgs {
  Table t;
  const Bond *bonds;
  uint32_t num_bonds;
  uint32_t row_capacity;     // LDS entries per wavefront (EMIT only)
  const int64_t *row_start;  // EMIT only: the global indptr
  uint32_t *row_nnz;         // count pass
  int32_t *col;
  double *val;
};

// M_rj + M_jr from the lane's bond for transition src -> dst (pair_coupling of operator_apply.hip, the
// lookup within the segment); *at: global index of j, -1 when j is outside the segment.
__device__ __forceinline__ double pair_coupling(const Table &t, const Segment &s, const Bond &bond,
                                                uint64_t key, double psi_r, uint32_t src, uint32_t dst,
                                                int64_t *at) {
  const double fwd = bond.m[dst * 4u + src];  // H_jr: row r's connection to j
  const double rev = bond.m[src * 4u + dst];  // H_rj: row j's connection back to r
  *at = -1;
  if (fwd == 0.0 && rev == 0.0) return 0.0;
  const int64_t j = find_in_segment(t, s, key ^ bond.flip[src ^ dst]);
  if (j < 0) return 0.0;
  *at = j;
  const double psi_j = fabs(t.psi[j]);
  double sum = 0.0;
  if (fwd != 0.0) sum = __dadd_rn(sum, __dmul_rn(__dmul_rn(fwd, psi_j), psi_r));
  if (rev != 0.0) sum = __dadd_rn(sum, __dmul_rn(__dmul_rn(rev, psi_r), psi_j));
  return sum;
}

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_ising_rows_seg(RowsArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const uint32_t lane = threadIdx.x & 63u;
  // (the wave index through readfirstlane: provably wavefront-uniform, so what the row shares sits in SGPRs)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.t.total) return;  // whole wavefront; no workgroup barrier below
  // per-wavefront staging area: vals f64[capacity] | cols i32[capacity]
  double *vals = reinterpret_cast<double *>(lds) + static_cast<size_t>(wave) * a.row_capacity;
  int32_t *cols = reinterpret_cast<int32_t *>(reinterpret_cast<double *>(lds) +
                                              static_cast<size_t>(kWaves) * a.row_capacity) +
                  static_cast<size_t>(wave) * a.row_capacity;
  const Segment s = segment_of_row(a.t, r);
  const uint64_t key = a.t.keys[r];
  const double psi_r = fabs(a.t.psi[r]);
  uint32_t kept = 0;
  double diagonal = 0.0;
  for (uint32_t first = 0; first < a.num_bonds; first += 64u) {
    const uint32_t bi = first + lane;
    double dval = 0.0;
    double v[3] = {0.0, 0.0, 0.0};
    int64_t c[3] = {-1, -1, -1};
    uint32_t mine = 0;
    if (bi < a.num_bonds) {
      const Bond &bond = a.bonds[bi];
      const uint32_t src = static_cast<uint32_t>(((key >> bond.a) & 1ull) * 2ull + ((key >> bond.b) & 1ull));
      dval = bond.m[src * 4u + src];
      uint32_t slot = 0;
#pragma unroll
      for (uint32_t dst = 0; dst < 4; ++dst) {
        if (dst == src) continue;
        int64_t at;
        // scipy keeps an entry of M + M^T iff the sum is non-zero, then scales it by 0.5
        const double x = pair_coupling(a.t, s, bond, key, psi_r, src, dst, &at);
        if (x != 0.0) {
          const double half = __dmul_rn(0.5, x);
          const int64_t local = at - static_cast<int64_t>(s.begin);
          // (constant indices: the three slots stay in registers)
          if (slot == 0) { v[0] = half; c[0] = local; }
          if (slot == 1) { v[1] = half; c[1] = local; }
          if (slot == 2) { v[2] = half; c[2] = local; }
          ++slot;
        }
      }
      mine = slot;
    }
    const uint32_t here = min(64u, a.num_bonds - first);
    for (uint32_t j = 0; j < here; ++j) diagonal = __dadd_rn(diagonal, __shfl(dval, j, 64));
    uint32_t total;
    const uint32_t before = wave_exclusive_scan_u32(mine, lane, &total);
    if (EMIT) {
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) {
        if (k < mine) {
          cols[kept + before + k] = static_cast<int32_t>(c[k]);
          vals[kept + before + k] = v[k];
        }
      }
    }
    kept += total;
  }
  // J_rr = 0.5 * (M_rr + M_rr), M_rr = (diag * |psi_r|) * |psi_r|
  const double m_rr = __dmul_rn(__dmul_rn(diagonal, psi_r), psi_r);
  const double twice = __dadd_rn(m_rr, m_rr);
  const bool has_diag = twice != 0.0;
  if (EMIT && has_diag && lane == 0) {
    cols[kept] = static_cast<int32_t>(r - s.begin);
    vals[kept] = __dmul_rn(0.5, twice);
  }
  kept += has_diag ? 1u : 0u;
  if (!EMIT) {
    if (lane == 0) a.row_nnz[r] = kept;
    return;
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  // columns of a row are distinct: rank = number of smaller columns
  const int64_t out = a.row_start[r];
  for (uint32_t e = lane; e < kept; e += 64u) {
    const int32_t mine_col = cols[e];
    uint32_t rank = 0;
    for (uint32_t o = 0; o < kept; ++o) rank += cols[o] < mine_col ? 1u : 0u;
    a.col[out + rank] = mine_col;
    a.val[out + rank] = vals[e];
  }
}

// ---------------------------------------------------------------------------
// rows that may reach a state more than once: the reference's arithmetic with its duplicates
// (k_merge_rows / k_sym_rows of operator_apply.hip, per segment)
// ---------------------------------------------------------------------------

struct MergeArgs {
  Table t;
  const int64_t *list_offsets;  // connections of row r: [list_offsets[r], list_offsets[r + 1])
  const uint64_t *other_keys;   // targets (representatives for a symmetric basis)
  const double *other_coeffs;
  uint32_t row_capacity;  // LDS entries per wavefront
  // Mhat: row r's distinct columns (segment-local, ascending) at [list_offsets[r], + mrow_nnz[r])
  uint32_t *mrow_nnz;
  int32_t *mcol;
  double *mval;
};

__global__ __launch_bounds__(kThreads) void k_merge_rows_seg(MergeArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.t.total) return;  // whole wavefront; only wave-level barriers below
  // per wavefront: vals f64[cap] | cols i32[cap] | leader u8[cap]
  double *vals = reinterpret_cast<double *>(lds) + static_cast<size_t>(wave) * a.row_capacity;
  int32_t *cols = reinterpret_cast<int32_t *>(reinterpret_cast<double *>(lds) +
                                              static_cast<size_t>(kWaves) * a.row_capacity) +
                  static_cast<size_t>(wave) * a.row_capacity;
  uint8_t *leader = reinterpret_cast<uint8_t *>(reinterpret_cast<int32_t *>(
                        reinterpret_cast<double *>(lds) + static_cast<size_t>(kWaves) * a.row_capacity) +
                    static_cast<size_t>(kWaves) * a.row_capacity) +
                    static_cast<size_t>(wave) * a.row_capacity;
  const Segment s = segment_of_row(a.t, r);
  const int64_t begin = a.list_offsets[r];
  uint32_t n = static_cast<uint32_t>(a.list_offsets[r + 1] - begin);
  n = n < a.row_capacity ? n : a.row_capacity;  // (a row holds at most max_connections entries)
  const double psi_r = fabs(a.t.psi[r]);
  for (uint32_t i = lane; i < n; i += 64u) {
    const int64_t j = find_in_segment(a.t, s, a.other_keys[begin + i]);
    cols[i] = j < 0 ? -1 : static_cast<int32_t>(j - static_cast<int64_t>(s.begin));
    // (coeff * |psi_j|) * |psi_r|, each product rounded
    vals[i] = j < 0 ? 0.0 : __dmul_rn(__dmul_rn(a.other_coeffs[begin + i], fabs(a.t.psi[j])), psi_r);
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  uint32_t mine = 0;
  for (uint32_t i = lane; i < n; i += 64u) {
    bool first = cols[i] >= 0;
    for (uint32_t k = 0; k < i && first; ++k) first = cols[k] != cols[i];
    leader[i] = first ? 1 : 0;
    mine += first ? 1u : 0u;
  }
  uint32_t distinct = mine;
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) distinct += __shfl_xor(distinct, step, 64);
  if (lane == 0) a.mrow_nnz[r] = distinct;
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  for (uint32_t i = lane; i < n; i += 64u) {
    if (!leader[i]) continue;
    const int32_t c = cols[i];
    double sum = 0.0;  // scipy: A_row[col] starts at 0 and takes the duplicates in storage order
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n; ++k) {
      if (k >= i && cols[k] == c) sum = __dadd_rn(sum, vals[k]);
      rank += (leader[k] && cols[k] < c) ? 1u : 0u;
    }
    a.mcol[begin + rank] = c;  // rank < distinct <= n: inside the row's range of the list
    a.mval[begin + rank] = sum;
  }
}

struct SymArgs {
  Table t;
  const int64_t *list_offsets;
  const uint32_t *mrow_nnz;
  const int32_t *mcol;
  const double *mval;
  const int64_t *row_start;  // EMIT: the global indptr
  uint32_t *row_nnz;         // count pass
  unsigned long long *missing;  // [0]: entries without a mirror; [1]: the first segment that has one
  int32_t *col;
  double *val;
};

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_sym_rows_seg(SymArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.t.total) return;
  const uint32_t g = a.t.row_segment[r];
  const uint64_t seg_begin = a.t.offsets[g];
  const int32_t local = static_cast<int32_t>(r - seg_begin);
  const int64_t begin = a.list_offsets[r], end = begin + a.mrow_nnz[r];
  int64_t written = EMIT ? a.row_start[r] : 0;
  uint32_t kept = 0;
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t e = base + lane;
    bool keep = false;
    int32_t j = -1;
    double x = 0.0;
    if (e < end) {
      j = a.mcol[e];
      const double forward = a.mval[e];
      // Mhat_jr: bisection among the sorted columns of global row begin + j
      const uint64_t other = seg_begin + static_cast<uint64_t>(j);
      int64_t lo = a.list_offsets[other];
      const int64_t stop = lo + a.mrow_nnz[other];
      int64_t hi = stop;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.mcol[mid] < local) {
          lo = mid + 1;
        } else {
          hi = mid;
        }
      }
      const bool mirrored = lo < stop && a.mcol[lo] == local;
      if (!mirrored && !EMIT) {
        atomicAdd(&a.missing[0], 1ull);
        atomicMin(&a.missing[1], static_cast<unsigned long long>(g));
      }
      x = __dadd_rn(forward, mirrored ? a.mval[lo] : 0.0);  // (M + M.T)_rj
      keep = x != 0.0;
    }
    const uint64_t ballot = __ballot(keep);
    if (EMIT && keep) {
      const int64_t at = written + __popcll(ballot & ((1ull << lane) - 1ull));
      a.col[at] = j;
      a.val[at] = __dmul_rn(0.5, x);
    }
    written += __popcll(ballot);
    kept += static_cast<uint32_t>(__popcll(ballot));
  }
  if (!EMIT && lane == 0) a.row_nnz[r] = kept;
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  return static_cast<unsigned>((items + per_block - 1) / per_block);
}

struct Events {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int create() {
    ASP_HIP_TRY(hipEventCreate(&ev0));
    ASP_HIP_TRY(hipEventCreate(&ev1));
    return ASP_OK;
  }
  void finish() const {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) asp::set_operator_last_ms(ms);
  }
  ~Events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

// What both variants hand back.
struct Outputs {
  uint64_t capacity;
  int64_t *indptr;
  int32_t *col;
  double *val;
  uint64_t *nnz;
  bool sizing() const { return capacity == 0 && !indptr && !col && !val; }
  // after *nnz is known: ASP_OK when the result fits
  int fits() const {
    if (*nnz > capacity || !indptr || !col || !val) {
      return asp::set_error(ASP_ERR_INVALID, "%llu couplings do not fit capacity %llu",
                            (unsigned long long)*nnz, (unsigned long long)capacity);
    }
    return ASP_OK;
  }
};

// LDS bytes per workgroup of the row kernels (the conditions of operator_ising).
size_t lds_bytes(const asp_operator *op, uint32_t *row_capacity) {
  if (op->unique_targets) {
    uint32_t cap = (op->max_connections + 1u) & ~1u;  // even: keeps the i32 area 8-byte aligned
    // the pair (rev != 0, fwd == 0) can add entries beyond max_connections: 3 per bond is the cap
    const uint32_t cap_all = 3u * op->num_bonds + 2u;
    if (cap < cap_all) cap = (cap_all + 1u) & ~1u;
    *row_capacity = cap;
    return static_cast<size_t>(kWaves) * cap * (sizeof(double) + sizeof(int32_t));
  }
  *row_capacity = (op->max_connections + 7u) & ~7u;
  return static_cast<size_t>(kWaves) * *row_capacity * (sizeof(double) + sizeof(int32_t) + 1);
}

int segments_unique(const asp_operator *op, uint64_t S, const uint64_t *offsets, const uint64_t *keys,
                    const double *psi, uint32_t row_capacity, size_t lds, const Outputs &o,
                    hipStream_t stream) {
  const uint64_t T = offsets[S];
  uint64_t slots_n = 1024;
  while (slots_n < 2 * T) slots_n <<= 1;
  DeviceBuffer<uint64_t> d_keys, d_offsets;
  DeviceBuffer<double> d_psi, d_val;
  DeviceBuffer<unsigned long long> d_slots;
  DeviceBuffer<uint32_t> d_row_segment, d_row_nnz;
  DeviceBuffer<int64_t> d_row_start, d_scratch;
  DeviceBuffer<int32_t> d_col;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_keys.alloc(T));
  ASP_TRY(d_psi.alloc(T));
  ASP_TRY(d_offsets.alloc(S + 1));
  ASP_TRY(d_slots.alloc(slots_n));
  ASP_TRY(d_row_segment.alloc(T));
  ASP_TRY(d_row_nnz.alloc(T));
  ASP_TRY(d_row_start.alloc(T + 1));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(T)));
  ASP_TRY(events.create());
  ASP_TRY(d_keys.upload(keys, T, stream));
  ASP_TRY(d_psi.upload(psi, T, stream));
  ASP_TRY(d_offsets.upload(offsets, S + 1, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  ASP_HIP_TRY(hipMemsetAsync(d_slots.ptr, 0, slots_n * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_row_segments, dim3(grid_for(T, kThreads)), dim3(kThreads), 0, stream, d_keys.ptr, T,
                     d_offsets.ptr, S, d_row_segment.ptr, d_slots.ptr, slots_n - 1);
  ASP_HIP_TRY(hipGetLastError());
  RowsArgs a{};
  a.t = Table{d_keys.ptr, d_psi.ptr, d_offsets.ptr, d_row_segment.ptr, d_slots.ptr, slots_n - 1, T};
  a.bonds = op->d_bonds.ptr;
  a.num_bonds = op->num_bonds;
  a.row_capacity = 0;
  a.row_nnz = d_row_nnz.ptr;
  hipLaunchKernelGGL(k_ising_rows_seg<false>, dim3(grid_for(T, kWaves)), dim3(kThreads), 0, stream, a);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(asp::exclusive_scan_u32(d_row_nnz.ptr, T, d_row_start.ptr, d_scratch.ptr, stream));
  int64_t total = 0;
  ASP_HIP_TRY(hipMemcpyAsync(&total, d_row_start.ptr + T, sizeof total, hipMemcpyDeviceToHost, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  *o.nnz = static_cast<uint64_t>(total);
  if (o.sizing()) {
    ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
    ASP_HIP_TRY(hipStreamSynchronize(stream));
    events.finish();
    return ASP_OK;
  }
  ASP_TRY(o.fits());
  ASP_TRY(d_col.alloc(*o.nnz));
  ASP_TRY(d_val.alloc(*o.nnz));
  a.row_start = d_row_start.ptr;
  a.col = d_col.ptr;
  a.val = d_val.ptr;
  a.row_capacity = row_capacity;
  ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_ising_rows_seg<true>), lds));
  hipLaunchKernelGGL(k_ising_rows_seg<true>, dim3(grid_for(T, kWaves)), dim3(kThreads), lds, stream, a);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  ASP_TRY(d_row_start.download(o.indptr, T + 1, stream));
  ASP_TRY(d_col.download(o.col, *o.nnz, stream));
  ASP_TRY(d_val.download(o.val, *o.nnz, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  events.finish();
  return ASP_OK;
}

int segments_with_duplicates(const asp_operator *op, uint64_t S, const uint64_t *offsets,
                             const uint64_t *keys, const double *psi, uint32_t row_capacity, size_t lds,
                             const Outputs &o, hipStream_t stream) {
  const uint64_t T = offsets[S];
  uint64_t slots_n = 1024;
  while (slots_n < 2 * T) slots_n <<= 1;
  asp::ConnectionList list;
  asp::Symmetrised sym;
  DeviceBuffer<uint64_t> d_offsets;
  DeviceBuffer<double> d_psi, d_mval, d_val;
  DeviceBuffer<unsigned long long> d_slots, d_missing;
  DeviceBuffer<uint32_t> d_row_segment, d_mrow_nnz, d_row_nnz;
  DeviceBuffer<int64_t> d_row_start, d_scratch;
  DeviceBuffer<int32_t> d_mcol, d_col;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_psi.alloc(T));
  ASP_TRY(d_offsets.alloc(S + 1));
  ASP_TRY(d_slots.alloc(slots_n));
  ASP_TRY(d_missing.alloc(2));
  ASP_TRY(d_row_segment.alloc(T));
  ASP_TRY(d_mrow_nnz.alloc(T));
  ASP_TRY(d_row_nnz.alloc(T));
  ASP_TRY(d_row_start.alloc(T + 1));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(T)));
  ASP_TRY(events.create());
  ASP_TRY(d_psi.upload(psi, T, stream));
  ASP_TRY(d_offsets.upload(offsets, S + 1, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  // the connections of every key of the table (per key: the order of the keys does not matter); the
  // keys are uploaded there, once.  First synchronisation: the size of the list.
  ASP_TRY(asp::connection_list_queue(op, T, keys, &list, &sym, stream));
  const uint64_t *d_keys = list.batch.d_keys.ptr;
  ASP_TRY(d_mcol.alloc(list.batch.total));
  ASP_TRY(d_mval.alloc(list.batch.total));
  ASP_HIP_TRY(hipMemsetAsync(d_slots.ptr, 0, slots_n * sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_missing.ptr, 0, sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_missing.ptr + 1, 0xFF, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_row_segments, dim3(grid_for(T, kThreads)), dim3(kThreads), 0, stream, d_keys, T,
                     d_offsets.ptr, S, d_row_segment.ptr, d_slots.ptr, slots_n - 1);
  ASP_HIP_TRY(hipGetLastError());
  const Table table{d_keys, d_psi.ptr, d_offsets.ptr, d_row_segment.ptr, d_slots.ptr, slots_n - 1, T};
  MergeArgs m{};
  m.t = table;
  m.list_offsets = list.batch.d_offsets.ptr;
  m.other_keys = list.d_other.ptr;
  m.other_coeffs = list.d_coeffs.ptr;
  m.row_capacity = row_capacity;
  m.mrow_nnz = d_mrow_nnz.ptr;
  m.mcol = d_mcol.ptr;
  m.mval = d_mval.ptr;
  ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_merge_rows_seg), lds));
  hipLaunchKernelGGL(k_merge_rows_seg, dim3(grid_for(T, kWaves)), dim3(kThreads), lds, stream, m);
  ASP_HIP_TRY(hipGetLastError());
  SymArgs y{};
  y.t = table;
  y.list_offsets = list.batch.d_offsets.ptr;
  y.mrow_nnz = d_mrow_nnz.ptr;
  y.mcol = d_mcol.ptr;
  y.mval = d_mval.ptr;
  y.row_nnz = d_row_nnz.ptr;
  y.missing = d_missing.ptr;
  hipLaunchKernelGGL(k_sym_rows_seg<false>, dim3(grid_for(T, kWaves)), dim3(kThreads), 0, stream, y);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(asp::exclusive_scan_u32(d_row_nnz.ptr, T, d_row_start.ptr, d_scratch.ptr, stream));
  int64_t total = 0;
  unsigned long long missing[2] = {0, 0};
  ASP_HIP_TRY(hipMemcpyAsync(&total, d_row_start.ptr + T, sizeof total, hipMemcpyDeviceToHost, stream));
  ASP_TRY(d_missing.download(missing, 2, stream));
  ASP_TRY(sym.fetch(stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  ASP_TRY(sym.check());  // (a coefficient divided by a zero norm reached sums that are dropped here)
  if (missing[0] != 0) {
    return asp::set_error(ASP_ERR_INVALID,
                          "%llu couplings have no mirror element (one-directional matrix elements), the "
                          "first in segment %llu: use the host route",
                          missing[0], missing[1]);
  }
  *o.nnz = static_cast<uint64_t>(total);
  if (o.sizing()) {
    ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
    ASP_HIP_TRY(hipStreamSynchronize(stream));
    events.finish();
    return ASP_OK;
  }
  ASP_TRY(o.fits());
  ASP_TRY(d_col.alloc(*o.nnz));
  ASP_TRY(d_val.alloc(*o.nnz));
  y.row_start = d_row_start.ptr;
  y.col = d_col.ptr;
  y.val = d_val.ptr;
  hipLaunchKernelGGL(k_sym_rows_seg<true>, dim3(grid_for(T, kWaves)), dim3(kThreads), 0, stream, y);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  ASP_TRY(d_row_start.download(o.indptr, T + 1, stream));
  ASP_TRY(d_col.download(o.col, *o.nnz, stream));
  ASP_TRY(d_val.download(o.val, *o.nnz, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  events.finish();
  return ASP_OK;
}

}  // namespace

extern "C" int asp_operator_ising_segments(asp_operator const *op, uint64_t num_segments,
                                           uint64_t const *offsets, uint64_t const *keys,
                                           double const *psi, uint64_t capacity, int64_t *indptr,
                                           int32_t *col, double *val, uint64_t *nnz) {
  asp_clear_error();
  // (pointer checks before anything is dereferenced; every check before any device work and before
  // any output is written)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  if (!nnz) return asp::set_error(ASP_ERR_INVALID, "null nnz pointer");
  const uint64_t S = num_segments;
  if (S && !offsets) {
    return asp::set_error(ASP_ERR_INVALID, "null offsets with %llu segments", (unsigned long long)S);
  }
  if (S && offsets[0] != 0) return asp::set_error(ASP_ERR_INVALID, "offsets[0] is not 0");
  for (uint64_t g = 0; g < S; ++g) {
    if (offsets[g + 1] < offsets[g]) {
      return asp::set_error(ASP_ERR_INVALID, "offsets decrease at index %llu", (unsigned long long)(g + 1));
    }
  }
  const uint64_t T = S ? offsets[S] : 0;
  if (T >= 0x7FFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^31-2 table entries");
  if (T && (!keys || !psi)) {
    return asp::set_error(ASP_ERR_INVALID, "null keys or psi with %llu table entries", (unsigned long long)T);
  }
  for (uint64_t g = 0; g < S; ++g) {
    for (uint64_t i = offsets[g] + 1; i < offsets[g + 1]; ++i) {
      if (keys[i - 1] >= keys[i]) {
        return asp::set_error(ASP_ERR_INVALID,
                              "the keys of segment %llu are not sorted and unique at index %llu",
                              (unsigned long long)g, (unsigned long long)(i - offsets[g]));
      }
    }
  }
  if (T == 0) {
    *nnz = 0;
    if (indptr) indptr[0] = 0;
    return ASP_OK;
  }
  uint32_t row_capacity = 0;
  const size_t lds = lds_bytes(op, &row_capacity);
  if (lds > 160u * 1024u) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%u bonds, %u connections per row need %zu bytes of LDS per workgroup",
                          op->num_bonds, op->max_connections, lds);
  }
  *nnz = 0;
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  const Outputs o{capacity, indptr, col, val, nnz};
  if (op->unique_targets) {
    return segments_unique(op, S, offsets, keys, psi, row_capacity, lds, o, scoped.stream);
  }
  return segments_with_duplicates(op, S, offsets, keys, psi, row_capacity, lds, o, scoped.stream);
}
