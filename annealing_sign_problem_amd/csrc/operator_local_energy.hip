// Local energies of signed amplitudes over many small tables in one call (specification ASP-ELOC-1,
// DESIGN.md §3.7), on gfx950: the sibling of the boundary field (operator_field.hip) that keeps EVERY
// connection of a row, the diagonal included, reads signed amplitudes and divides by the row's own:
//   hphi[r] = sum_e coeff_e * phi[p_e]      eloc[r] = hphi[r] / phi[rows[r]]
// over the entries asp_operator_apply returns for the row's key, in its order, p_e the position of the
// target among the keys of the row's OWN segment.  The adds run strictly in connection order from +0.0,
// every operation rounded.  A target outside the segment contributes nothing and is counted in
// missing[r] when its coefficient is non-zero.
//
// HBM layout: offsets u64[S+1]; keys u64[T], phi f64[T] (segments concatenated, each ascending);
//   rows u64[N], row_segment u32[N]; ONE open-addressing hash over all T entries
//   {fingerprint:32 | global index+1:32}, u64[2^s >= 2T], hashed with a per-segment salt
//   (k_segment_insert), so that a state present in every segment does not form one probe chain;
//   out: hphi f64[N], eloc f64[N], missing u32[N].
// Mapping: one wavefront per row, four rows per workgroup.  k_eloc_rows: lanes over the bonds in
//   chunks of 64, at most three transitions per lane, the diagonal by k_apply's left-to-right sum in a
//   pass of its own (it is the FIRST term); k_eloc_list: lanes over the row's entries of the device
//   connection list (symmetry-adapted bases, single-site flips), duplicates as separate terms.  Each
//   lane decides its connections with one probe; the terms then enter ONE accumulator in connection
//   order — the contributing lanes are walked through a ballot, the value read from the owning lane —
//   and the accumulator carries over from chunk to chunk.  Lane 0 stores the three outputs.  No
//   atomics and no reduction of the accumulator; `missing` is an integer wave reduction.
// Traffic: 12 B/row in, 20 B/row out; the probes hit the L2-resident table.  Integer/latency-bound.
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

// The segment of table entry i: the last g with offsets[g] <= i (empty segments share their start
// with the next one and are skipped by that rule).
__device__ __forceinline__ uint64_t segment_of(const uint64_t *__restrict__ offsets,
                                               uint64_t num_segments, uint64_t i) {
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

__global__ __launch_bounds__(kThreads) void k_segment_insert(const uint64_t *__restrict__ keys,
                                                            uint64_t total,
                                                            const uint64_t *__restrict__ offsets,
                                                            uint64_t num_segments,
                                                            unsigned long long *__restrict__ slots,
                                                            uint64_t mask) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= total) return;
  const uint64_t h = mix64(keys[i] ^ segment_salt(segment_of(offsets, num_segments, i)));
  const unsigned long long entry = (h & 0xFFFFFFFF00000000ull) | (i + 1);
  uint64_t at = h & mask;
  while (atomicCAS(&slots[at], 0ull, entry) != 0ull) at = (at + 1) & mask;
}

struct ElocArgs {
  const uint64_t *keys;
  const double *phi;
  const uint64_t *offsets;  // u64[S + 1]
  const unsigned long long *slots;
  uint64_t mask;
  const uint64_t *rows;
  const uint32_t *row_segment;
  uint64_t num_rows;
  double *hphi;
  double *eloc;
  uint32_t *missing;
  // k_eloc_rows
  const Bond *bonds;
  uint32_t num_bonds;
  // k_eloc_list
  const int64_t *list_offsets;
  const uint64_t *other_keys;
  const double *other_coeffs;
};

// What a row's probes share: the salt and the range of its segment.
struct Segment {
  uint64_t salt, begin, end;
};

// Global index of `needle` among the keys of the segment, or -1.  The table holds every segment's
// entries; an entry of another segment (or another key with the same fingerprint) is passed over.
__device__ __forceinline__ int64_t find_in_segment(const ElocArgs &a, const Segment &s, uint64_t needle) {
  const uint64_t h = mix64(needle ^ s.salt);
  const uint32_t fingerprint = static_cast<uint32_t>(h >> 32);
  for (uint64_t at = h & a.mask;; at = (at + 1) & a.mask) {
    const unsigned long long slot = a.slots[at];
    if (slot == 0) return -1;
    if (static_cast<uint32_t>(slot >> 32) != fingerprint) continue;
    const uint64_t idx = static_cast<uint32_t>(slot) - 1u;
    if (idx >= s.begin && idx < s.end && a.keys[idx] == needle) return static_cast<int64_t>(idx);
  }
}

// One connection: coeff * phi[p] when the target is in the segment (*adds), else nothing; *lost when
// it is not and the coefficient is non-zero.
__device__ __forceinline__ double connection_term(const ElocArgs &a, const Segment &s, uint64_t target,
                                                  double coeff, bool *adds, bool *lost) {
  const int64_t p = find_in_segment(a, s, target);
  *adds = p >= 0;
  *lost = p < 0 && coeff != 0.0;
  return p >= 0 ? __dmul_rn(coeff, a.phi[p]) : 0.0;
}

__device__ __forceinline__ void finish_row(const ElocArgs &a, uint64_t r, uint64_t at, uint32_t lane,
                                           double acc, uint32_t lost) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) lost += __shfl_xor(lost, step, 64);
  if (lane == 0) {
    a.hphi[r] = acc;
    a.eloc[r] = __ddiv_rn(acc, a.phi[at]);
    a.missing[r] = lost;
  }
}

__global__ __launch_bounds__(kThreads) void k_eloc_rows(ElocArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  // (the wave index through readfirstlane: provably wavefront-uniform, so what the row shares sits in SGPRs)
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= a.num_rows) return;  // whole wavefront; no barrier below
  const uint64_t at = a.rows[r];
  const uint32_t g = a.row_segment[r];
  const Segment s{segment_salt(g), a.offsets[g], a.offsets[g + 1]};
  const uint64_t key = a.keys[at];
  // the first connection: the diagonal, the left-to-right sum over the bonds (k_apply); its target
  // is the row's own key, which the segment holds at `at`
  double diagonal = 0.0;
  for (uint32_t first = 0; first < a.num_bonds; first += 64u) {
    const uint32_t bi = first + lane;
    double dval = 0.0;
    if (bi < a.num_bonds) {
      const Bond &bond = a.bonds[bi];
      const uint32_t src =
          static_cast<uint32_t>(((key >> bond.a) & 1ull) * 2ull + ((key >> bond.b) & 1ull));
      dval = bond.m[src * 4u + src];
    }
    const uint32_t here = min(64u, a.num_bonds - first);
    for (uint32_t j = 0; j < here; ++j) diagonal = __dadd_rn(diagonal, __shfl(dval, j, 64));
  }
  double acc = __dadd_rn(0.0, __dmul_rn(diagonal, a.phi[at]));
  uint32_t lost = 0;
  for (uint32_t first = 0; first < a.num_bonds; first += 64u) {
    const uint32_t bi = first + lane;
    double t[3] = {0.0, 0.0, 0.0};
    bool on[3] = {false, false, false};
    if (bi < a.num_bonds) {
      const Bond &bond = a.bonds[bi];
      const uint32_t src =
          static_cast<uint32_t>(((key >> bond.a) & 1ull) * 2ull + ((key >> bond.b) & 1ull));
      uint32_t slot = 0;  // the lane's connections in dst order (k_apply's order)
#pragma unroll
      for (uint32_t dst = 0; dst < 4; ++dst) {
        const double c = bond.m[dst * 4u + src];
        if (dst == src || c == 0.0) continue;
        bool adds, miss;
        const double x = connection_term(a, s, key ^ bond.flip[src ^ dst], c, &adds, &miss);
        lost += miss ? 1u : 0u;
        if (slot == 0) { t[0] = x; on[0] = adds; }
        if (slot == 1) { t[1] = x; on[1] = adds; }
        if (slot == 2) { t[2] = x; on[2] = adds; }
        ++slot;
      }
    }
    const uint64_t w0 = __ballot(on[0]), w1 = __ballot(on[1]), w2 = __ballot(on[2]);
    // connection order: bond by bond, and within a bond by dst
    for (uint64_t who = w0 | w1 | w2; who; who &= who - 1) {
      const int j = __builtin_ctzll(who);
      if ((w0 >> j) & 1ull) acc = __dadd_rn(acc, __shfl(t[0], j, 64));
      if ((w1 >> j) & 1ull) acc = __dadd_rn(acc, __shfl(t[1], j, 64));
      if ((w2 >> j) & 1ull) acc = __dadd_rn(acc, __shfl(t[2], j, 64));
    }
  }
  finish_row(a, r, at, lane, acc, lost);
}

__global__ __launch_bounds__(kThreads) void k_eloc_list(ElocArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  // (the wave index through readfirstlane: provably wavefront-uniform, so what the row shares sits in SGPRs)
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= a.num_rows) return;  // whole wavefront; no barrier below
  const uint64_t at = a.rows[r];
  const uint32_t g = a.row_segment[r];
  const Segment s{segment_salt(g), a.offsets[g], a.offsets[g + 1]};
  const int64_t begin = a.list_offsets[r], end = a.list_offsets[r + 1];
  double acc = 0.0;
  uint32_t lost = 0;
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t e = base + lane;
    double t = 0.0;
    bool adds = false, miss = false;
    if (e < end) t = connection_term(a, s, a.other_keys[e], a.other_coeffs[e], &adds, &miss);
    lost += miss ? 1u : 0u;
    // acc + the terms of the contributing lanes, ascending lane order (wave-uniform walk)
    for (uint64_t who = __ballot(adds); who; who &= who - 1) {
      acc = __dadd_rn(acc, __shfl(t, __builtin_ctzll(who), 64));
    }
  }
  finish_row(a, r, at, lane, acc, lost);
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  return static_cast<unsigned>((items + per_block - 1) / per_block);
}

uint64_t slots_for(uint64_t n) {
  uint64_t slots_n = 1024;
  while (slots_n < 2 * n) slots_n <<= 1;
  return slots_n;
}

struct Events {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int create() {
    ASP_HIP_TRY(hipEventCreate(&ev0));
    ASP_HIP_TRY(hipEventCreate(&ev1));
    return ASP_OK;
  }
  ~Events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

}  // namespace

extern "C" int asp_operator_local_energy(asp_operator const *op, uint64_t num_segments,
                                         uint64_t const *offsets, uint64_t const *keys,
                                         double const *phi, uint64_t num_rows, uint64_t const *rows,
                                         double *hphi, double *eloc, uint32_t *missing) {
  asp_clear_error();
  // (pointer checks before anything is dereferenced; every check before any device work and before
  // any output is written)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  const uint64_t S = num_segments, N = num_rows;
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
  if (T >= 0xFFFFFFFFull || N >= 0x7FFFFFFFull) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 table entries or 2^31-2 rows");
  }
  if (T && (!keys || !phi)) {
    return asp::set_error(ASP_ERR_INVALID, "null keys or phi with %llu table entries", (unsigned long long)T);
  }
  for (uint64_t g = 0; g < S; ++g) {
    for (uint64_t i = offsets[g] + 1; i < offsets[g + 1]; ++i) {
      if (keys[i - 1] >= keys[i]) {
        return asp::set_error(ASP_ERR_INVALID, "the keys of segment %llu are not sorted and unique",
                              (unsigned long long)g);
      }
    }
  }
  if (N && !rows) return asp::set_error(ASP_ERR_INVALID, "null rows with %llu rows", (unsigned long long)N);
  for (uint64_t r = 0; r < N; ++r) {
    if (rows[r] >= T) {
      return asp::set_error(ASP_ERR_INVALID, "row %llu points at entry %llu of a table of %llu",
                            (unsigned long long)r, (unsigned long long)rows[r], (unsigned long long)T);
    }
  }
  if (eloc) {
    for (uint64_t r = 0; r < N; ++r) {
      const double x = phi[rows[r]];
      if (x == 0.0 || !(x == x) || x - x != 0.0) {
        return asp::set_error(ASP_ERR_INVALID, "row %llu has a zero, NaN or infinite amplitude: no local energy",
                              (unsigned long long)r);
      }
    }
  }
  if (N == 0) return ASP_OK;
  // the segment of every row: the last one that starts at or before its entry
  std::vector<uint32_t> row_segment(N);
  std::vector<uint64_t> row_keys;
  for (uint64_t r = 0; r < N; ++r) {
    row_segment[r] = static_cast<uint32_t>(std::upper_bound(offsets, offsets + S + 1, rows[r]) - offsets - 1);
  }
  if (!op->unique_targets) {
    row_keys.resize(N);
    for (uint64_t r = 0; r < N; ++r) row_keys[r] = keys[rows[r]];
  }
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  const uint64_t slots_n = slots_for(T);
  asp::ConnectionList list;
  DeviceBuffer<uint64_t> d_keys, d_offsets, d_rows;
  DeviceBuffer<double> d_phi, d_hphi, d_eloc;
  DeviceBuffer<uint32_t> d_row_segment, d_missing;
  DeviceBuffer<unsigned long long> d_slots;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_keys.alloc(T));
  ASP_TRY(d_phi.alloc(T));
  ASP_TRY(d_offsets.alloc(S + 1));
  ASP_TRY(d_rows.alloc(N));
  ASP_TRY(d_row_segment.alloc(N));
  ASP_TRY(d_hphi.alloc(N));
  ASP_TRY(d_eloc.alloc(N));
  ASP_TRY(d_missing.alloc(N));
  ASP_TRY(d_slots.alloc(slots_n));
  ASP_TRY(events.create());
  ASP_TRY(d_keys.upload(keys, T, stream));
  ASP_TRY(d_phi.upload(phi, T, stream));
  ASP_TRY(d_offsets.upload(offsets, S + 1, stream));
  ASP_TRY(d_rows.upload(rows, N, stream));
  ASP_TRY(d_row_segment.upload(row_segment.data(), N, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  if (!op->unique_targets) {
    // rows may reach a state twice: the walk runs over the connection list of the row keys (fails
    // here for a key of norm 0)
    ASP_TRY(asp::connection_list(op, N, row_keys.data(), &list, stream));
  }
  ASP_HIP_TRY(hipMemsetAsync(d_slots.ptr, 0, slots_n * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_segment_insert, dim3(grid_for(T, kThreads)), dim3(kThreads), 0, stream, d_keys.ptr, T,
                     d_offsets.ptr, S, d_slots.ptr, slots_n - 1);
  ASP_HIP_TRY(hipGetLastError());
  ElocArgs a{};
  a.keys = d_keys.ptr;
  a.phi = d_phi.ptr;
  a.offsets = d_offsets.ptr;
  a.slots = d_slots.ptr;
  a.mask = slots_n - 1;
  a.rows = d_rows.ptr;
  a.row_segment = d_row_segment.ptr;
  a.num_rows = N;
  a.hphi = d_hphi.ptr;
  a.eloc = d_eloc.ptr;
  a.missing = d_missing.ptr;
  if (op->unique_targets) {
    a.bonds = op->d_bonds.ptr;
    a.num_bonds = op->num_bonds;
    hipLaunchKernelGGL(k_eloc_rows, dim3(grid_for(N, kWaves)), dim3(kThreads), 0, stream, a);
  } else {
    a.list_offsets = list.batch.d_offsets.ptr;
    a.other_keys = list.d_other.ptr;
    a.other_coeffs = list.d_coeffs.ptr;
    hipLaunchKernelGGL(k_eloc_list, dim3(grid_for(N, kWaves)), dim3(kThreads), 0, stream, a);
  }
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  if (hphi) ASP_TRY(d_hphi.download(hphi, N, stream));
  if (eloc) ASP_TRY(d_eloc.download(eloc, N, stream));
  if (missing) ASP_TRY(d_missing.download(missing, N, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, events.ev0, events.ev1) == hipSuccess) asp::set_operator_last_ms(ms);
  return ASP_OK;
}
