// The boundary fields of many clusters in one call (specification ASP-FIELD-SEG-1), on
// gfx950: asp_operator_field over every segment of a concatenated table, in shared launches.  For segment
// g the result is, bit for bit, what asp_operator_field returns for its keys, amplitudes and environment
// alone: a connection of row r that leaves the cluster and ends in the environment state p of the SAME
// segment adds (coeff * |psi_r|) * env_psi[p] to ONE accumulator, in connection order from +0.0, every
// operation rounded, field[r] = scale * sum; a connection with a non-zero coefficient that ends in neither
// set of the segment is counted in unresolved[g].
//
// HBM layout: offsets u64[S+1], keys u64[T], psi f64[T]; env_offsets u64[S+1], env_keys u64[E], env_psi
//   f64[E] (segments concatenated, each ascending); row_segment u32[T]; TWO open-addressing hashes
//   {fingerprint:32 | global index+1:32}, u64[2^s >= 2T] over the cluster entries and u64[2^t >= 2E] over
//   the environment entries, both hashed with the per-segment salt of operator_ising_segments.hip, so that
//   a state present in every segment does not form one probe chain; out: field f64[T], unresolved u64[S].
// Mapping: k_segment_insert: one lane per entry of either table, row -> segment by bisection, CAS insert at
//   load factor <= 1/2.  The row kernels: one wavefront per table row, four rows per workgroup; the row's
//   segment goes through readfirstlane, so (salt, begin, end, env_begin, env_end) are scalar loads.
//   k_field_rows_seg: lanes over the bonds in chunks of 64, at most three transitions per lane;
//   k_field_list_seg: lanes over the row's entries of the device connection list (symmetry-adapted bases,
//   single-site flips), duplicates as separate terms.  A lane decides its connections with one hash (the
//   two tables share the salt) and one or two probes, each accepting only an entry of the row's own
//   segment; the terms enter the accumulator through the ballot walk of operator_field.hip, and the
//   accumulator carries over from chunk to chunk.  Lane 0 stores field[r].  No LDS, no atomics on the
//   field, no dependency between workgroups; the lost connections of a row are a wave reduction plus one
//   integer atomic add to unresolved[g].
// Host synchronisations per call, whatever S is: one (unique targets: the download) or two (the size of the
//   connection list, and the download).
// Traffic: 20 B/row + 16 B/environment entry in, 8 B/row out; the probes hit the L2-resident tables.
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

// (segment_of and segment_salt are those of operator_ising_segments.hip)
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

// entry -> segment for every entry of a table (cluster or environment), and the entry into that table's
// salted hash; row_segment may be null (the environment's rows are never walked).
__global__ __launch_bounds__(kThreads) void k_segment_insert(const uint64_t *__restrict__ keys, uint64_t total,
                                                            const uint64_t *__restrict__ offsets,
                                                            uint64_t num_segments,
                                                            uint32_t *__restrict__ row_segment,
                                                            unsigned long long *__restrict__ slots,
                                                            uint64_t mask) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= total) return;
  const uint64_t g = segment_of(offsets, num_segments, i);
  if (row_segment) row_segment[i] = static_cast<uint32_t>(g);
  const uint64_t h = mix64(keys[i] ^ segment_salt(g));
  const unsigned long long entry = (h & 0xFFFFFFFF00000000ull) | (i + 1);
  uint64_t at = h & mask;
  while (atomicCAS(&slots[at], 0ull, entry) != 0ull) at = (at + 1) & mask;
}

struct FieldSegArgs {
  const uint64_t *keys;
  const double *psi;
  const uint64_t *offsets;  // u64[S + 1]
  const uint32_t *row_segment;
  const unsigned long long *slots;  // hash of keys
  uint64_t mask;
  uint64_t total;  // T
  const uint64_t *env_keys;
  const double *env_psi;
  const uint64_t *env_offsets;          // u64[S + 1]
  const unsigned long long *env_slots;  // hash of env_keys
  uint64_t env_mask;
  double scale;
  double *field;
  unsigned long long *unresolved;  // u64[S]
  // k_field_rows_seg
  const Bond *bonds;
  uint32_t num_bonds;
  // k_field_list_seg
  const int64_t *list_offsets;
  const uint64_t *other_keys;
  const double *other_coeffs;
  const double *norms;                // symmetry-adapted basis: the source norms, else null
  unsigned long long *first_outside;  // the first segment with a row of norm 0
};

// What a row shares with its segment: wavefront-uniform.
struct Segment {
  uint32_t g;
  uint64_t salt, begin, end, env_begin, env_end;
};

__device__ __forceinline__ Segment segment_of_row(const FieldSegArgs &a, uint64_t r) {
  const uint32_t g = __builtin_amdgcn_readfirstlane(a.row_segment[r]);
  return Segment{g, segment_salt(g), a.offsets[g], a.offsets[g + 1], a.env_offsets[g], a.env_offsets[g + 1]};
}

// Is the key with hash h one of table[begin, end)?  Its global index, or -1.
__device__ __forceinline__ int64_t find_in_range(const unsigned long long *__restrict__ slots, uint64_t mask,
                                                 const uint64_t *__restrict__ table, uint64_t begin,
                                                 uint64_t end, uint64_t h, uint64_t needle) {
  const uint32_t fingerprint = static_cast<uint32_t>(h >> 32);
  for (uint64_t at = h & mask;; at = (at + 1) & mask) {
    const unsigned long long slot = slots[at];
    if (slot == 0) return -1;
    if (static_cast<uint32_t>(slot >> 32) != fingerprint) continue;
    const uint64_t idx = static_cast<uint32_t>(slot) - 1u;
    if (idx >= begin && idx < end && table[idx] == needle) return static_cast<int64_t>(idx);
  }
}

// One connection: its term when it leaves the cluster into the environment of the segment (*adds), else
// nothing; *lost when it ends in neither set of the segment with a non-zero coefficient.
__device__ __forceinline__ double boundary_term(const FieldSegArgs &a, const Segment &s, uint64_t target,
                                                double coeff, double psi_r, bool *adds, bool *lost) {
  *adds = false;
  *lost = false;
  const uint64_t h = mix64(target ^ s.salt);
  if (find_in_range(a.slots, a.mask, a.keys, s.begin, s.end, h, target) >= 0) return 0.0;
  const int64_t p = find_in_range(a.env_slots, a.env_mask, a.env_keys, s.env_begin, s.env_end, h, target);
  if (p < 0) {
    *lost = coeff != 0.0;
    return 0.0;
  }
  *adds = true;
  return __dmul_rn(__dmul_rn(coeff, psi_r), a.env_psi[p]);
}

// acc + the terms of the lanes in `who`, ascending lane order (wave-uniform walk)
__device__ __forceinline__ double add_in_lane_order(double acc, double term, uint64_t who) {
  while (who) {
    const int j = __builtin_ctzll(who);
    acc = __dadd_rn(acc, __shfl(term, j, 64));
    who &= who - 1;
  }
  return acc;
}

__device__ __forceinline__ void finish_row(const FieldSegArgs &a, const Segment &s, uint64_t r, uint32_t lane,
                                           double acc, uint32_t lost) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) lost += __shfl_xor(lost, step, 64);
  if (lane == 0) {
    a.field[r] = __dmul_rn(a.scale, acc);
    if (lost) atomicAdd(&a.unresolved[s.g], static_cast<unsigned long long>(lost));
  }
}

__global__ __launch_bounds__(kThreads) void k_field_rows_seg(FieldSegArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  // (the wave index through readfirstlane: provably wavefront-uniform, so what the row shares sits in SGPRs)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.total) return;  // whole wavefront; no barrier below
  const Segment s = segment_of_row(a, r);
  const uint64_t key = a.keys[r];
  const double psi_r = fabs(a.psi[r]);
  double acc = 0.0;
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
        const double x = boundary_term(a, s, key ^ bond.flip[src ^ dst], c, psi_r, &adds, &miss);
        lost += miss ? 1u : 0u;
        // (constant indices: the three slots stay in registers)
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
  finish_row(a, s, r, lane, acc, lost);
}

__global__ __launch_bounds__(kThreads) void k_field_list_seg(FieldSegArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.total) return;  // whole wavefront; no barrier below
  const Segment s = segment_of_row(a, r);
  // a row outside the sector: the call fails, and its message names the first such segment
  if (a.norms && lane == 0 && a.norms[r] == 0.0) atomicMin(a.first_outside, static_cast<unsigned long long>(s.g));
  const double psi_r = fabs(a.psi[r]);
  const int64_t begin = a.list_offsets[r], end = a.list_offsets[r + 1];
  double acc = 0.0;
  uint32_t lost = 0;
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t e = base + lane;
    double t = 0.0;
    bool adds = false, miss = false;
    if (e < end) t = boundary_term(a, s, a.other_keys[e], a.other_coeffs[e], psi_r, &adds, &miss);
    lost += miss ? 1u : 0u;
    acc = add_in_lane_order(acc, t, __ballot(adds));
  }
  finish_row(a, s, r, lane, acc, lost);
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
  void finish() const {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) asp::set_operator_last_ms(ms);
  }
  ~Events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

// offsets of one kind ("" or "environment "): from 0, non-decreasing
int check_offsets(const char *what, uint64_t S, const uint64_t *offsets) {
  if (S && !offsets) {
    return asp::set_error(ASP_ERR_INVALID, "null %soffsets with %llu segments", what, (unsigned long long)S);
  }
  if (S && offsets[0] != 0) return asp::set_error(ASP_ERR_INVALID, "%soffsets[0] is not 0", what);
  for (uint64_t g = 0; g < S; ++g) {
    if (offsets[g + 1] < offsets[g]) {
      return asp::set_error(ASP_ERR_INVALID, "%soffsets decrease at index %llu", what,
                            (unsigned long long)(g + 1));
    }
  }
  return ASP_OK;
}

int check_ascending(const char *what, uint64_t S, const uint64_t *offsets, const uint64_t *keys) {
  for (uint64_t g = 0; g < S; ++g) {
    for (uint64_t i = offsets[g] + 1; i < offsets[g + 1]; ++i) {
      if (keys[i - 1] >= keys[i]) {
        return asp::set_error(ASP_ERR_INVALID,
                              "the %skeys of segment %llu are not sorted and unique at index %llu", what,
                              (unsigned long long)g, (unsigned long long)(i - offsets[g]));
      }
    }
  }
  return ASP_OK;
}

}  // namespace

extern "C" int asp_operator_field_segments(asp_operator const *op, uint64_t num_segments,
                                           uint64_t const *offsets, uint64_t const *keys, double const *psi,
                                           uint64_t const *env_offsets, uint64_t const *env_keys,
                                           double const *env_psi, double scale, double *field,
                                           uint64_t *unresolved) {
  asp_clear_error();
  // (pointer checks before anything is dereferenced; every check before any device work and before any
  // output is written; the handle is not read before the tables have passed)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  const uint64_t S = num_segments;
  ASP_TRY(check_offsets("", S, offsets));
  ASP_TRY(check_offsets("environment ", S, env_offsets));
  const uint64_t T = S ? offsets[S] : 0, E = S ? env_offsets[S] : 0;
  if (T >= 0xFFFFFFFFull || E >= 0xFFFFFFFFull) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 table entries or environment entries");
  }
  if (T && (!keys || !psi || !field)) {
    return asp::set_error(ASP_ERR_INVALID, "null keys, psi or field with %llu table entries",
                          (unsigned long long)T);
  }
  if (E && (!env_keys || !env_psi)) {
    return asp::set_error(ASP_ERR_INVALID, "null environment arrays with %llu environment entries",
                          (unsigned long long)E);
  }
  ASP_TRY(check_ascending("", S, offsets, keys));
  ASP_TRY(check_ascending("environment ", S, env_offsets, env_keys));
  if (T == 0) {
    if (unresolved) std::fill(unresolved, unresolved + S, 0ull);
    return ASP_OK;
  }
  if (!op->unique_targets && T > 0xFFFFFFFFull / std::max<uint32_t>(op->max_connections, 1u)) {
    // (an upper bound, so that it is known before any launch: every key has at most max_connections)
    return asp::set_error(ASP_ERR_TOO_LARGE, "%llu table entries of at most %u connections: 2^32 or more",
                          (unsigned long long)T, op->max_connections);
  }
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  const uint64_t slots_n = slots_for(T), env_slots_n = slots_for(E);
  asp::ConnectionList list;
  asp::Symmetrised sym;
  DeviceBuffer<uint64_t> d_keys, d_offsets, d_env_keys, d_env_offsets;
  DeviceBuffer<double> d_psi, d_env_psi, d_field;
  DeviceBuffer<unsigned long long> d_slots, d_env_slots, d_unresolved;  // d_unresolved: u64[S] | first_outside
  DeviceBuffer<uint32_t> d_row_segment;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_psi.alloc(T));
  ASP_TRY(d_offsets.alloc(S + 1));
  ASP_TRY(d_env_keys.alloc(E));
  ASP_TRY(d_env_psi.alloc(E));
  ASP_TRY(d_env_offsets.alloc(S + 1));
  ASP_TRY(d_field.alloc(T));
  ASP_TRY(d_slots.alloc(slots_n));
  ASP_TRY(d_env_slots.alloc(env_slots_n));
  ASP_TRY(d_unresolved.alloc(S + 1));
  ASP_TRY(d_row_segment.alloc(T));
  ASP_TRY(events.create());
  ASP_TRY(d_psi.upload(psi, T, stream));
  ASP_TRY(d_offsets.upload(offsets, S + 1, stream));
  ASP_TRY(d_env_keys.upload(env_keys, E, stream));
  ASP_TRY(d_env_psi.upload(env_psi, E, stream));
  ASP_TRY(d_env_offsets.upload(env_offsets, S + 1, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  const uint64_t *device_keys = nullptr;
  if (op->unique_targets) {
    ASP_TRY(d_keys.alloc(T));
    ASP_TRY(d_keys.upload(keys, T, stream));
    device_keys = d_keys.ptr;
  } else {
    // rows may reach a state twice: the walk runs over the connection list of every key of the table (per
    // key: the order of the keys does not matter); the keys are uploaded there, once.  First
    // synchronisation: the size of the list.
    ASP_TRY(asp::connection_list_queue(op, T, keys, &list, &sym, stream));
    device_keys = list.batch.d_keys.ptr;
  }
  ASP_HIP_TRY(hipMemsetAsync(d_slots.ptr, 0, slots_n * sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_env_slots.ptr, 0, env_slots_n * sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_unresolved.ptr, 0, S * sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_unresolved.ptr + S, 0xFF, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_segment_insert, dim3(grid_for(T, kThreads)), dim3(kThreads), 0, stream, device_keys, T,
                     d_offsets.ptr, S, d_row_segment.ptr, d_slots.ptr, slots_n - 1);
  ASP_HIP_TRY(hipGetLastError());
  if (E) {
    hipLaunchKernelGGL(k_segment_insert, dim3(grid_for(E, kThreads)), dim3(kThreads), 0, stream,
                       d_env_keys.ptr, E, d_env_offsets.ptr, S, static_cast<uint32_t *>(nullptr),
                       d_env_slots.ptr, env_slots_n - 1);
    ASP_HIP_TRY(hipGetLastError());
  }
  FieldSegArgs a{};
  a.keys = device_keys;
  a.psi = d_psi.ptr;
  a.offsets = d_offsets.ptr;
  a.row_segment = d_row_segment.ptr;
  a.slots = d_slots.ptr;
  a.mask = slots_n - 1;
  a.total = T;
  a.env_keys = d_env_keys.ptr;
  a.env_psi = d_env_psi.ptr;
  a.env_offsets = d_env_offsets.ptr;
  a.env_slots = d_env_slots.ptr;
  a.env_mask = env_slots_n - 1;
  a.scale = scale;
  a.field = d_field.ptr;
  a.unresolved = d_unresolved.ptr;
  if (op->unique_targets) {
    a.bonds = op->d_bonds.ptr;
    a.num_bonds = op->num_bonds;
    hipLaunchKernelGGL(k_field_rows_seg, dim3(grid_for(T, kWaves)), dim3(kThreads), 0, stream, a);
  } else {
    a.list_offsets = list.batch.d_offsets.ptr;
    a.other_keys = list.d_other.ptr;
    a.other_coeffs = list.d_coeffs.ptr;
    a.norms = sym.d_norms.ptr;
    a.first_outside = d_unresolved.ptr + S;
    hipLaunchKernelGGL(k_field_list_seg, dim3(grid_for(T, kWaves)), dim3(kThreads), 0, stream, a);
  }
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  // (the results wait on the host until the sector check has passed: no output is written before it)
  std::vector<double> h_field(T);
  std::vector<unsigned long long> h_unresolved(S + 1);
  ASP_TRY(d_field.download(h_field.data(), T, stream));
  ASP_TRY(d_unresolved.download(h_unresolved.data(), S + 1, stream));
  ASP_TRY(sym.fetch(stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  if (sym.outside != 0) {
    // (a coefficient divided by a zero norm reached sums that are dropped here)
    return asp::set_error(ASP_ERR_INVALID,
                          "%llu states lie outside the symmetry sector (norm 0: an element of their "
                          "stabiliser has character -1), the first in segment %llu; they are not basis states",
                          sym.outside, h_unresolved[S]);
  }
  events.finish();
  std::copy(h_field.begin(), h_field.end(), field);
  if (unresolved) std::copy(h_unresolved.begin(), h_unresolved.begin() + S, unresolved);
  return ASP_OK;
}
