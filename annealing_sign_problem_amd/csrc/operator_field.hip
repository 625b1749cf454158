// Boundary field of a cluster (specification ASP-FIELD-1), on gfx950: the miss
// branch of the reference's coupling build (cbits/build_matrix.c:49).  A connection of row r that
// leaves the cluster and ends in an environment state p adds
//   (coeff * |psi_r|) * env_psi[p]
// to field[r]; the adds run strictly in connection order from +0.0, every operation rounded, and
// field[r] = scale * sum.  A connection that ends neither in the cluster nor in the environment
// contributes nothing and is counted in `unresolved` when its coefficient is non-zero.
//
// HBM layout: keys u64[K], psi f64[K], env_keys u64[E], env_psi f64[E] (all sorted by key);
//   two open-addressing hashes {fingerprint:32 | index+1:32}, u64[2^s >= 2K] and u64[2^t >= 2E]
//   (asp::key_hash_build, the insert path of the coupling build); out: field f64[K].
// Mapping: one wavefront per row.  k_field_rows: lanes over the bonds in chunks of 64, at most
//   three transitions per lane; k_field_list: lanes over the row's entries of the device connection
//   list (symmetry-adapted bases, single-site flips), duplicates as separate terms.  Each lane
//   decides its connections with one or two hash probes; the terms then enter ONE accumulator in
//   connection order — the contributing lanes are walked through a ballot, the value read from
//   the owning lane — and the accumulator carries over from chunk to chunk.  Lane 0 stores
//   field[r].  No atomics on the field; `unresolved` is a wave reduction plus one atomic add.
// Traffic: 16 B/row in, 8 B/row out; the probes hit L2-resident tables.  Integer/latency-bound.
#include <vector>

#include "asp_common.hpp"
#include "operator_internal.hpp"

namespace {

using asp::Bond;
using asp::DeviceBuffer;
using asp::find_key;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct FieldArgs {
  const uint64_t *keys;
  const double *psi;
  const unsigned long long *slots;      // hash of keys
  uint64_t mask;
  const uint64_t *env_keys;
  const double *env_psi;
  const unsigned long long *env_slots;  // hash of env_keys
  uint64_t env_mask;
  uint64_t num_spins;
  double scale;
  double *field;
  unsigned long long *unresolved;
  // k_field_rows
  const Bond *bonds;
  uint32_t num_bonds;
  // k_field_list
  const int64_t *offsets;
  const uint64_t *other_keys;
  const double *other_coeffs;
};

// One connection: its term when it leaves the cluster into the environment (*adds), else nothing;
// *lost when it ends in neither set with a non-zero coefficient.
__device__ __forceinline__ double boundary_term(const FieldArgs &a, uint64_t target, double coeff,
                                                double psi_r, bool *adds, bool *lost) {
  *adds = false;
  *lost = false;
  if (find_key(a.slots, a.mask, a.keys, target) >= 0) return 0.0;
  const int64_t p = find_key(a.env_slots, a.env_mask, a.env_keys, target);
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

__device__ __forceinline__ void finish_row(const FieldArgs &a, uint64_t r, uint32_t lane, double acc,
                                           uint32_t lost) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) lost += __shfl_xor(lost, step, 64);
  if (lane == 0) {
    a.field[r] = __dmul_rn(a.scale, acc);
    if (lost) atomicAdd(a.unresolved, static_cast<unsigned long long>(lost));
  }
}

__global__ __launch_bounds__(kThreads) void k_field_rows(FieldArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (r >= a.num_spins) return;  // whole wavefront; no barrier below
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
        const double x = boundary_term(a, key ^ bond.flip[src ^ dst], c, psi_r, &adds, &miss);
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
  finish_row(a, r, lane, acc, lost);
}

__global__ __launch_bounds__(kThreads) void k_field_list(FieldArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (r >= a.num_spins) return;  // whole wavefront; no barrier below
  const double psi_r = fabs(a.psi[r]);
  const int64_t begin = a.offsets[r], end = a.offsets[r + 1];
  double acc = 0.0;
  uint32_t lost = 0;
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t e = base + lane;
    double t = 0.0;
    bool adds = false, miss = false;
    if (e < end) t = boundary_term(a, a.other_keys[e], a.other_coeffs[e], psi_r, &adds, &miss);
    lost += miss ? 1u : 0u;
    acc = add_in_lane_order(acc, t, __ballot(adds));
  }
  finish_row(a, r, lane, acc, lost);
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  return static_cast<unsigned>((items + per_block - 1) / per_block);
}

uint64_t slots_for(uint64_t n) {
  uint64_t slots_n = 1024;
  while (slots_n < 2 * n) slots_n <<= 1;
  return slots_n;
}

bool ascending(const uint64_t *keys, uint64_t n) {
  for (uint64_t i = 1; i < n; ++i) {
    if (keys[i - 1] >= keys[i]) return false;
  }
  return true;
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

extern "C" int asp_operator_field(asp_operator const *op, uint64_t num_spins, uint64_t const *keys,
                                  double const *psi, uint64_t num_env, uint64_t const *env_keys,
                                  double const *env_psi, double scale, double *field,
                                  uint64_t *unresolved) {
  asp_clear_error();
  // (pointer checks only up to here: nothing is dereferenced before they pass)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  const uint64_t K = num_spins, E = num_env;
  if (K && (!keys || !psi || !field)) {
    return asp::set_error(ASP_ERR_INVALID, "null keys, psi or field with %llu spins",
                          (unsigned long long)K);
  }
  if (E && (!env_keys || !env_psi)) {
    return asp::set_error(ASP_ERR_INVALID, "null environment arrays with %llu environment states",
                          (unsigned long long)E);
  }
  if (K >= 0x7FFFFFFFull || E >= 0xFFFFFFFFull) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^31-1 spins or 2^32-2 environment states");
  }
  if (!ascending(keys, K)) return asp::set_error(ASP_ERR_INVALID, "keys are not sorted and unique");
  if (!ascending(env_keys, E)) {
    return asp::set_error(ASP_ERR_INVALID, "environment keys are not sorted and unique");
  }
  if (unresolved) *unresolved = 0;
  if (K == 0) return ASP_OK;
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  const uint64_t slots_n = slots_for(K), env_slots_n = slots_for(E);
  asp::ConnectionList list;
  DeviceBuffer<uint64_t> d_keys, d_env_keys;
  DeviceBuffer<double> d_psi, d_env_psi, d_field;
  DeviceBuffer<unsigned long long> d_slots, d_env_slots, d_unresolved;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_psi.alloc(K));
  ASP_TRY(d_env_keys.alloc(E));
  ASP_TRY(d_env_psi.alloc(E));
  ASP_TRY(d_field.alloc(K));
  ASP_TRY(d_slots.alloc(slots_n));
  ASP_TRY(d_env_slots.alloc(env_slots_n));
  ASP_TRY(d_unresolved.alloc(1));
  ASP_TRY(events.create());
  ASP_TRY(d_psi.upload(psi, K, stream));
  ASP_TRY(d_env_keys.upload(env_keys, E, stream));
  ASP_TRY(d_env_psi.upload(env_psi, E, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  const uint64_t *device_keys = nullptr;
  if (op->unique_targets) {
    ASP_TRY(d_keys.alloc(K));
    ASP_TRY(d_keys.upload(keys, K, stream));
    device_keys = d_keys.ptr;
  } else {
    // rows may reach a state twice: the walk runs over the connection list of the
    // duplicate-keeping coupling build (fails here for a key of norm 0)
    ASP_TRY(asp::connection_list(op, K, keys, &list, stream));
    device_keys = list.batch.d_keys.ptr;
  }
  ASP_TRY(asp::key_hash_build(device_keys, K, d_slots.ptr, slots_n, stream));
  ASP_TRY(asp::key_hash_build(d_env_keys.ptr, E, d_env_slots.ptr, env_slots_n, stream));
  ASP_HIP_TRY(hipMemsetAsync(d_unresolved.ptr, 0, sizeof(unsigned long long), stream));
  FieldArgs a{};
  a.keys = device_keys;
  a.psi = d_psi.ptr;
  a.slots = d_slots.ptr;
  a.mask = slots_n - 1;
  a.env_keys = d_env_keys.ptr;
  a.env_psi = d_env_psi.ptr;
  a.env_slots = d_env_slots.ptr;
  a.env_mask = env_slots_n - 1;
  a.num_spins = K;
  a.scale = scale;
  a.field = d_field.ptr;
  a.unresolved = d_unresolved.ptr;
  if (op->unique_targets) {
    a.bonds = op->d_bonds.ptr;
    a.num_bonds = op->num_bonds;
    hipLaunchKernelGGL(k_field_rows, dim3(grid_for(K, kWaves)), dim3(kThreads), 0, stream, a);
  } else {
    a.offsets = list.batch.d_offsets.ptr;
    a.other_keys = list.d_other.ptr;
    a.other_coeffs = list.d_coeffs.ptr;
    hipLaunchKernelGGL(k_field_list, dim3(grid_for(K, kWaves)), dim3(kThreads), 0, stream, a);
  }
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  unsigned long long lost = 0;
  ASP_TRY(d_field.download(field, K, stream));
  ASP_TRY(d_unresolved.download(&lost, 1, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, events.ev0, events.ev1) == hipSuccess) asp::set_operator_last_ms(ms);
  if (unresolved) *unresolved = lost;
  return ASP_OK;
}
