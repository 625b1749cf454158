// Internals of asp_operator shared by operator_apply.hip, operator_field.hip, operator_local_energy.hip,
// operator_ising_segments.hip and sector_basis.hip.
#pragma once

#include <cstdint>
#include <vector>

#include "asp_common.hpp"

namespace asp {

struct Bond {
  double m[16];  // m[dst * 4 + src]
  uint32_t a, b;
  uint64_t flip[4];  // flip[x] = key bits toggled by a transition with src ^ dst == x
};

struct SymmetryArgs {
  const uint8_t *table;  // [num_permutations][64]
  uint32_t num_permutations;
  uint32_t number_spins;
  int32_t inversion;  // 0, +1, -1
  uint64_t mask;      // low number_spins bits
};

// ---- the cluster's key hash (device side) -----------------------------------
// slots u64[2^s]: open addressing, {fingerprint:32 | index+1:32}, 0 = empty; filled by
// asp::key_hash_build (k_key_insert, operator_apply.hip).
#ifdef __HIPCC__
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// Index of `needle` in keys, or -1.
__device__ __forceinline__ int64_t find_key(const unsigned long long *__restrict__ slots,
                                            uint64_t mask, const uint64_t *__restrict__ keys,
                                            uint64_t needle) {
  const uint64_t h = mix64(needle);
  const uint32_t fingerprint = static_cast<uint32_t>(h >> 32);
  for (uint64_t at = h & mask;; at = (at + 1) & mask) {
    const unsigned long long slot = slots[at];
    if (slot == 0) return -1;
    if (static_cast<uint32_t>(slot >> 32) != fingerprint) continue;
    const uint32_t idx = static_cast<uint32_t>(slot) - 1u;
    if (keys[idx] == needle) return idx;
  }
}
#endif

// other_counts / offsets / total of a batch; on return the inputs are resident.
struct ApplyBatch {
  DeviceBuffer<uint64_t> d_keys;
  DeviceBuffer<int64_t> d_counts, d_offsets, d_scratch;
  uint64_t total = 0;
};

// The connections of a batch as asp_operator_apply returns them, left on the device: row r's
// entries at [batch.d_offsets[r], batch.d_offsets[r + 1]), the diagonal entry first; for a
// symmetry-adapted basis the representatives and rescaled coefficients, duplicates kept.
struct ConnectionList {
  ApplyBatch batch;
  DeviceBuffer<uint64_t> d_other;
  DeviceBuffer<double> d_coeffs;
};

// What the symmetrise pass leaves behind besides the entries: the source norms and the number of
// sources outside the sector (norm 0), which the caller reads with the next size it copies back.
struct Symmetrised {
  DeviceBuffer<double> d_norms;
  DeviceBuffer<unsigned long long> d_outside;
  unsigned long long outside = 0;
  // queues the copy of the counter (no-op for a plain basis); valid after the next synchronisation
  int fetch(hipStream_t stream) {
    if (!d_outside.ptr) return ASP_OK;
    return d_outside.download(&outside, 1, stream);
  }
  // after that synchronisation: ASP_ERR_INVALID when a source lies outside the sector
  int check() const {
    if (outside == 0) return ASP_OK;
    return set_error(ASP_ERR_INVALID,
                     "%llu states lie outside the symmetry sector (norm 0: an element of their "
                     "stabiliser has character -1); they are not basis states", outside);
  }
};

}  // namespace asp

struct asp_operator;

namespace asp {

// Fills `out` on `stream` and waits for it; ASP_ERR_INVALID when a key lies outside the symmetry
// sector (norm 0).  Declare a StreamFence after `out`.
int connection_list(const asp_operator *op, uint64_t n, const uint64_t *keys, ConnectionList *out,
                    hipStream_t stream);
// connection_list up to its last wait: the entries are queued on `stream`, and the sources outside the
// sector are counted in `sym` (Symmetrised::fetch, a synchronisation, then check).  The caller holds a
// StreamFence declared after `out` and `sym`.
int connection_list_queue(const asp_operator *op, uint64_t n, const uint64_t *keys, ConnectionList *out,
                          Symmetrised *sym, hipStream_t stream);
// connection_list_queue in EXTENSION mode (asp_operator_extend's): in out->d_other the targets of a
// symmetry-adapted basis are representatives, and a target of norm 0 is the "no state" value
// op->symmetry().mask; out->d_coeffs is scratch.  One synchronisation inside (the connection count).
int extension_list_queue(const asp_operator *op, uint64_t n, const uint64_t *keys, ConnectionList *out,
                         Symmetrised *sym, hipStream_t stream);
// extension_list_queue for n keys that are ALREADY on the device: the caller has allocated out->batch.d_keys and
// queued on `stream` whatever fills its first n entries; no upload.  The other buffers of `out` only grow, so a
// caller that comes back pass after pass (asp_operator_grow_segments) keeps them; call it when nothing queued
// earlier on `stream` still reads them.  One synchronisation inside (the connection count).
int extension_list_queue_device(const asp_operator *op, uint64_t n, ConnectionList *out, Symmetrised *sym,
                                hipStream_t stream);
// Clears slots[slots_n] (a power of two >= 2n) and inserts the n device keys.
int key_hash_build(const uint64_t *d_keys, uint64_t n, unsigned long long *d_slots, uint64_t slots_n,
                   hipStream_t stream);
// What asp_operator_last_ms reports for the calling thread.
void set_operator_last_ms(float ms);

}  // namespace asp

struct asp_operator {
  uint32_t number_spins = 0;
  uint32_t num_bonds = 0;
  uint32_t max_connections = 1;
  bool unique_targets = true;
  std::vector<asp::Bond> bonds;
  asp::DeviceBuffer<asp::Bond> d_bonds;
  // symmetry-adapted basis (asp_operator_set_symmetry); num_permutations == 0: plain basis
  uint32_t num_permutations = 0;
  int32_t inversion = 0;
  asp::DeviceBuffer<uint8_t> d_table;
  asp::SymmetryArgs symmetry() const {
    return asp::SymmetryArgs{d_table.ptr, num_permutations, number_spins, inversion,
                        number_spins >= 64 ? ~0ull : ((1ull << number_spins) - 1ull)};
  }
};

