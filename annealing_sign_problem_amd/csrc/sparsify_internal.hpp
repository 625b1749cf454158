// What sparsify.hip and level_segments.hip share: the lock-free union-find forest (smaller root wins,
// so the final root of a component is its smallest spin — deterministic) and the timing slot that
// asp_sparsify_last_ms reads.
#pragma once

#include <cstdint>

#include "asp_common.hpp"

namespace asp {

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x) {
  uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    const uint32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != p) {  // path halving: only ever replaces a parent by one of its ancestors
      __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  while (a != b) {
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }  // a > b: hang the larger root under the smaller
    const uint32_t seen = atomicCAS(&parent[a], a, b);
    if (seen == a) return;
    a = find_root(parent, seen);  // somebody re-rooted a meanwhile
    b = find_root(parent, b);
  }
}
#endif

// What asp_sparsify_last_ms reports for the calling thread (sparsify.hip).
void set_sparsify_last_ms(float ms);

}  // namespace asp
