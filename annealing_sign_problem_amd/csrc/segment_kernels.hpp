// What the segmented device calls share (level_segments.hip: cutoff and extension of a round; cluster_grow.hip:
// the growth of a round): the launch geometry, the event pair, the segment search and the flag-first /
// scatter-first kernels that turn per-segment sorted runs into per-segment unique lists.  Everything sits in an
// anonymous namespace: each translation unit that includes this header gets its own kernels.
#pragma once

#include <cstdint>

#include "asp_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

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
  float elapsed() const {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess ? ms : 0.0f;
  }
  ~Events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

// The segment whose range holds item i: offsets[g] <= i < offsets[g + 1] (empty segments are skipped).
__device__ __forceinline__ uint32_t segment_of(const uint64_t *__restrict__ offsets, uint64_t num_segments,
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
  return static_cast<uint32_t>(lo);
}

// segment_start[g] = connection offset of segment g's first key (g = 0 ... G: the last one is N), and a 1
// in flag[] at the first connection of every non-empty segment (flag[] was cleared).  (The growth compacts before
// it sorts and has a start kernel of its own: not every includer launches this one.)
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_segment_starts(const uint64_t *__restrict__ offsets,
                                                            uint64_t num_segments,
                                                            const int64_t *__restrict__ connection_offsets,
                                                            uint64_t connections,
                                                            uint32_t *__restrict__ segment_start,
                                                            uint32_t *__restrict__ flag) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g > num_segments) return;
  const uint64_t start = static_cast<uint64_t>(connection_offsets[offsets[g]]);
  segment_start[g] = static_cast<uint32_t>(start);
  if (g < num_segments && offsets[g + 1] > offsets[g] && start < connections) flag[start] = 1u;
}

// flag[i] (on entry: 1 at a segment's first connection) = first of its run WITHIN the segment and not
// the "no state" value `drop` (left out when `dropping`).
__global__ __launch_bounds__(kThreads) void k_flag_first_seg(const uint64_t *__restrict__ sorted, uint64_t n,
                                                            bool dropping, uint64_t drop,
                                                            uint32_t *__restrict__ flag) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const bool first = flag[i] != 0u || i == 0 || sorted[i] != sorted[i - 1];
  flag[i] = (first && !(dropping && sorted[i] == drop)) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void k_segment_counts(const uint32_t *__restrict__ segment_start,
                                                            uint64_t num_segments,
                                                            const int64_t *__restrict__ position,
                                                            int64_t *__restrict__ out_offsets) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g <= num_segments) out_offsets[g] = position[segment_start[g]];
}

__global__ __launch_bounds__(kThreads) void k_scatter_first(const uint64_t *__restrict__ sorted, uint64_t n,
                                                           const uint32_t *__restrict__ flag,
                                                           const int64_t *__restrict__ position,
                                                           uint64_t *__restrict__ out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) out[position[i]] = sorted[i];
}

}  // namespace
