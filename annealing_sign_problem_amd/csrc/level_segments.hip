// One level of a round of clusters in segmented device calls, on gfx950: the cutoff of ALL clusters
// (asp_sparsify_component_segments, specification ASP-SPARSIFY-SEG-1) and the one-hop
// extension of ALL clusters (asp_operator_extend_segments, ASP-EXTEND-SEG-1).  Between
// the two sits the existing asp_operator_ising_segments, whose output conventions are this file's input
// conventions: segments concatenated, ONE global indptr from 0, columns local to their segment.
//
// ---- asp_sparsify_component_segments ----
// For segment g the result is, bit for bit, what asp_sparsify_component (sparsify.hip) returns for the
// rebased segment with anchors[g].  The kernels there work on whole rows, one wavefront per row, so the
// concatenated table is balanced as it is; new is everything that knows about segments.
// HBM layout: offsets u64[G+1], anchors u64[G]; indptr i64[T+1], indices i32[nnz] (segment-local), data
//   f64[nnz], frozen u8[T]; row_segment u32[T]; max_bits u64[G] (bit pattern of max|data| per segment);
//   parent u32[T] — ONE union-find forest on GLOBAL spin numbers (col + offsets[g]); an edge never leaves
//   its segment, so neither does a component —, root u32[T]; keep u32[T] + keep8 u8[T]; stray u32[G],
//   first_stray u32; new_index i64[T+1] (scan of keep) -> kept_offsets i64[G+1]; row_kept u32[T] (per OLD
//   row, 0 for a dropped one) -> nnz_before i64[T+1] (scan) -> out_indptr i64[kept+1]; out_indices i32[],
//   out_data f64[].
// Kernels (one stream): k_row_segment -> k_segment_abs_max (wave reduction, then atomicMax on the bit
//   pattern of |x| into max_bits[g]: exact, the maximum is order-independent) -> k_init_parent ->
//   k_hook_edges_seg (threshold = __dmul_rn(reltol, max of the ROW'S segment), read on the device: the
//   single call's first synchronisation is gone) -> k_flatten -> k_mark_segments (against
//   root[offsets[g] + anchors[g]]; per-segment stray counters, atomicMin for the first stray segment) ->
//   scan -> k_segment_sums -> k_slice_seg<count> -> scan -> k_compact_indptr -> [sync] ->
//   k_slice_seg<emit> (local column = new_index[offsets[g] + col] - new_index[offsets[g]]) -> [sync].
// Launches: 13 plus the two scans', whatever G is.  Host synchronisations: ONE for the mask-only call,
// TWO for a full call (asp_sparsify_component: five), whatever G is.
//
// ---- asp_operator_extend_segments ----
// out[out_offsets[g] : out_offsets[g+1]] is asp_operator_extend of segment g's keys.  The action and the
// symmetrise pass do not care about segments and run ONCE over the concatenated keys
// (asp::extension_list_queue, operator_apply.hip).
// HBM layout: keys u64[T], connection offsets i64[T+1], targets u64[N] ("no state" = all sites up for the
//   norm-0 orbits of a -1 sector); segment_start u32[G+1] = connection offset of the segment's first key;
//   sorted u64[N]; flag u32[N]; position i64[N+1]; out u64[count]; out_offsets i64[G+1].
// Kernels: k_apply<count> -> scan -> [sync] -> k_apply<emit> -> symmetrise -> k_segment_starts (also puts a
//   1 into flag[] at every segment's first connection) -> rocprim::segmented_radix_sort_keys on the bits
//   [0, number_spins) with segment_start as the segment offsets (any number of sites, any number of
//   segments: nothing is packed above the key) -> k_flag_first_seg (first of a run OR first of a segment,
//   and not the "no state" value, which sorts last in EVERY segment) -> scan -> k_segment_counts -> [sync]
//   -> k_scatter_first -> [sync].  Host synchronisations: TWO for the sizing call, THREE for a full call
//   (plus what rocprim's segmented sort does internally, which does not depend on G either).
#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "asp_common.hpp"
#include "operator_internal.hpp"
#include "segment_kernels.hpp"
#include "sparsify_internal.hpp"

namespace {

using asp::DeviceBuffer;
using asp::unite;

// (kThreads, kWaves, grid_for, Events, segment_of and the flag-first / scatter-first kernels of the extension:
// segment_kernels.hpp, shared with cluster_grow.hip)

// The offset refusals shared by the two entry points; *total = offsets[num_segments].
int check_offsets(uint64_t num_segments, const uint64_t *offsets, uint64_t *total) {
  const uint64_t G = num_segments;
  if (G && !offsets) {
    return asp::set_error(ASP_ERR_INVALID, "null offsets with %llu segments", (unsigned long long)G);
  }
  if (G >= 0xFFFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 segments");
  if (G && offsets[0] != 0) return asp::set_error(ASP_ERR_INVALID, "offsets[0] is not 0");
  for (uint64_t g = 0; g < G; ++g) {
    if (offsets[g + 1] < offsets[g]) {
      return asp::set_error(ASP_ERR_INVALID, "offsets decrease at index %llu", (unsigned long long)(g + 1));
    }
  }
  *total = G ? offsets[G] : 0;
  if (*total >= 0xFFFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 table entries");
  return ASP_OK;
}

__global__ __launch_bounds__(kThreads) void k_row_segment(const uint64_t *__restrict__ offsets,
                                                         uint64_t num_segments, uint64_t total,
                                                         uint32_t *__restrict__ row_segment) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < total) row_segment[i] = segment_of(offsets, num_segments, i);
}

// ===========================================================================
// the cutoff of many clusters
// ===========================================================================

__device__ __forceinline__ unsigned long long double_bits_abs(double x) {
  return static_cast<unsigned long long>(__double_as_longlong(x)) & 0x7FFFFFFFFFFFFFFFull;
}

struct SegGraph {
  const int64_t *indptr;   // i64[T + 1], global
  const int32_t *indices;  // segment-local columns
  const double *data;
  const uint8_t *frozen;   // u8[T]
  const uint64_t *offsets;  // u64[G + 1]
  const uint32_t *row_segment;
  unsigned long long *max_bits;  // u64[G]
  uint32_t *parent;              // u32[T], global spin numbers
  uint64_t total;                // T
  double reltol;
};

// max |data| of every segment: the bit pattern of |x| orders like |x| for finite values.
__global__ __launch_bounds__(kThreads) void k_segment_abs_max(SegGraph a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= a.total) return;  // whole wavefront
  unsigned long long best = 0;
  for (int64_t k = a.indptr[row] + lane, end = a.indptr[row + 1]; k < end; k += 64) {
    const unsigned long long b = double_bits_abs(a.data[k]);
    best = b > best ? b : best;
  }
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) {
    const unsigned long long other = __shfl_xor(best, step, 64);
    best = other > best ? other : best;
  }
  if (lane == 0 && best != 0) atomicMax(&a.max_bits[a.row_segment[row]], best);
}

// The pruned element M'_ij (sparsify.hip's pruned() with the segment's threshold); i, j global.
__device__ __forceinline__ double pruned(const SegGraph &a, double threshold, uint32_t i, uint32_t j,
                                         double value) {
  if (a.frozen[i] && a.frozen[j]) return value;
  return fabs(value) < threshold ? 0.0 : value;
}

// M'_ji by binary search for the LOCAL column i - base in global row j (0 when there is no such element).
__device__ __forceinline__ double pruned_transposed(const SegGraph &a, double threshold, uint32_t base,
                                                    uint32_t i, uint32_t j) {
  const uint32_t needle = i - base;
  const int64_t end = a.indptr[j + 1];
  int64_t lo = a.indptr[j], hi = end;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (static_cast<uint32_t>(a.indices[mid]) < needle) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  if (lo < end && static_cast<uint32_t>(a.indices[lo]) == needle) return pruned(a, threshold, j, i, a.data[lo]);
  return 0.0;
}

__global__ __launch_bounds__(kThreads) void k_init_parent(uint32_t *parent, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n) parent[i] = static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(kThreads) void k_hook_edges_seg(SegGraph a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= a.total) return;
  const uint32_t i = static_cast<uint32_t>(row);
  const uint32_t g = a.row_segment[i];
  const uint32_t base = static_cast<uint32_t>(a.offsets[g]);
  // one rounded product, as numpy's `reltol * max_coupling`; reltol * 0 for a segment without non-zeros
  const double threshold = __dmul_rn(a.reltol, __longlong_as_double(static_cast<long long>(a.max_bits[g])));
  const int64_t begin = a.indptr[i], end = a.indptr[i + 1];
  for (int64_t k = begin + lane; k < end; k += 64) {
    const uint32_t j = base + static_cast<uint32_t>(a.indices[k]);
    if (j == i) continue;
    const double mine = pruned(a, threshold, i, j, a.data[k]);
    const double theirs = pruned_transposed(a, threshold, base, i, j);
    // scipy: entry of M' + M'^T kept iff the sum is non-zero, scaled by 0.5, zeros eliminated
    if (__dmul_rn(0.5, __dadd_rn(mine, theirs)) != 0.0) unite(a.parent, i, j);
  }
}

// Roots into a SEPARATE array with a read-only walk (see sparsify.hip's k_flatten).
__global__ __launch_bounds__(kThreads) void k_flatten(const uint32_t *__restrict__ parent,
                                                     uint32_t *__restrict__ root, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t x = static_cast<uint32_t>(i);
  for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
  root[i] = x;
}

// keep[i] = same component as the anchor of i's segment; stray[g] counts the frozen spins of segment g
// outside it, first_stray is the smallest such g.
__global__ __launch_bounds__(kThreads) void k_mark_segments(const uint32_t *__restrict__ root,
                                                           const uint8_t *__restrict__ frozen,
                                                           const uint64_t *__restrict__ offsets,
                                                           const uint64_t *__restrict__ anchors,
                                                           const uint32_t *__restrict__ row_segment,
                                                           uint64_t n, uint32_t *__restrict__ keep,
                                                           uint8_t *__restrict__ keep8,
                                                           uint32_t *__restrict__ stray,
                                                           uint32_t *__restrict__ first_stray) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = row_segment[i];
  const bool in = root[i] == root[offsets[g] + anchors[g]];
  keep[i] = in ? 1u : 0u;
  keep8[i] = in ? 1 : 0;
  if (frozen[i] && !in) {
    atomicAdd(&stray[g], 1u);
    atomicMin(first_stray, g);
  }
}

// kept_offsets[g] = new_index[offsets[g]] for g = 0 ... G; summary = {first stray segment, its count}.
__global__ __launch_bounds__(kThreads) void k_segment_sums(const uint64_t *__restrict__ offsets,
                                                          uint64_t num_segments,
                                                          const int64_t *__restrict__ new_index,
                                                          const uint32_t *__restrict__ stray,
                                                          const uint32_t *__restrict__ first_stray,
                                                          int64_t *__restrict__ kept_offsets,
                                                          uint32_t *__restrict__ summary) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g > num_segments) return;
  kept_offsets[g] = new_index[offsets[g]];
  if (g == 0) {
    const uint32_t first = *first_stray;
    summary[0] = first;
    summary[1] = first < num_segments ? stray[first] : 0u;
  }
}

struct SegSlice {
  const int64_t *indptr;
  const int32_t *indices;
  const double *data;
  const uint32_t *keep;
  const int64_t *new_index;  // exclusive scan of keep over the whole table
  const uint64_t *offsets;
  const uint32_t *row_segment;
  uint32_t *row_kept;         // per OLD row
  const int64_t *nnz_before;  // exclusive scan of row_kept
  int32_t *out_indices;
  double *out_data;
  uint64_t total;
};

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_slice_seg(SegSlice a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= a.total) return;  // whole wavefront
  if (!a.keep[row]) {
    if (!EMIT && lane == 0) a.row_kept[row] = 0;
    return;
  }
  const uint64_t base = a.offsets[a.row_segment[row]];
  const int64_t first_new = a.new_index[base];
  const int64_t begin = a.indptr[row], end = a.indptr[row + 1];
  int64_t out = EMIT ? a.nnz_before[row] : 0;
  uint32_t total = 0;
  for (int64_t at = begin; at < end; at += 64) {
    const int64_t k = at + lane;
    const bool live = k < end && a.keep[base + static_cast<uint32_t>(a.indices[k])];
    const uint64_t votes = __ballot(live);
    if (EMIT && live) {
      const int64_t to = out + __popcll(votes & ((1ull << lane) - 1ull));
      a.out_indices[to] = static_cast<int32_t>(a.new_index[base + static_cast<uint32_t>(a.indices[k])] - first_new);
      a.out_data[to] = a.data[k];
    }
    const uint32_t here = static_cast<uint32_t>(__popcll(votes));
    out += here;
    total += here;
  }
  if (!EMIT && lane == 0) a.row_kept[row] = total;
}

// out_indptr[new row] = non-zeros kept before it; the last entry is the total.
__global__ __launch_bounds__(kThreads) void k_compact_indptr(const uint32_t *__restrict__ keep,
                                                            const int64_t *__restrict__ new_index,
                                                            const int64_t *__restrict__ nnz_before,
                                                            uint64_t n, int64_t *__restrict__ out_indptr) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i > n) return;
  if (i == n || keep[i]) out_indptr[new_index[i]] = nnz_before[i];
}

// ===========================================================================
// the extension of many clusters
// ===========================================================================

// k_segment_starts -> sort -> k_flag_first_seg -> scan -> k_segment_counts -> k_scatter_first: segment_kernels.hpp

}  // namespace

extern "C" int asp_sparsify_component_segments(uint64_t num_segments, uint64_t const *offsets,
                                               int64_t const *indptr, int32_t const *indices,
                                               double const *data, uint8_t const *is_frozen, double reltol,
                                               uint64_t const *anchors, uint8_t *keep, uint64_t *kept_offsets,
                                               uint64_t capacity, int64_t *out_indptr, int32_t *out_indices,
                                               double *out_data, uint64_t *out_nnz) {
  asp_clear_error();
  // (every check before any device work and before any output is written)
  const uint64_t G = num_segments;
  if (!kept_offsets || !out_nnz) return asp::set_error(ASP_ERR_INVALID, "null count pointer");
  if (G && !anchors) {
    return asp::set_error(ASP_ERR_INVALID, "null anchors with %llu segments", (unsigned long long)G);
  }
  uint64_t T = 0;
  ASP_TRY(check_offsets(G, offsets, &T));
  if (T == 0) {  // no device needed
    *out_nnz = 0;
    for (uint64_t g = 0; g <= G; ++g) kept_offsets[g] = 0;
    if (out_indptr) out_indptr[0] = 0;
    return ASP_OK;
  }
  if (!indptr || !is_frozen || !keep) return asp::set_error(ASP_ERR_INVALID, "null input array");
  if (indptr[0] != 0) return asp::set_error(ASP_ERR_INVALID, "indptr[0] must be 0");
  for (uint64_t i = 0; i < T; ++i) {
    if (indptr[i + 1] < indptr[i]) return asp::set_error(ASP_ERR_INVALID, "indptr is not monotone");
  }
  const uint64_t nnz = static_cast<uint64_t>(indptr[T]);
  if (nnz && (!indices || !data)) return asp::set_error(ASP_ERR_INVALID, "null indices/data");
  for (uint64_t g = 0; g < G; ++g) {
    const uint64_t n = offsets[g + 1] - offsets[g];
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
      for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) {
        if (indices[k] < 0 || static_cast<uint64_t>(indices[k]) >= n) {
          return asp::set_error(ASP_ERR_INVALID, "column index out of range in row %llu of segment %llu",
                                (unsigned long long)(i - offsets[g]), (unsigned long long)g);
        }
        if (k > indptr[i] && indices[k - 1] >= indices[k]) {
          return asp::set_error(ASP_ERR_INVALID, "row %llu of segment %llu is not sorted and duplicate-free",
                                (unsigned long long)(i - offsets[g]), (unsigned long long)g);
        }
      }
    }
    if (n && anchors[g] >= n) {
      return asp::set_error(ASP_ERR_INVALID, "anchor spin of segment %llu out of range", (unsigned long long)g);
    }
  }
  ASP_TRY(asp::require_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  DeviceBuffer<uint64_t> d_offsets, d_anchors;
  DeviceBuffer<int64_t> d_indptr, d_new_index, d_kept_offsets, d_nnz_before, d_out_indptr, d_scratch;
  DeviceBuffer<int32_t> d_indices, d_out_indices;
  DeviceBuffer<double> d_data, d_out_data;
  DeviceBuffer<uint8_t> d_frozen, d_keep8;
  DeviceBuffer<uint32_t> d_row_segment, d_parent, d_root, d_keep, d_row_kept, d_stray, d_first, d_summary;
  DeviceBuffer<unsigned long long> d_max;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(d_offsets.alloc(G + 1));
  ASP_TRY(d_anchors.alloc(G));
  ASP_TRY(d_indptr.alloc(T + 1));
  ASP_TRY(d_indices.alloc(nnz));
  ASP_TRY(d_data.alloc(nnz));
  ASP_TRY(d_frozen.alloc(T));
  ASP_TRY(d_keep8.alloc(T));
  ASP_TRY(d_row_segment.alloc(T));
  ASP_TRY(d_parent.alloc(T));
  ASP_TRY(d_root.alloc(T));
  ASP_TRY(d_keep.alloc(T));
  ASP_TRY(d_row_kept.alloc(T));
  ASP_TRY(d_new_index.alloc(T + 1));
  ASP_TRY(d_nnz_before.alloc(T + 1));
  ASP_TRY(d_out_indptr.alloc(T + 1));
  ASP_TRY(d_kept_offsets.alloc(G + 1));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(T)));
  ASP_TRY(d_stray.alloc(G));
  ASP_TRY(d_first.alloc(1));
  ASP_TRY(d_summary.alloc(2));
  ASP_TRY(d_max.alloc(G));
  ASP_TRY(events.create());
  ASP_TRY(d_offsets.upload(offsets, G + 1, stream));
  ASP_TRY(d_anchors.upload(anchors, G, stream));
  ASP_TRY(d_indptr.upload(indptr, T + 1, stream));
  ASP_TRY(d_indices.upload(indices, nnz, stream));
  ASP_TRY(d_data.upload(data, nnz, stream));
  ASP_TRY(d_frozen.upload(is_frozen, T, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  ASP_HIP_TRY(hipMemsetAsync(d_max.ptr, 0, G * sizeof(unsigned long long), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_stray.ptr, 0, G * sizeof(uint32_t), stream));
  ASP_HIP_TRY(hipMemsetAsync(d_first.ptr, 0xFF, sizeof(uint32_t), stream));
  const dim3 block(kThreads);
  const dim3 per_item(grid_for(T, kThreads)), per_row(grid_for(T, kWaves)), per_segment(grid_for(G + 1, kThreads));
  hipLaunchKernelGGL(k_row_segment, per_item, block, 0, stream, d_offsets.ptr, G, T, d_row_segment.ptr);
  SegGraph graph{d_indptr.ptr, d_indices.ptr, d_data.ptr, d_frozen.ptr, d_offsets.ptr, d_row_segment.ptr,
                 d_max.ptr, d_parent.ptr, T, reltol};
  hipLaunchKernelGGL(k_segment_abs_max, per_row, block, 0, stream, graph);
  hipLaunchKernelGGL(k_init_parent, per_item, block, 0, stream, d_parent.ptr, T);
  hipLaunchKernelGGL(k_hook_edges_seg, per_row, block, 0, stream, graph);
  hipLaunchKernelGGL(k_flatten, per_item, block, 0, stream, d_parent.ptr, d_root.ptr, T);
  hipLaunchKernelGGL(k_mark_segments, per_item, block, 0, stream, d_root.ptr, d_frozen.ptr, d_offsets.ptr,
                     d_anchors.ptr, d_row_segment.ptr, T, d_keep.ptr, d_keep8.ptr, d_stray.ptr, d_first.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(asp::exclusive_scan_u32(d_keep.ptr, T, d_new_index.ptr, d_scratch.ptr, stream));
  hipLaunchKernelGGL(k_segment_sums, per_segment, block, 0, stream, d_offsets.ptr, G, d_new_index.ptr,
                     d_stray.ptr, d_first.ptr, d_kept_offsets.ptr, d_summary.ptr);
  // the kept block of the UN-pruned matrix (common.py:674): lengths of the kept rows, per OLD row
  SegSlice slice{d_indptr.ptr, d_indices.ptr, d_data.ptr, d_keep.ptr, d_new_index.ptr, d_offsets.ptr,
                 d_row_segment.ptr, d_row_kept.ptr, nullptr, nullptr, nullptr, T};
  hipLaunchKernelGGL(k_slice_seg<false>, per_row, block, 0, stream, slice);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(asp::exclusive_scan_u32(d_row_kept.ptr, T, d_nnz_before.ptr, d_scratch.ptr, stream));
  hipLaunchKernelGGL(k_compact_indptr, dim3(grid_for(T + 1, kThreads)), block, 0, stream, d_keep.ptr,
                     d_new_index.ptr, d_nnz_before.ptr, T, d_out_indptr.ptr);
  ASP_HIP_TRY(hipGetLastError());
  const bool mask_only = !out_indptr && !out_indices && !out_data && capacity == 0;
  if (mask_only) ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  // first synchronisation: the stray summary, every size and the mask
  uint32_t summary[2] = {0, 0};
  int64_t kept_nnz = 0;
  std::vector<int64_t> kept(G + 1);
  std::vector<uint8_t> mask(T);
  ASP_TRY(d_summary.download(summary, 2, stream));
  ASP_HIP_TRY(hipMemcpyAsync(&kept_nnz, d_nnz_before.ptr + T, sizeof kept_nnz, hipMemcpyDeviceToHost, stream));
  ASP_TRY(d_kept_offsets.download(kept.data(), G + 1, stream));
  ASP_TRY(d_keep8.download(mask.data(), T, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  if (summary[0] != 0xFFFFFFFFu) {
    // the reference asserts this (common.py:666)
    return asp::set_error(ASP_ERR_INVALID,
                          "segment %u: %u frozen spins are not connected to the anchor after the cutoff",
                          summary[0], summary[1]);
  }
  std::memcpy(keep, mask.data(), T);
  for (uint64_t g = 0; g <= G; ++g) kept_offsets[g] = static_cast<uint64_t>(kept[g]);
  *out_nnz = static_cast<uint64_t>(kept_nnz);
  if (mask_only) {
    asp::set_sparsify_last_ms(events.elapsed());
    return ASP_OK;
  }
  if (!out_indptr || !out_indices || !out_data || *out_nnz > capacity) {
    return asp::set_error(ASP_ERR_INVALID, "%llu kept couplings do not fit capacity %llu",
                          (unsigned long long)*out_nnz, (unsigned long long)capacity);
  }
  ASP_TRY(d_out_indices.alloc(*out_nnz));
  ASP_TRY(d_out_data.alloc(*out_nnz));
  slice.nnz_before = d_nnz_before.ptr;
  slice.out_indices = d_out_indices.ptr;
  slice.out_data = d_out_data.ptr;
  hipLaunchKernelGGL(k_slice_seg<true>, per_row, block, 0, stream, slice);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  ASP_TRY(d_out_indptr.download(out_indptr, static_cast<uint64_t>(kept[G]) + 1, stream));
  ASP_TRY(d_out_indices.download(out_indices, *out_nnz, stream));
  ASP_TRY(d_out_data.download(out_data, *out_nnz, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));  // second synchronisation
  asp::set_sparsify_last_ms(events.elapsed());
  return ASP_OK;
}

extern "C" int asp_operator_extend_segments(asp_operator const *op, uint64_t num_segments,
                                            uint64_t const *offsets, uint64_t const *keys, uint64_t capacity,
                                            uint64_t *out, uint64_t *out_offsets, uint64_t *count) {
  asp_clear_error();
  // (every check before any launch and before any output is written)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  if (!count || !out_offsets) return asp::set_error(ASP_ERR_INVALID, "null count pointer");
  const uint64_t G = num_segments;
  uint64_t T = 0;
  ASP_TRY(check_offsets(G, offsets, &T));
  if (T == 0) {  // no device needed
    *count = 0;
    for (uint64_t g = 0; g <= G; ++g) out_offsets[g] = 0;
    return ASP_OK;
  }
  if (!keys) return asp::set_error(ASP_ERR_INVALID, "null keys with %llu table entries", (unsigned long long)T);
  // the sort looks at the bits [0, number_spins) only (asp_operator_extend)
  if (op->number_spins < 64) {
    for (uint64_t g = 0; g < G; ++g) {
      for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
        if (keys[i] >> op->number_spins) {
          return asp::set_error(ASP_ERR_INVALID, "key %llu of segment %llu has a bit at or above site %u",
                                (unsigned long long)(i - offsets[g]), (unsigned long long)g, op->number_spins);
        }
      }
    }
  }
  if (T > 0xFFFFFFFFull / std::max<uint32_t>(op->max_connections, 1u)) {
    // (an upper bound, so that it is known before any launch: every key has at most max_connections)
    return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 connections");
  }
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  Events events;
  asp::ConnectionList list;
  asp::Symmetrised sym;
  DeviceBuffer<uint64_t> d_offsets, d_sorted, d_unique;
  DeviceBuffer<uint32_t> d_flag, d_segment_start;
  DeviceBuffer<int64_t> d_pos, d_out_offsets, d_scratch;
  DeviceBuffer<uint8_t> d_temp;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(events.create());
  ASP_TRY(d_offsets.alloc(G + 1));
  ASP_TRY(d_offsets.upload(offsets, G + 1, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  // first synchronisation inside: the number of connections
  ASP_TRY(asp::extension_list_queue(op, T, keys, &list, &sym, stream));
  const uint64_t N = list.batch.total;
  if (N >= (1ull << 32)) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 connections");
  ASP_TRY(d_sorted.alloc(N));
  ASP_TRY(d_flag.alloc(N));
  ASP_TRY(d_pos.alloc(N + 1));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(N)));
  ASP_TRY(d_segment_start.alloc(G + 1));
  ASP_TRY(d_out_offsets.alloc(G + 1));
  const dim3 block(kThreads);
  const dim3 per_segment(grid_for(G + 1, kThreads)), per_connection(grid_for(N, kThreads));
  ASP_HIP_TRY(hipMemsetAsync(d_flag.ptr, 0, (N ? N : 1) * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_segment_starts, per_segment, block, 0, stream, d_offsets.ptr, G,
                     list.batch.d_offsets.ptr, N, d_segment_start.ptr, d_flag.ptr);
  ASP_HIP_TRY(hipGetLastError());
  const asp::SymmetryArgs symmetry = op->symmetry();
  const bool dropping = op->num_permutations != 0 && op->inversion < 0;
  if (N > 0) {
    size_t temp_bytes = 0;
    ASP_HIP_TRY(rocprim::segmented_radix_sort_keys(
        nullptr, temp_bytes, list.d_other.ptr, d_sorted.ptr, static_cast<unsigned>(N), static_cast<unsigned>(G),
        d_segment_start.ptr, d_segment_start.ptr + 1, 0, op->number_spins, stream));
    ASP_TRY(d_temp.alloc(temp_bytes ? temp_bytes : 1));
    ASP_HIP_TRY(rocprim::segmented_radix_sort_keys(
        d_temp.ptr, temp_bytes, list.d_other.ptr, d_sorted.ptr, static_cast<unsigned>(N), static_cast<unsigned>(G),
        d_segment_start.ptr, d_segment_start.ptr + 1, 0, op->number_spins, stream));
    hipLaunchKernelGGL(k_flag_first_seg, per_connection, block, 0, stream, d_sorted.ptr, N, dropping,
                       symmetry.mask, d_flag.ptr);
    ASP_HIP_TRY(hipGetLastError());
  }
  ASP_TRY(asp::exclusive_scan_u32(d_flag.ptr, N, d_pos.ptr, d_scratch.ptr, stream));
  hipLaunchKernelGGL(k_segment_counts, per_segment, block, 0, stream, d_segment_start.ptr, G, d_pos.ptr,
                     d_out_offsets.ptr);
  ASP_HIP_TRY(hipGetLastError());
  const bool sizing = capacity == 0 && !out;
  if (sizing) ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  std::vector<int64_t> counts(G + 1);
  ASP_TRY(d_out_offsets.download(counts.data(), G + 1, stream));
  ASP_TRY(sym.fetch(stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));  // second synchronisation
  ASP_TRY(sym.check());
  for (uint64_t g = 0; g <= G; ++g) out_offsets[g] = static_cast<uint64_t>(counts[g]);
  *count = static_cast<uint64_t>(counts[G]);
  if (sizing) {
    asp::set_operator_last_ms(events.elapsed());
    return ASP_OK;
  }
  if (*count > capacity || !out) {
    return asp::set_error(ASP_ERR_INVALID, "%llu states do not fit capacity %llu", (unsigned long long)*count,
                          (unsigned long long)capacity);
  }
  ASP_TRY(d_unique.alloc(*count));
  if (N > 0) {
    hipLaunchKernelGGL(k_scatter_first, per_connection, block, 0, stream, d_sorted.ptr, N, d_flag.ptr, d_pos.ptr,
                       d_unique.ptr);
    ASP_HIP_TRY(hipGetLastError());
  }
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  ASP_TRY(d_unique.download(out, *count, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));  // third synchronisation
  asp::set_operator_last_ms(events.elapsed());
  return ASP_OK;
}
