// The growth of a round of sampled clusters in one segmented device call, on gfx950:
// asp_operator_grow_segments, specification ASP-GROW-1.  Segment g grows a cluster of at most
// sizes[g] states around seeds[g] by breadth-first passes: the frontier is visited in ascending order, and every
// target that is not a member yet is kept with ONE Philox4x32-10 draw, counter (i, k, t, ids[g]) = (position of
// the source in the frontier, position of the target in the source's row, pass, stream id).  A segment's result
// depends on (operator, seed, size, id, keep probability, rng seed) only.
//
// HBM layout, resident between the passes:
//   members u64[2][sum sizes]: segment g's sorted members in ITS slot [slot[g], slot[g] + count[g]) of the table
//     which[g] (a pass merges into the other table, a finished segment keeps the one it has); slot u64[G + 1] are
//     the prefix sums of sizes, so a slot never overflows: |M| <= sizes[g] is the law.
//   per segment u32: count, which, passes; and of the pass that is prepared: applied (sources that are applied: a
//     prefix of the frontier), limit (frontier states that are added: a prefix), ends, added.
//   frontier u64[2][F] with offsets i64[G + 1] (ascending and duplicate-free per segment; empty for a finished
//     segment: that IS "not live"), grows u32[F], grows_before u32[F] (exclusive count within the segment).
//   keys u64[K] = the applied sources of all segments, key_segment u32[K], key offsets i64[G + 1].
// One pass t, for ALL segments, K and F known from the pass before:
//   action on the resident keys (asp::extension_list_queue_device: k_apply<count> -> scan -> [sync: N] ->
//   k_apply<emit> -> symmetrise) -> k_grow_draw (one thread per connection) -> scan -> k_grow_compact ->
//   k_grow_kept_starts -> rocprim::segmented_radix_sort_keys on the bits [0, number_spins) -> k_flag_first_seg ->
//   k_grow_clip -> scan -> k_segment_counts -> k_scatter_first (= frontier t + 1) -> k_grow_merge (members of
//   pass t into the other table) -> k_grow_stop for pass t + 1 (one workgroup per segment) -> scan -> k_grow_keys
//   -> [sync: F and K of pass t + 1, sources outside the sector].
// Launches per pass: ten kernels and a fill, plus the three scans', the sort's and the action's, whatever G is.
// Host synchronisations: TWO per pass, plus two at the end (sizes, then states).
#include <algorithm>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "asp_common.hpp"
#include "operator_internal.hpp"
#include "sa_device.hpp"
#include "segment_kernels.hpp"

namespace {

using asp::DeviceBuffer;

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct GrowTables {
  const uint64_t *sizes;  // u64[G]
  const uint64_t *slot;   // u64[G + 1]
  uint64_t *members[2];
  uint32_t *count, *which, *passes;
  uint32_t *applied, *limit, *ends, *added;
};

// First position in the ascending a[0 .. n) whose value is not below x.
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *__restrict__ a, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

__device__ __forceinline__ bool contains(const uint64_t *__restrict__ a, uint32_t n, uint64_t x) {
  const uint32_t at = lower_bound(a, n, x);
  return at < n && a[at] == x;
}

// Before pass 0: M = {seed}, F_0 = [seed].
__global__ __launch_bounds__(kThreads) void k_grow_init(GrowTables s, const uint64_t *__restrict__ seeds,
                                                       uint64_t num_segments, uint64_t *__restrict__ frontier,
                                                       int64_t *__restrict__ frontier_offsets) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g > num_segments) return;
  frontier_offsets[g] = static_cast<int64_t>(g);
  if (g == num_segments) return;
  s.members[0][s.slot[g]] = seeds[g];
  s.count[g] = 1u;
  s.which[g] = 0u;
  s.passes[g] = 0u;
  frontier[g] = seeds[g];
}

// One workgroup per segment, step 1 of the law for the pass that is prepared: grows[i] = frontier state i is no
// member yet; stop = the first i at which |M| + (grows up to and including i) reaches the size.  A running block
// scan over tiles of kThreads frontier states (a frontier is longer than a workgroup); tiles behind stop are not
// looked at, and nobody reads their grows[].
__global__ __launch_bounds__(kThreads) void k_grow_stop(GrowTables s, const uint64_t *__restrict__ frontier,
                                                       const int64_t *__restrict__ frontier_offsets,
                                                       uint32_t *__restrict__ grows,
                                                       uint32_t *__restrict__ grows_before, uint32_t pass) {
  __shared__ uint32_t wave_total[kWaves];
  __shared__ uint32_t first_hit;
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int64_t begin = frontier_offsets[g];
  const uint32_t nf = static_cast<uint32_t>(frontier_offsets[g + 1] - begin);
  if (nf == 0) {  // finished (or never reached): nothing applied, nothing added
    if (tid == 0) s.applied[g] = s.limit[g] = s.ends[g] = s.added[g] = 0u;
    return;
  }
  const uint64_t *F = frontier + begin;
  const uint64_t *M = s.members[s.which[g]] + s.slot[g];
  const uint32_t mc = s.count[g];
  const uint64_t size = s.sizes[g];
  if (tid == 0) first_hit = kNone;
  __syncthreads();
  uint32_t running = 0, stop = kNone;
  for (uint32_t base = 0; base < nf; base += kThreads) {
    const uint32_t i = base + tid;
    const bool in = i < nf;
    const bool grow = in && !contains(M, mc, F[i]);
    const uint64_t votes = __ballot(grow);
    const uint32_t below = static_cast<uint32_t>(__popcll(votes & ((1ull << lane) - 1ull)));
    if (lane == 0) wave_total[wave] = static_cast<uint32_t>(__popcll(votes));
    __syncthreads();
    uint32_t wave_before = 0, tile_total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t v = wave_total[w];
      wave_before += static_cast<uint32_t>(w) < wave ? v : 0u;
      tile_total += v;
    }
    const uint32_t before = running + wave_before + below;
    if (in) {
      grows[begin + i] = grow ? 1u : 0u;
      grows_before[begin + i] = before;
      if (static_cast<uint64_t>(mc) + before + (grow ? 1u : 0u) >= size) atomicMin(&first_hit, i);
    }
    __syncthreads();
    stop = first_hit;  // the same for every thread
    if (stop != kNone) {
      if (i == stop) s.added[g] = before + (grow ? 1u : 0u);
      break;
    }
    running += tile_total;
  }
  if (tid == 0) {
    if (stop != kNone) {
      s.applied[g] = pass == 0 ? 1u : stop;  // (pass 0: the seed is applied whatever the size, so that a seed
      s.limit[g] = stop + 1u;                //  outside the sector is always noticed; its draws have no effect)
      s.ends[g] = 1u;
    } else {
      s.applied[g] = nf;
      s.limit[g] = nf;
      s.ends[g] = 0u;
      s.added[g] = running;
    }
  }
}

// keys[j] = the j-th applied source of the call: segment g's frontier states [0, applied[g]).
__global__ __launch_bounds__(kThreads) void k_grow_keys(const int64_t *__restrict__ key_offsets,
                                                       uint64_t num_segments, const uint64_t *__restrict__ frontier,
                                                       const int64_t *__restrict__ frontier_offsets,
                                                       uint64_t capacity, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ key_segment) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t total = static_cast<uint64_t>(key_offsets[num_segments]);
  if (j >= total || j >= capacity) return;
  const uint32_t g = segment_of(reinterpret_cast<const uint64_t *>(key_offsets), num_segments, j);
  keys[j] = frontier[frontier_offsets[g] + static_cast<int64_t>(j - static_cast<uint64_t>(key_offsets[g]))];
  key_segment[j] = g;
}

struct DrawArgs {
  GrowTables s;
  const uint32_t *ids;
  const uint64_t *frontier;
  const int64_t *frontier_offsets;
  const int64_t *key_offsets;         // i64[G + 1]
  const uint32_t *key_segment;        // u32[K]
  const int64_t *connection_offsets;  // i64[K + 1]
  const uint64_t *targets;            // u64[N]
  uint64_t keys, connections;
  uint64_t threshold;  // floor(p * 2^32)
  uint32_t pass, seed_lo, seed_hi;
  bool dropping;
  uint64_t drop;  // the "no state" value of the extension mode
  uint32_t *keep;
};

// Step 2 of the law, one thread per connection.
__global__ __launch_bounds__(kThreads) void k_grow_draw(DrawArgs a) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= a.connections) return;
  const uint32_t row = segment_of(reinterpret_cast<const uint64_t *>(a.connection_offsets), a.keys, c);
  const uint32_t g = a.key_segment[row];
  const uint32_t i = row - static_cast<uint32_t>(a.key_offsets[g]);
  const uint32_t k = static_cast<uint32_t>(c - static_cast<uint64_t>(a.connection_offsets[row]));
  const uint64_t x = a.targets[c];
  uint32_t keep = 0;
  if (!a.s.ends[g] && !(a.dropping && x == a.drop)) {  // (what a segment draws in its last pass has no effect)
    const uint64_t *M = a.s.members[a.s.which[g]] + a.s.slot[g];
    bool member = contains(M, a.s.count[g], x);
    if (!member) {
      const int64_t begin = a.frontier_offsets[g];
      const uint32_t nf = static_cast<uint32_t>(a.frontier_offsets[g + 1] - begin);
      const uint32_t at = lower_bound(a.frontier + begin, nf, x);
      member = at < nf && a.frontier[begin + at] == x && at <= i;
    }
    if (!member) {
      const asp::dev::Philox4 r = asp::dev::philox4x32_10(i, k, a.pass, a.ids[g], a.seed_lo, a.seed_hi);
      keep = static_cast<uint64_t>(r.w[0]) < a.threshold ? 1u : 0u;
    }
  }
  a.keep[c] = keep;
}

__global__ __launch_bounds__(kThreads) void k_grow_compact(const uint64_t *__restrict__ targets, uint64_t n,
                                                          const uint32_t *__restrict__ keep,
                                                          const int64_t *__restrict__ position,
                                                          uint64_t *__restrict__ kept) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (c < n && keep[c]) kept[position[c]] = targets[c];
}

// kept_start[g] = position of segment g's first kept target among all kept ones (g = 0 ... G: the last one is
// their number), and a 1 in flag[] there (flag[] was cleared).
__global__ __launch_bounds__(kThreads) void k_grow_kept_starts(const int64_t *__restrict__ key_offsets,
                                                              uint64_t num_segments,
                                                              const int64_t *__restrict__ connection_offsets,
                                                              const int64_t *__restrict__ position,
                                                              uint64_t connections,
                                                              uint32_t *__restrict__ kept_start,
                                                              uint32_t *__restrict__ flag) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g > num_segments) return;
  const int64_t start = position[connection_offsets[key_offsets[g]]];
  kept_start[g] = static_cast<uint32_t>(start);
  if (g < num_segments && start < position[connections]) flag[start] = 1u;
}

// The flags behind the last kept target belong to nothing (the sort's output is longer than what it sorted).
__global__ __launch_bounds__(kThreads) void k_grow_clip(const int64_t *__restrict__ position, uint64_t n,
                                                       uint32_t *__restrict__ flag) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n && static_cast<int64_t>(i) >= position[n]) flag[i] = 0u;
}

// One workgroup per segment: members of the pass = members before it, merged with the frontier states
// [0, limit) that grow, into the OTHER table.  Both lists ascend and share no state, so every state finds its
// place by one binary search in the other list.
__global__ __launch_bounds__(kThreads) void k_grow_merge(GrowTables s, const uint64_t *__restrict__ frontier,
                                                        const int64_t *__restrict__ frontier_offsets,
                                                        const uint32_t *__restrict__ grows,
                                                        const uint32_t *__restrict__ grows_before) {
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const int64_t begin = frontier_offsets[g];
  const uint32_t nf = static_cast<uint32_t>(frontier_offsets[g + 1] - begin);
  if (nf == 0) return;
  const uint32_t from = s.which[g], mc = s.count[g], limit = s.limit[g], added = s.added[g];
  const uint64_t room = s.sizes[g];
  const uint64_t *F = frontier + begin;
  const uint64_t *M = s.members[from] + s.slot[g];
  uint64_t *out = s.members[from ^ 1u] + s.slot[g];
  for (uint32_t j = tid; j < mc; j += kThreads) {
    const uint64_t x = M[j];
    const uint32_t at = lower_bound(F, limit, x);
    const uint64_t to = static_cast<uint64_t>(j) + (at < limit ? grows_before[begin + at] : added);
    if (to < room) out[to] = x;
  }
  for (uint32_t i = tid; i < limit; i += kThreads) {
    if (!grows[begin + i]) continue;
    const uint64_t x = F[i];
    const uint64_t to = static_cast<uint64_t>(grows_before[begin + i]) + lower_bound(M, mc, x);
    if (to < room) out[to] = x;
  }
  __syncthreads();  // (every thread has read which / count)
  if (tid == 0) {
    s.count[g] = mc + added;
    s.which[g] = from ^ 1u;
    s.passes[g] += 1u;
  }
}

__global__ __launch_bounds__(kThreads) void k_grow_emit(GrowTables s, const int64_t *__restrict__ out_offsets,
                                                       uint64_t *__restrict__ out) {
  const uint32_t g = blockIdx.x;
  const uint64_t *M = s.members[s.which[g]] + s.slot[g];
  uint64_t *to = out + out_offsets[g];
  for (uint32_t j = threadIdx.x, n = s.count[g]; j < n; j += kThreads) to[j] = M[j];
}

}  // namespace

extern "C" int asp_operator_grow_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *seeds,
                                          uint64_t const *sizes, uint32_t const *ids, double keep_probability,
                                          uint64_t rng_seed, uint64_t capacity, uint64_t *out,
                                          uint64_t *out_offsets, uint64_t *count, uint32_t *passes) {
  asp_clear_error();
  // (every check before any launch and before any output is written)
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  if (!count || !out_offsets) return asp::set_error(ASP_ERR_INVALID, "null count pointer");
  const uint64_t G = num_segments;
  if (G && (!seeds || !sizes || !ids)) {
    return asp::set_error(ASP_ERR_INVALID, "null seeds, sizes or ids with %llu segments", (unsigned long long)G);
  }
  if (!(keep_probability >= 0.0 && keep_probability <= 1.0)) {
    return asp::set_error(ASP_ERR_INVALID, "keep probability %g is not in [0, 1]", keep_probability);
  }
  if (G >= 0xFFFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 segments");
  std::vector<uint64_t> slot(G + 1, 0);
  for (uint64_t g = 0; g < G; ++g) {
    if (sizes[g] == 0) return asp::set_error(ASP_ERR_INVALID, "size of segment %llu is 0", (unsigned long long)g);
    if (sizes[g] >= 0xFFFFFFFFull || slot[g] + sizes[g] >= 0xFFFFFFFFull) {
      return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32-2 states");
    }
    slot[g + 1] = slot[g] + sizes[g];
  }
  const uint64_t total = slot[G];
  if (capacity < total) {
    return asp::set_error(ASP_ERR_INVALID, "capacity %llu is below the sum of the sizes, %llu",
                          (unsigned long long)capacity, (unsigned long long)total);
  }
  if (G && !out) return asp::set_error(ASP_ERR_INVALID, "null output with %llu segments", (unsigned long long)G);
  if (G == 0) {  // no device needed
    *count = 0;
    out_offsets[0] = 0;
    return ASP_OK;
  }
  if (op->number_spins < 64) {  // the sort looks at the bits [0, number_spins) only
    for (uint64_t g = 0; g < G; ++g) {
      if (seeds[g] >> op->number_spins) {
        return asp::set_error(ASP_ERR_INVALID, "seed of segment %llu has a bit at or above site %u",
                              (unsigned long long)g, op->number_spins);
      }
    }
  }
  const uint64_t threshold = static_cast<uint64_t>(keep_probability * 4294967296.0);  // exact product, floor
  const uint64_t per_key = std::max<uint32_t>(op->max_connections, 1u);
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  Events events;
  asp::ConnectionList list;
  asp::Symmetrised sym;
  DeviceBuffer<uint64_t> d_seeds, d_sizes, d_slot, d_members[2], d_frontier[2], d_kept, d_sorted, d_out;
  DeviceBuffer<uint32_t> d_ids, d_state, d_grows[2], d_before[2], d_key_segment, d_keep, d_flag, d_kept_start;
  DeviceBuffer<int64_t> d_frontier_offsets[2], d_key_offsets, d_position, d_unique_position, d_out_offsets;
  DeviceBuffer<int64_t> d_scratch;
  DeviceBuffer<uint8_t> d_temp;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers go
  ASP_TRY(events.create());
  ASP_TRY(d_seeds.alloc(G));
  ASP_TRY(d_sizes.alloc(G));
  ASP_TRY(d_ids.alloc(G));
  ASP_TRY(d_slot.alloc(G + 1));
  ASP_TRY(d_members[0].alloc(total));
  ASP_TRY(d_members[1].alloc(total));
  ASP_TRY(d_state.alloc(7 * G));
  ASP_TRY(d_frontier[0].alloc(G));
  ASP_TRY(d_grows[0].alloc(G));
  ASP_TRY(d_before[0].alloc(G));
  ASP_TRY(d_frontier_offsets[0].alloc(G + 1));
  ASP_TRY(d_frontier_offsets[1].alloc(G + 1));
  ASP_TRY(d_key_offsets.alloc(G + 1));
  ASP_TRY(d_kept_start.alloc(G + 1));
  ASP_TRY(d_out_offsets.alloc(G + 1));
  // (a segment applies fewer than sizes[g] sources in a pass: each one grew the cluster or was a member)
  ASP_TRY(list.batch.d_keys.alloc(total));
  ASP_TRY(d_key_segment.alloc(total));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(G)));
  ASP_TRY(d_seeds.upload(seeds, G, stream));
  ASP_TRY(d_sizes.upload(sizes, G, stream));
  ASP_TRY(d_ids.upload(ids, G, stream));
  ASP_TRY(d_slot.upload(slot.data(), G + 1, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev0, stream));
  GrowTables tables{d_sizes.ptr, d_slot.ptr, {d_members[0].ptr, d_members[1].ptr},
                    d_state.ptr, d_state.ptr + G, d_state.ptr + 2 * G, d_state.ptr + 3 * G,
                    d_state.ptr + 4 * G, d_state.ptr + 5 * G, d_state.ptr + 6 * G};
  const dim3 block(kThreads);
  const dim3 per_segment(grid_for(G + 1, kThreads)), segment_blocks(static_cast<unsigned>(G));
  const asp::SymmetryArgs symmetry = op->symmetry();
  const bool dropping = op->num_permutations != 0 && op->inversion < 0;
  hipLaunchKernelGGL(k_grow_init, per_segment, block, 0, stream, tables, d_seeds.ptr, G, d_frontier[0].ptr,
                     d_frontier_offsets[0].ptr);
  ASP_HIP_TRY(hipGetLastError());

  // Step 1 of pass `pass` on frontier table `b` and the applied sources as the action's resident keys;
  // `bound` >= the number of frontier states.
  auto prepare = [&](int b, uint32_t pass, uint64_t bound) -> int {
    hipLaunchKernelGGL(k_grow_stop, segment_blocks, block, 0, stream, tables, d_frontier[b].ptr,
                       d_frontier_offsets[b].ptr, d_grows[b].ptr, d_before[b].ptr, pass);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(asp::exclusive_scan_u32(tables.applied, G, d_key_offsets.ptr, d_scratch.ptr, stream));
    const uint64_t threads = std::min(bound, total);
    if (threads > 0) {
      hipLaunchKernelGGL(k_grow_keys, dim3(grid_for(threads, kThreads)), block, 0, stream, d_key_offsets.ptr, G,
                         d_frontier[b].ptr, d_frontier_offsets[b].ptr, total, list.batch.d_keys.ptr,
                         d_key_segment.ptr);
      ASP_HIP_TRY(hipGetLastError());
    }
    return ASP_OK;
  };

  int cur = 0;
  uint32_t pass = 0;
  uint64_t K = G;  // pass 0 applies every seed
  ASP_TRY(prepare(cur, pass, G));
  for (;;) {
    // (an upper bound, so that it is known before the pass's launches: every key has at most max_connections)
    if (K > 0xFFFFFFFFull / per_key) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 connections in a pass");
    uint64_t N = 0;
    if (K > 0) {
      // first synchronisation of the pass inside: the number of connections
      ASP_TRY(asp::extension_list_queue_device(op, K, &list, &sym, stream));
      N = list.batch.total;
      if (N >= (1ull << 32)) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 connections in a pass");
    }
    const int next = cur ^ 1;
    if (N > 0) {
      // (what these replace was last used before the previous pass's second synchronisation)
      ASP_TRY(d_keep.ensure(N));
      ASP_TRY(d_flag.ensure(N));
      ASP_TRY(d_position.ensure(N + 1));
      ASP_TRY(d_unique_position.ensure(N + 1));
      ASP_TRY(d_kept.ensure(N));
      ASP_TRY(d_sorted.ensure(N));
      ASP_TRY(d_frontier[next].ensure(N));
      ASP_TRY(d_grows[next].ensure(N));
      ASP_TRY(d_before[next].ensure(N));
      ASP_TRY(d_scratch.ensure(asp::scan_scratch_elems(std::max(N, G))));
      size_t temp_bytes = 0;
      ASP_HIP_TRY(rocprim::segmented_radix_sort_keys(
          nullptr, temp_bytes, d_kept.ptr, d_sorted.ptr, static_cast<unsigned>(N), static_cast<unsigned>(G),
          d_kept_start.ptr, d_kept_start.ptr + 1, 0, op->number_spins, stream));
      ASP_TRY(d_temp.ensure(temp_bytes ? temp_bytes : 1));
      const dim3 per_connection(grid_for(N, kThreads));
      DrawArgs draw{tables, d_ids.ptr, d_frontier[cur].ptr, d_frontier_offsets[cur].ptr, d_key_offsets.ptr,
                    d_key_segment.ptr, list.batch.d_offsets.ptr, list.d_other.ptr, K, N, threshold, pass,
                    static_cast<uint32_t>(rng_seed), static_cast<uint32_t>(rng_seed >> 32), dropping,
                    symmetry.mask, d_keep.ptr};
      hipLaunchKernelGGL(k_grow_draw, per_connection, block, 0, stream, draw);
      ASP_HIP_TRY(hipGetLastError());
      ASP_TRY(asp::exclusive_scan_u32(d_keep.ptr, N, d_position.ptr, d_scratch.ptr, stream));
      ASP_HIP_TRY(hipMemsetAsync(d_flag.ptr, 0, N * sizeof(uint32_t), stream));
      hipLaunchKernelGGL(k_grow_compact, per_connection, block, 0, stream, list.d_other.ptr, N, d_keep.ptr,
                         d_position.ptr, d_kept.ptr);
      hipLaunchKernelGGL(k_grow_kept_starts, per_segment, block, 0, stream, d_key_offsets.ptr, G,
                         list.batch.d_offsets.ptr, d_position.ptr, N, d_kept_start.ptr, d_flag.ptr);
      ASP_HIP_TRY(hipGetLastError());
      // (the sort's `size` only sizes its temporary keys: the segments end at the last kept target)
      ASP_HIP_TRY(rocprim::segmented_radix_sort_keys(
          d_temp.ptr, temp_bytes, d_kept.ptr, d_sorted.ptr, static_cast<unsigned>(N), static_cast<unsigned>(G),
          d_kept_start.ptr, d_kept_start.ptr + 1, 0, op->number_spins, stream));
      hipLaunchKernelGGL(k_flag_first_seg, per_connection, block, 0, stream, d_sorted.ptr, N, false, 0ull,
                         d_flag.ptr);
      hipLaunchKernelGGL(k_grow_clip, per_connection, block, 0, stream, d_position.ptr, N, d_flag.ptr);
      ASP_HIP_TRY(hipGetLastError());
      ASP_TRY(asp::exclusive_scan_u32(d_flag.ptr, N, d_unique_position.ptr, d_scratch.ptr, stream));
      hipLaunchKernelGGL(k_segment_counts, per_segment, block, 0, stream, d_kept_start.ptr, G,
                         d_unique_position.ptr, d_frontier_offsets[next].ptr);
      hipLaunchKernelGGL(k_scatter_first, per_connection, block, 0, stream, d_sorted.ptr, N, d_flag.ptr,
                         d_unique_position.ptr, d_frontier[next].ptr);
      ASP_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_grow_merge, segment_blocks, block, 0, stream, tables, d_frontier[cur].ptr,
                       d_frontier_offsets[cur].ptr, d_grows[cur].ptr, d_before[cur].ptr);
    ASP_HIP_TRY(hipGetLastError());
    if (N == 0) break;  // nothing was applied: no next frontier
    ASP_TRY(prepare(next, pass + 1, N));
    int64_t frontier_total = 0, keys_total = 0;
    ASP_HIP_TRY(hipMemcpyAsync(&frontier_total, d_frontier_offsets[next].ptr + G, sizeof frontier_total,
                               hipMemcpyDeviceToHost, stream));
    ASP_HIP_TRY(hipMemcpyAsync(&keys_total, d_key_offsets.ptr + G, sizeof keys_total, hipMemcpyDeviceToHost,
                               stream));
    ASP_TRY(sym.fetch(stream));
    ASP_HIP_TRY(hipStreamSynchronize(stream));  // second synchronisation of the pass
    ASP_TRY(sym.check());
    if (frontier_total == 0) break;  // no segment is live
    if (pass == 0xFFFFFFFFu) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 passes");
    cur = next;
    ++pass;
    K = static_cast<uint64_t>(keys_total);
  }
  ASP_TRY(asp::exclusive_scan_u32(tables.count, G, d_out_offsets.ptr, d_scratch.ptr, stream));
  std::vector<int64_t> offsets(G + 1);
  std::vector<uint32_t> ran(G);
  ASP_TRY(d_out_offsets.download(offsets.data(), G + 1, stream));
  ASP_HIP_TRY(hipMemcpyAsync(ran.data(), tables.passes, G * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  const uint64_t states = static_cast<uint64_t>(offsets[G]);
  if (states > capacity) {  // (cannot happen: |M| <= sizes[g])
    return asp::set_error(ASP_ERR_INVALID, "%llu states do not fit capacity %llu", (unsigned long long)states,
                          (unsigned long long)capacity);
  }
  ASP_TRY(d_out.alloc(states));
  hipLaunchKernelGGL(k_grow_emit, segment_blocks, block, 0, stream, tables, d_out_offsets.ptr, d_out.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev1, stream));
  ASP_TRY(d_out.download(out, states, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  for (uint64_t g = 0; g <= G; ++g) out_offsets[g] = static_cast<uint64_t>(offsets[g]);
  *count = states;
  if (passes) std::copy(ran.begin(), ran.end(), passes);
  asp::set_operator_last_ms(events.elapsed());
  return ASP_OK;
}
