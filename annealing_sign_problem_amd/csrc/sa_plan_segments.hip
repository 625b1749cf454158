// The sweep plans of a whole round in one call (asp_sa_plan_create_segments; law ASP-PLAN-SEG-1,
// DESIGN.md §4.15) and the read-back of a plan's device arrays (asp_sa_plan_read_array).  gfx950 only.
//
// A plan is made in three steps.  FRONT, on the device, for all segments at once: every stored entry is
// validated, finds its mirror and forms v = J_ij + J_ji; the rows keep the entries with v != 0.0 in column
// order (A = offdiag(J + J^T) in CSR), with the stored diagonal, sum_k |A_ik| added left to right and
// the smallest non-zero 2 |A_ik| per row.  HOST, per segment on a small pool of threads: DSATUR, the
// permutation, the blocks and the host copy of the ELL (sa_layout_back), the scales folded in row order
// from the rows' statistics.  BACK, on the device: the small structure arrays go up in one staged copy and
// one kernel over all 64-row blocks of all segments writes every array a plan holds, the padded ELL from
// the A that is still there.  The number of launches, copies and synchronisations is fixed.
//
// A segment with a stored off-diagonal entry whose mirror is not stored has entries in A that J lacks:
// it is flagged by the front and takes build_sa_layout whole; its A travels up inside the staged copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "asp_common.hpp"
#include "sa_colour.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

namespace {

using asp::DeviceBuffer;
using asp::SaHostLayout;

constexpr int kThreads = 256;
constexpr uint32_t kNoSegment = 0xFFFFFFFFu;
constexpr unsigned kMaxHostThreads = 16;

thread_local float t_last_ms = 0.0f;  // asp_sa_plan_segments_last_ms

// Per row, what the front hands to the host.
struct RowStats {
  double diagonal;   // J_ii where stored
  double abs_sum;    // sum_k |A_ik|, in a_ptr order
  double min_delta;  // smallest non-zero 2 |A_ik|, +inf: none
  uint32_t has_diagonal;
  uint32_t pad;
};

struct FrontArgs {
  const uint64_t *offsets;  // [G + 1]
  const int64_t *indptr;    // [T + 1]
  const int32_t *indices;   // [nnz], segment-local
  const double *data;       // [nnz]
  const double *field;      // [T]
  uint64_t num_segments, rows, nnz;
  double *merged;           // [nnz] J_ij + J_ji
  uint8_t *kept;            // [nnz] the entry is an entry of A
  uint32_t *row_count;      // [T]
  uint32_t *host_front;     // [G] a mirror is missing
  uint32_t *first_bad;      // the first segment with a content error, kNoSegment: none
};

// The segment of global row r: the last g with offsets[g] <= r (empty segments are skipped over).
__device__ __forceinline__ uint64_t segment_of_row(const uint64_t *__restrict__ offsets, uint64_t num_segments,
                                                   uint64_t r) {
  uint64_t lo = 0, hi = num_segments - 1;  // invariant: offsets[lo] <= r < offsets[hi + 1]
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (offsets[mid] <= r) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

// One thread per stored entry: validation (asp_sa_plan_create's content checks), the mirror, the sum.
__global__ __launch_bounds__(kThreads) void k_plan_front_entries(FrontArgs a) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; e < a.nnz; e += stride) {
    uint64_t lo = 0, hi = a.rows - 1;  // the row: indptr[lo] <= e < indptr[hi + 1]
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (static_cast<uint64_t>(a.indptr[mid]) <= e) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const uint64_t r = lo;
    const uint64_t g = segment_of_row(a.offsets, a.num_segments, r);
    const uint64_t base = a.offsets[g], n = a.offsets[g + 1] - base, i = r - base;
    const int32_t j = a.indices[e];
    const double x = a.data[e];
    bool bad = j < 0 || static_cast<uint64_t>(j) >= n;
    if (!bad && e > static_cast<uint64_t>(a.indptr[r]) && a.indices[e - 1] >= j) bad = true;
    if (!isfinite(x)) bad = true;
    if (bad) {
      atomicMin(a.first_bad, static_cast<uint32_t>(g));
      a.merged[e] = 0.0;
      a.kept[e] = 0;
      continue;
    }
    if (static_cast<uint64_t>(j) == i) {  // the diagonal: not an entry of A
      a.merged[e] = 0.0;
      a.kept[e] = 0;
      continue;
    }
    // J_ji by binary search in row j of the same segment (a row that is not sorted is an error found by
    // its own entries; the search stays inside the row whatever it holds)
    const int64_t begin = a.indptr[base + j], end = a.indptr[base + j + 1];
    int64_t left = begin, right = end;
    while (left < right) {
      const int64_t mid = left + (right - left) / 2;
      if (static_cast<uint64_t>(a.indices[mid]) < i && a.indices[mid] >= 0) {
        left = mid + 1;
      } else {
        right = mid;
      }
    }
    double y = 0.0;  // J_ji or +0
    if (left < end && a.indices[left] >= 0 && static_cast<uint64_t>(a.indices[left]) == i) {
      y = a.data[left];
    } else {
      atomicOr(&a.host_front[g], 1u);
    }
    const double v = x + y;
    a.merged[e] = v;
    a.kept[e] = v != 0.0 ? 1 : 0;
  }
}

// One thread per row: its number of entries in A, its stored diagonal, and the field's check.
__global__ __launch_bounds__(kThreads) void k_plan_front_count(FrontArgs a, RowStats *__restrict__ stats) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < a.rows; r += stride) {
    const uint64_t g = segment_of_row(a.offsets, a.num_segments, r);
    const uint64_t i = r - a.offsets[g];
    uint32_t count = 0, seen = 0;
    double d = 0.0;
    for (int64_t k = a.indptr[r]; k < a.indptr[r + 1]; ++k) {
      count += a.kept[k];
      if (a.indices[k] >= 0 && static_cast<uint64_t>(a.indices[k]) == i) {
        d = a.data[k];
        seen = 1;
      }
    }
    if (!isfinite(a.field[r])) atomicMin(a.first_bad, static_cast<uint32_t>(g));
    a.row_count[r] = count;
    stats[r].diagonal = d;
    stats[r].has_diagonal = seen;
    stats[r].pad = 0;
  }
}

// One thread per row: the row of A in ascending column order, and its statistics as k_rw_row_stats of
// csrc/sa_reweight.hip forms them (plain f64 adds, left to right).
__global__ __launch_bounds__(kThreads) void k_plan_front_fill(FrontArgs a, const int64_t *__restrict__ a_ptr,
                                                              int32_t *__restrict__ a_col,
                                                              double *__restrict__ a_val,
                                                              RowStats *__restrict__ stats) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < a.rows; r += stride) {
    int64_t at = a_ptr[r];
    double row = 0.0;
    double least = __longlong_as_double(0x7FF0000000000000ll);  // +inf
    for (int64_t k = a.indptr[r]; k < a.indptr[r + 1]; ++k) {
      if (!a.kept[k]) continue;
      const double v = a.merged[k];
      a_col[at] = a.indices[k];
      a_val[at] = v;
      ++at;
      const double m = fabs(v);
      row += m;
      const double twice = 2.0 * m;
      if (m > 0.0 && twice < least) least = twice;
    }
    stats[r].abs_sum = row;
    stats[r].min_delta = least;
  }
}

// What the back kernel knows of one segment: where its A and its structure lie, and the plan's arrays.
struct BackSegment {
  const int64_t *a_ptr;  // [n + 1]; its values index a_col / a_val
  const int32_t *a_col;
  const double *a_val;
  const double *field;             // [n] original order
  const uint32_t *st_pos_of_spin;  // the staged structure
  const uint32_t *st_spin_of_pos, *st_block_width, *st_color_block_start;
  const uint64_t *st_ell_off;
  uint32_t *color_block_start, *block_width, *ell_col, *ell_col4, *spin_of_pos, *pos_of_spin;  // the plan's
  uint64_t *ell_off;
  double *ell_val, *field_pos;
  uint32_t num_blocks, num_colors;
  uint32_t first_item;  // the segment's first work item: one per block, one for a segment without blocks
  uint32_t pad;
};

// One wavefront per 64-row block of any segment: lane l owns position b * 64 + l.  The block copies its
// share of the structure arrays and fills its slabs of the quad-interleaved ELL (sa_plan.cpp, "sliced
// ELL") a quad at a time: one 16-byte store of columns (and of wide-layout byte addresses) and two of
// values per lane, 1 KiB per wavefront store.  The last block of a segment adds the zero tail slabs.
__global__ __launch_bounds__(kThreads) void k_plan_back_fill(const BackSegment *__restrict__ segments,
                                                             uint32_t num_segments, uint32_t num_items) {
  const uint32_t lane = threadIdx.x % 64u;
  const uint32_t item = blockIdx.x * (kThreads / 64u) + threadIdx.x / 64u;
  if (item >= num_items) return;
  uint32_t lo = 0, hi = num_segments - 1;  // segments[lo].first_item <= item < segments[hi + 1].first_item
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (segments[mid].first_item <= item) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  const BackSegment &S = segments[lo];
  const uint32_t b = item - S.first_item;
  if (b == 0) {
    for (uint32_t c = lane; c <= S.num_colors; c += 64u) S.color_block_start[c] = S.st_color_block_start[c];
  }
  if (S.num_blocks == 0) {  // no spins: the plan holds color_block_start[1] and ell_off[1] only
    if (lane == 0) S.ell_off[0] = 0;
    return;
  }
  const uint32_t width = S.st_block_width[b];
  const uint64_t first_slab = S.st_ell_off[b];
  const bool last = b + 1 == S.num_blocks;
  if (lane == 0) {
    S.block_width[b] = width;
    S.ell_off[b] = first_slab;
    if (last) S.ell_off[b + 1] = S.st_ell_off[b + 1];
  }
  const uint32_t pos = b * 64u + lane;
  const uint32_t spin = S.st_spin_of_pos[pos];
  const bool real = spin != asp::kDummySpin;
  S.spin_of_pos[pos] = spin;
  S.field_pos[pos] = real ? S.field[spin] : 0.0;
  int64_t begin = 0, degree = 0;
  if (real) {
    S.pos_of_spin[spin] = pos;
    begin = S.a_ptr[spin];
    degree = S.a_ptr[spin + 1] - begin;
  }
  uint4 *col_out = reinterpret_cast<uint4 *>(S.ell_col);
  uint4 *col4_out = reinterpret_cast<uint4 *>(S.ell_col4);
  double2 *val_out = reinterpret_cast<double2 *>(S.ell_val);
  const uint64_t first_quad = first_slab / 4;  // (widths are multiples of 4)
  for (uint32_t q = 0; q < width / 4u; ++q) {
    uint32_t c[4];
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t k = static_cast<int64_t>(q) * 4 + j;
      if (k < degree) {
        c[j] = S.st_pos_of_spin[S.a_col[begin + k]];
        v[j] = S.a_val[begin + k];
      } else {  // padding: own position, +0.0
        c[j] = pos;
        v[j] = 0.0;
      }
    }
    const uint64_t quad = first_quad + q;
    col_out[quad * 64 + lane] = make_uint4(c[0], c[1], c[2], c[3]);
    if (col4_out) col4_out[quad * 64 + lane] = make_uint4(c[0] * 4u, c[1] * 4u, c[2] * 4u, c[3] * 4u);
    val_out[(quad * 2 + 0) * 64 + lane] = make_double2(v[0], v[1]);
    val_out[(quad * 2 + 1) * 64 + lane] = make_double2(v[2], v[3]);
  }
  if (last) {  // kEllTailSlabs slabs of zeros = two quads
    const uint64_t tail_quad = (first_slab + width) / 4;
    for (uint32_t q = 0; q < asp::kEllTailSlabs / 4; ++q) {
      col_out[(tail_quad + q) * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
      if (col4_out) col4_out[(tail_quad + q) * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
      val_out[((tail_quad + q) * 2 + 0) * 64 + lane] = make_double2(0.0, 0.0);
      val_out[((tail_quad + q) * 2 + 1) * 64 + lane] = make_double2(0.0, 0.0);
    }
  }
}
static_assert(asp::kEllTailSlabs % 4 == 0 && asp::kWidthAlign == 4, "the back kernel stores whole quads");

unsigned grid_for(uint64_t items) {  // (the front kernels stride over their items by the grid)
  return static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>((items + kThreads - 1) / kThreads, 1u << 16)));
}

struct Events {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t e : ev) {
      if (e) (void)hipEventDestroy(e);
    }
  }
  int create() {
    for (auto &e : ev) ASP_HIP_TRY(hipEventCreate(&e));
    return ASP_OK;
  }
};

// f(g) for every g < count on at most kMaxHostThreads host threads (ASP_HOST_THREADS lowers it), the
// segments handed out one at a time.  The machine's core count does not size it.
template <typename F>
void for_each_segment(uint64_t count, unsigned workers, F f) {
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t g = next.fetch_add(1); g < count; g = next.fetch_add(1)) f(g);
  };
  std::vector<std::thread> pool;
  pool.reserve(workers > 0 ? workers - 1 : 0);
  for (unsigned t = 1; t < workers; ++t) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
}

unsigned pool_size(uint64_t num_segments) {
  unsigned limit = kMaxHostThreads;
  if (const char *env = std::getenv("ASP_HOST_THREADS")) {
    const int forced = std::atoi(env);
    if (forced >= 1) limit = std::min<unsigned>(static_cast<unsigned>(forced), kMaxHostThreads);
  }
  return static_cast<unsigned>(std::min<uint64_t>(limit, std::max<uint64_t>(1, num_segments)));
}

template <typename T>
size_t words_of(size_t count) {  // 8-byte words that hold `count` elements of T
  return (count * sizeof(T) + 7) / 8;
}

struct PlanDeleter {
  void operator()(asp_sa_plan *p) const { asp_sa_plan_destroy(p); }
};

int create_segments(uint64_t G, uint64_t T, const uint64_t *offsets, const int64_t *indptr, const int32_t *indices,
                    const double *data, const double *field, asp_sa_plan **out_plans) {
  const uint64_t nnz = T ? static_cast<uint64_t>(indptr[T]) : 0;
  // ASP_PLAN_SEGMENTS_TIMING=1: wall time of the call's steps on stderr (development aid; tools/time_plan_segments.py)
  const bool timing = std::getenv("ASP_PLAN_SEGMENTS_TIMING") != nullptr;
  auto step_start = std::chrono::steady_clock::now();
  auto step = [&](const char *name) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "  plan segments %-7s %9.3f ms\n", name,
                 std::chrono::duration<double, std::milli>(now - step_start).count());
    step_start = now;
  };
  std::vector<std::unique_ptr<asp_sa_plan, PlanDeleter>> plans(G);
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  int num_cus = 0;
  size_t max_lds = 0;
  ASP_TRY(asp::device_limits(&num_cus, &max_lds));
  int team_mode = -1;  // ASP_SA_TEAM, as asp_sa_plan_create reads it
  if (const char *env = std::getenv("ASP_SA_TEAM")) {
    const int team = std::atoi(env);
    if (team == 0 || team == 2 || team == 4 || team == 8) team_mode = team;
  }
  // host landing places of the front (declared before the buffers: the fence below waits first)
  std::vector<int64_t> a_ptr(T + 1, 0);
  std::vector<int32_t> a_col(nnz);
  std::vector<double> a_val(nnz);
  std::vector<RowStats> stats(T);
  std::vector<uint32_t> flags(G + 1, 0);  // host_front[G] | first_bad
  flags[G] = kNoSegment;
  std::vector<uint64_t> staged;
  std::vector<BackSegment> table(G);
  DeviceBuffer<uint64_t> d_offsets, d_staged;
  DeviceBuffer<int64_t> d_indptr, d_a_ptr, d_scratch;
  DeviceBuffer<int32_t> d_indices, d_a_col;
  DeviceBuffer<double> d_data, d_field, d_merged, d_a_val;
  DeviceBuffer<uint8_t> d_kept;
  DeviceBuffer<uint32_t> d_row_count, d_flags;
  DeviceBuffer<RowStats> d_stats;
  DeviceBuffer<BackSegment> d_table;
  Events events;
  asp::StreamFence fence(stream);  // error exits wait for the stream before the buffers and vectors go
  ASP_TRY(events.create());
  float device_ms = 0.0f;
  if (T > 0) {
    // ---- front -------------------------------------------------------------------------------
    ASP_TRY(d_offsets.alloc(G + 1));
    ASP_TRY(d_indptr.alloc(T + 1));
    ASP_TRY(d_indices.alloc(nnz));
    ASP_TRY(d_data.alloc(nnz));
    ASP_TRY(d_field.alloc(T));
    ASP_TRY(d_merged.alloc(nnz));
    ASP_TRY(d_kept.alloc(nnz));
    ASP_TRY(d_row_count.alloc(T));
    ASP_TRY(d_flags.alloc(G + 1));
    ASP_TRY(d_stats.alloc(T));
    ASP_TRY(d_a_ptr.alloc(T + 1));
    ASP_TRY(d_a_col.alloc(nnz));
    ASP_TRY(d_a_val.alloc(nnz));
    ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(T)));
    ASP_TRY(d_offsets.upload(offsets, G + 1, stream));
    ASP_TRY(d_indptr.upload(indptr, T + 1, stream));
    ASP_TRY(d_indices.upload(indices, nnz, stream));
    ASP_TRY(d_data.upload(data, nnz, stream));
    ASP_TRY(d_field.upload(field, T, stream));
    ASP_HIP_TRY(hipMemsetAsync(d_flags.ptr, 0, G * sizeof(uint32_t), stream));
    ASP_HIP_TRY(hipMemsetAsync(d_flags.ptr + G, 0xFF, sizeof(uint32_t), stream));  // kNoSegment
    ASP_HIP_TRY(hipEventRecord(events.ev[0], stream));
    FrontArgs args{d_offsets.ptr, d_indptr.ptr, d_indices.ptr, d_data.ptr, d_field.ptr, G, T, nnz,
                   d_merged.ptr, d_kept.ptr, d_row_count.ptr, d_flags.ptr, d_flags.ptr + G};
    if (nnz > 0) {
      hipLaunchKernelGGL(k_plan_front_entries, dim3(grid_for(nnz)), dim3(kThreads), 0, stream, args);
    }
    hipLaunchKernelGGL(k_plan_front_count, dim3(grid_for(T)), dim3(kThreads), 0, stream, args, d_stats.ptr);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(asp::exclusive_scan_u32(d_row_count.ptr, T, d_a_ptr.ptr, d_scratch.ptr, stream));
    hipLaunchKernelGGL(k_plan_front_fill, dim3(grid_for(T)), dim3(kThreads), 0, stream, args, d_a_ptr.ptr,
                       d_a_col.ptr, d_a_val.ptr, d_stats.ptr);
    ASP_HIP_TRY(hipGetLastError());
    ASP_HIP_TRY(hipEventRecord(events.ev[1], stream));
    ASP_TRY(d_flags.download(flags.data(), G + 1, stream));
    ASP_TRY(d_a_ptr.download(a_ptr.data(), T + 1, stream));
    ASP_TRY(d_a_col.download(a_col.data(), nnz, stream));
    ASP_TRY(d_a_val.download(a_val.data(), nnz, stream));
    ASP_TRY(d_stats.download(stats.data(), T, stream));
    ASP_HIP_TRY(hipStreamSynchronize(stream));  // first synchronisation
    float ms = 0.0f;
    ASP_HIP_TRY(hipEventElapsedTime(&ms, events.ev[0], events.ev[1]));
    device_ms += ms;
  }
  step("front");
  // ---- host: per segment the layout's back and the scales ------------------------------------------
  const uint64_t first_bad = flags[G] == kNoSegment ? G : flags[G];
  std::vector<int> rc_of(G, ASP_OK);
  std::vector<std::string> message_of(G);
  // (a segment after the first one in error is never looked at: the call fails with that one)
  const uint64_t to_build = std::min<uint64_t>(G, first_bad + 1);
  const unsigned workers = pool_size(to_build);
  for_each_segment(to_build, workers, [&](uint64_t g) {
    const uint64_t base = offsets[g], n = offsets[g + 1] - base;
    asp_sa_plan *p = new (std::nothrow) asp_sa_plan();
    if (!p) {
      rc_of[g] = ASP_ERR_ALLOC;
      message_of[g] = "out of host memory";
      return;
    }
    plans[g].reset(p);
    SaHostLayout &L = p->host;
    const int64_t first = n ? indptr[base] : 0;
    std::vector<int64_t> local;  // the segment's indptr from 0 (the pattern's, too)
    if (n > 0) {
      local.resize(n + 1);
      for (uint64_t i = 0; i <= n; ++i) local[i] = indptr[base + i] - first;
    }
    int rc = ASP_OK;
    if (n == 0 || flags[g] != 0 || g == first_bad) {
      // no spins, a missing mirror, or the content error whose message asp_sa_plan_create words
      rc = asp::build_sa_layout(n, local.data(), indices ? indices + first : nullptr, data ? data + first : nullptr,
                                field ? field + base : nullptr, &L);
      if (rc == ASP_OK && g == first_bad) {
        rc = asp::set_error(ASP_ERR_INVALID, "the device refused the segment and the host accepts it");
      }
    } else if (n >= (1ull << 31)) {
      rc = asp::set_error(ASP_ERR_TOO_LARGE, "%llu spins exceed the 2^31 limit", (unsigned long long)n);
    } else {
      asp::sa_layout_count_build();
      L = SaHostLayout();
      L.num_spins = n;
      const int64_t a_first = a_ptr[base];
      L.a_ptr.resize(n + 1);
      for (uint64_t i = 0; i <= n; ++i) L.a_ptr[i] = a_ptr[base + i] - a_first;
      L.a_col.assign(a_col.begin() + a_first, a_col.begin() + a_ptr[base + n]);
      L.a_val.assign(a_val.begin() + a_first, a_val.begin() + a_ptr[base + n]);
      double diag = 0.0;  // D in row order
      std::vector<double> row_sum(n), row_min(n);
      for (uint64_t i = 0; i < n; ++i) {
        const RowStats &s = stats[base + i];
        if (s.has_diagonal) diag = diag + s.diagonal;
        row_sum[i] = s.abs_sum;
        row_min[i] = s.min_delta;
      }
      L.diag_sum = diag;
      rc = asp::sa_layout_back(field + base, workers > 1 ? 1u : asp::sa_layout_host_threads(n), &L);
      if (rc == ASP_OK) rc = asp::sa_layout_scales_from_rows(field + base, row_sum.data(), row_min.data(), &L);
    }
    if (rc != ASP_OK) {
      rc_of[g] = rc;
      message_of[g] = asp::error_state().message;
      return;
    }
    p->pattern = std::make_shared<asp::SaPattern>();
    if (n > 0) {
      p->pattern->nnz = static_cast<uint64_t>(local[n]);
      p->pattern->indptr.swap(local);
      p->pattern->indices.assign(indices + first, indices + first + p->pattern->nnz);
    }
    p->team_mode = team_mode;
    p->num_cus = num_cus;
    p->max_lds = max_lds;
  });
  for (uint64_t g = 0; g < to_build; ++g) {
    if (rc_of[g] != ASP_OK) {
      return asp::set_error(rc_of[g], "segment %llu: %s", (unsigned long long)g, message_of[g].c_str());
    }
  }
  step("host");
  // ---- back ----------------------------------------------------------------------------------------
  // every plan's stream, events and arrays; the staged structure and the table of segments
  uint64_t items = 0;
  size_t staged_words = 0;
  for (uint64_t g = 0; g < G; ++g) {
    asp_sa_plan *p = plans[g].get();
    ASP_TRY(asp::stream_acquire(&p->stream));
    for (auto &e : p->ev) ASP_HIP_TRY(hipEventCreate(&e));
  }
  step("handles");
  for (uint64_t g = 0; g < G; ++g) {
    asp_sa_plan *p = plans[g].get();
    const SaHostLayout &L = p->host;
    ASP_TRY(p->color_block_start.alloc(L.color_block_start.size()));
    ASP_TRY(p->block_width.alloc(L.block_width.size()));
    ASP_TRY(p->ell_off.alloc(L.ell_off.size()));
    ASP_TRY(p->ell_col.alloc(L.ell_col.size()));
    ASP_TRY(p->ell_val.alloc(L.ell_val.size()));
    ASP_TRY(p->spin_of_pos.alloc(L.spin_of_pos.size()));
    ASP_TRY(p->pos_of_spin.alloc(L.pos_of_spin.size()));
    ASP_TRY(p->field_pos.alloc(L.field_pos.size()));
    if (asp::colour::sweep_lds_bytes(L, asp::colour::kWide) <= p->max_lds) ASP_TRY(p->ell_col4.alloc(L.ell_col.size()));
    BackSegment &S = table[g];
    std::memset(&S, 0, sizeof S);
    S.num_blocks = L.num_blocks;
    S.num_colors = L.num_colors;
    S.first_item = static_cast<uint32_t>(items);
    items += std::max<uint32_t>(L.num_blocks, 1u);
    if (items >= 0xFFFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 2 blocks in one round");
    staged_words += words_of<uint32_t>(L.pos_of_spin.size()) + words_of<uint32_t>(L.spin_of_pos.size()) +
                    words_of<uint32_t>(L.block_width.size()) + words_of<uint32_t>(L.color_block_start.size()) +
                    L.ell_off.size();
    if (L.num_spins > 0 && flags[g] != 0) {
      staged_words += L.a_ptr.size() + words_of<int32_t>(L.a_col.size()) + L.a_val.size();
    }
  }
  step("alloc");
  staged.assign(staged_words, 0);
  ASP_TRY(d_staged.alloc(staged_words));
  ASP_TRY(d_table.alloc(G));
  size_t at = 0;
  auto stage_in = [&](const void *src, size_t bytes, size_t words) {
    if (bytes) std::memcpy(staged.data() + at, src, bytes);
    const uint64_t *where = d_staged.ptr + at;
    at += words;
    return where;
  };
  for (uint64_t g = 0; g < G; ++g) {
    asp_sa_plan *p = plans[g].get();
    const SaHostLayout &L = p->host;
    BackSegment &S = table[g];
    const uint64_t base = offsets[g];
    S.st_pos_of_spin = reinterpret_cast<const uint32_t *>(
        stage_in(L.pos_of_spin.data(), L.pos_of_spin.size() * 4, words_of<uint32_t>(L.pos_of_spin.size())));
    S.st_spin_of_pos = reinterpret_cast<const uint32_t *>(
        stage_in(L.spin_of_pos.data(), L.spin_of_pos.size() * 4, words_of<uint32_t>(L.spin_of_pos.size())));
    S.st_block_width = reinterpret_cast<const uint32_t *>(
        stage_in(L.block_width.data(), L.block_width.size() * 4, words_of<uint32_t>(L.block_width.size())));
    S.st_color_block_start = reinterpret_cast<const uint32_t *>(stage_in(
        L.color_block_start.data(), L.color_block_start.size() * 4, words_of<uint32_t>(L.color_block_start.size())));
    S.st_ell_off = stage_in(L.ell_off.data(), L.ell_off.size() * 8, L.ell_off.size());
    if (L.num_spins > 0 && flags[g] != 0) {  // A of the host front
      S.a_ptr = reinterpret_cast<const int64_t *>(stage_in(L.a_ptr.data(), L.a_ptr.size() * 8, L.a_ptr.size()));
      S.a_col = reinterpret_cast<const int32_t *>(
          stage_in(L.a_col.data(), L.a_col.size() * 4, words_of<int32_t>(L.a_col.size())));
      S.a_val = reinterpret_cast<const double *>(stage_in(L.a_val.data(), L.a_val.size() * 8, L.a_val.size()));
    } else if (L.num_spins > 0) {  // A of the device front: global row pointers into the round's arrays
      S.a_ptr = d_a_ptr.ptr + base;
      S.a_col = d_a_col.ptr;
      S.a_val = d_a_val.ptr;
    }
    S.field = L.num_spins > 0 ? d_field.ptr + base : nullptr;
    S.color_block_start = p->color_block_start.ptr;
    S.block_width = p->block_width.ptr;
    S.ell_col = p->ell_col.ptr;
    S.ell_col4 = p->ell_col4.ptr;
    S.spin_of_pos = p->spin_of_pos.ptr;
    S.pos_of_spin = p->pos_of_spin.ptr;
    S.ell_off = p->ell_off.ptr;
    S.ell_val = p->ell_val.ptr;
    S.field_pos = p->field_pos.ptr;
  }
  ASP_TRY(d_staged.upload(staged.data(), staged_words, stream));
  ASP_TRY(d_table.upload(table.data(), G, stream));
  ASP_HIP_TRY(hipEventRecord(events.ev[2], stream));
  const unsigned per_group = kThreads / 64;
  hipLaunchKernelGGL(k_plan_back_fill, dim3(static_cast<unsigned>((items + per_group - 1) / per_group)), dim3(kThreads),
                     0, stream, d_table.ptr, static_cast<uint32_t>(G), static_cast<uint32_t>(items));
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev[3], stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));  // second synchronisation: the plans are ready on any stream
  float ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&ms, events.ev[2], events.ev[3]));
  t_last_ms = device_ms + ms;
  step("back");
  for (uint64_t g = 0; g < G; ++g) out_plans[g] = plans[g].release();
  return ASP_OK;
}

}  // namespace

extern "C" {

int asp_sa_plan_create_segments(uint64_t num_segments, uint64_t const *offsets, int64_t const *indptr,
                                int32_t const *indices, double const *data, double const *field,
                                asp_sa_plan **out_plans) {
  asp_clear_error();
  t_last_ms = 0.0f;
  const uint64_t G = num_segments;
  if (G == 0) return ASP_OK;  // nothing to make: no device needed
  // (every check before any device work)
  if (!out_plans) return asp::set_error(ASP_ERR_INVALID, "null out_plans with %llu segments", (unsigned long long)G);
  for (uint64_t g = 0; g < G; ++g) out_plans[g] = nullptr;
  if (!offsets) return asp::set_error(ASP_ERR_INVALID, "null offsets with %llu segments", (unsigned long long)G);
  if (offsets[0] != 0) return asp::set_error(ASP_ERR_INVALID, "offsets[0] must be 0");
  for (uint64_t g = 0; g < G; ++g) {
    if (offsets[g + 1] < offsets[g]) return asp::set_error(ASP_ERR_INVALID, "offsets decrease at segment %llu", (unsigned long long)g);
  }
  const uint64_t T = offsets[G];
  if (G >= 0xFFFFFFFFull || T >= 0xFFFFFFFFull) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%llu spins in %llu segments exceed the 2^32 - 2 limit",
                          (unsigned long long)T, (unsigned long long)G);
  }
  if (T > 0) {
    if (!indptr || !field) return asp::set_error(ASP_ERR_INVALID, "null indptr/field");
    if (indptr[0] != 0) return asp::set_error(ASP_ERR_INVALID, "indptr[0] must be 0");
    for (uint64_t i = 0; i < T; ++i) {
      if (indptr[i + 1] < indptr[i]) return asp::set_error(ASP_ERR_INVALID, "indptr is not monotone");
    }
    const uint64_t nnz = static_cast<uint64_t>(indptr[T]);
    if (nnz >= 0xFFFFFFFFull) {
      return asp::set_error(ASP_ERR_TOO_LARGE, "%llu stored couplings exceed the 2^32 - 2 limit", (unsigned long long)nnz);
    }
    if (nnz > 0 && (!indices || !data)) return asp::set_error(ASP_ERR_INVALID, "null indices/data");
  }
  ASP_TRY(asp::require_device());
  return create_segments(G, T, offsets, indptr, indices, data, field, out_plans);
}

float asp_sa_plan_segments_last_ms(void) { return t_last_ms; }

int asp_sa_plan_read_array(asp_sa_plan const *p, int which, void *dst, uint64_t capacity_bytes, uint64_t *bytes) {
  asp_clear_error();
  if (bytes) *bytes = 0;
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (!bytes) return asp::set_error(ASP_ERR_INVALID, "null byte count");
  const void *src = nullptr;
  uint64_t size = 0;
  auto take = [&](const auto &buffer) {
    src = buffer.ptr;
    size = buffer.ptr ? buffer.count * sizeof(*buffer.ptr) : 0;
  };
  switch (which) {
    case ASP_SA_ARRAY_COLOR_BLOCK_START: take(p->color_block_start); break;
    case ASP_SA_ARRAY_BLOCK_WIDTH: take(p->block_width); break;
    case ASP_SA_ARRAY_ELL_OFF: take(p->ell_off); break;
    case ASP_SA_ARRAY_ELL_COL: take(p->ell_col); break;
    case ASP_SA_ARRAY_ELL_COL4: take(p->ell_col4); break;
    case ASP_SA_ARRAY_ELL_VAL: take(p->ell_val); break;
    case ASP_SA_ARRAY_SPIN_OF_POS: take(p->spin_of_pos); break;
    case ASP_SA_ARRAY_POS_OF_SPIN: take(p->pos_of_spin); break;
    case ASP_SA_ARRAY_FIELD_POS: take(p->field_pos); break;
    default: return asp::set_error(ASP_ERR_INVALID, "unknown plan array %d", which);
  }
  *bytes = size;
  if (size > capacity_bytes || (size > 0 && !dst)) {
    return asp::set_error(ASP_ERR_INVALID, "the array holds %llu bytes, the buffer %llu", (unsigned long long)size,
                          (unsigned long long)capacity_bytes);
  }
  if (size == 0) return ASP_OK;
  ASP_TRY(asp::bind_device());
  ASP_HIP_TRY(hipMemcpyAsync(dst, src, size, hipMemcpyDeviceToHost, p->stream));
  ASP_HIP_TRY(hipStreamSynchronize(p->stream));
  return ASP_OK;
}

}  // extern "C"
