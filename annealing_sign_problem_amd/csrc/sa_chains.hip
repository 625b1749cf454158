// asp_sa_chains: resumable annealing chains (include/asp.h section 4).
//
// A handle is a set of chains of one plan whose state lives on the device BETWEEN calls, in a form
// that depends on nothing the launcher chooses: the current and the best configuration of every
// chain packed in original spin order (bit = +1), the current and the best tracked energy, the
// accepted flips, and one sweep counter.  asp_sa_chains_advance runs a segment of sweeps from that
// state in either visiting order (csrc/sa_sweep.hip: k_sa_sweep_resume; csrc/sa_shuffled.hip: the
// chunked sweep started from a loaded state) with the sweep index of the random words and of the
// shuffled orders counted from the chains' first sweep, so any split of a schedule into segments is
// the closed call's chain, bit for bit.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "asp_common.hpp"
#include "sa_device.hpp"
#include "sa_internal.hpp"

namespace {

using namespace asp::dev;

// The random start of the closed calls (x0 == NULL): spin i of global replica r is up iff bit 0 of
// word r % 4 of Philox4x32-10(counter (i, 2^32 - 1, r / 4, 0), key seed) is set.  A wavefront per
// word of a chain; lane j owns spin 64 w + j and the word is one ballot.
__global__ __launch_bounds__(256) void k_chains_random_start(uint64_t seed, uint32_t replica_first,
                                                             uint32_t num_spins, uint32_t words,
                                                             uint64_t *__restrict__ x) {
  const uint32_t chain = blockIdx.x, lane = threadIdx.x & 63u;
  const uint32_t r = replica_first + chain;
  for (uint32_t w = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6); w < words;
       w += gridDim.y * (blockDim.x >> 6)) {
    const uint32_t i = w * 64u + lane;  // (w is uniform over the wavefront)
    bool up = false;
    if (i < num_spins) {
      const Philox4 rnd = philox4x32_10(i, 0xFFFFFFFFu, r >> 2, 0u, static_cast<uint32_t>(seed),
                                        static_cast<uint32_t>(seed >> 32));
      up = (pick_word(rnd, r & 3u) & 1u) != 0u;
    }
    const uint64_t word = __ballot(up);
    if (lane == 0) x[static_cast<uint64_t>(chain) * words + w] = word;
  }
}

// `count` configurations of `words` words, `stride` words apart (0: the same one for all), with the
// bits past the last spin cleared — the closed calls never report them, and a configuration that is
// never improved on is reported as it came in.
std::vector<uint64_t> staged(const uint64_t *x, uint64_t stride, uint32_t count, uint32_t words, uint64_t num_spins) {
  std::vector<uint64_t> out(static_cast<size_t>(count) * words);
  const uint64_t tail = (num_spins & 63u) ? (1ull << (num_spins & 63u)) - 1ull : ~0ull;
  for (uint32_t r = 0; r < count; ++r) {
    const uint64_t *row = x + static_cast<uint64_t>(r) * stride;
    for (uint32_t w = 0; w < words; ++w) out[static_cast<size_t>(r) * words + w] = row[w];
    if (words) out[static_cast<size_t>(r) * words + words - 1] &= tail;
  }
  return out;
}

bool nothing_to_run(const asp_sa_chains *c) { return c->repetitions == 0 || c->plan->host.num_spins == 0; }

// Progress of a batched segment (asp_sa_chains_advance_batch): what asp_sa_chains_export before and
// after the segment would tell, for every handle of the batch in ONE buffer and one copy to the host.
// Row i of `table` describes handle i; its chains own `out` entries [at, at + chains) of three planes
// of `total` entries each: the best tracked energies before the segment (kept on the device), after
// it, and the current ones (the host's entry 0 of the next trace); improved[i] counts the chains whose
// best fell strictly.
struct ProgressRow {
  const long long *e_cur, *e_best;
  uint64_t at;
  uint32_t chains;
};
// after = false: before the sweeps (plane 0); true: after them (planes 1 and 2, the counts).
// A workgroup per handle.
__global__ __launch_bounds__(256) void k_chains_progress(const ProgressRow *table, uint64_t total, bool after,
                                                         long long *__restrict__ out,
                                                         uint32_t *__restrict__ improved) {
  const ProgressRow row = table[blockIdx.x];
  uint32_t fell = 0;
  for (uint32_t r = threadIdx.x; r < row.chains; r += blockDim.x) {
    const long long best = row.e_best[r];
    if (!after) {
      out[row.at + r] = best;
    } else {
      out[total + row.at + r] = best;
      out[2 * total + row.at + r] = row.e_cur[r];
      fell += best < out[row.at + r] ? 1u : 0u;
    }
  }
  if (!after) return;
  __shared__ uint32_t sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  if (fell) atomicAdd(&sum, fell);
  __syncthreads();
  if (threadIdx.x == 0) improved[blockIdx.x] = sum;
}

thread_local float g_chains_batch_ms = 0.0f;

// One validated item of asp_sa_chains_advance_batch (betas) or asp_sa_chains_advance_ladder_batch
// (chain_betas); a call holds one kind only.
struct BatchSegment {
  asp_sa_chains *chains;
  double const *betas, *chain_betas;
  uint32_t num_sweeps, order;
  int64_t *out_trace, *out_tracked_best;
  uint32_t *out_improved;
};

int check_distinct_plans(const std::vector<BatchSegment> &items) {
  std::vector<asp_sa_chains *> handles(items.size());
  for (size_t i = 0; i < items.size(); ++i) handles[i] = items[i].chains;
  return asp::check_distinct_plans(handles);
}

// The device half of the two batched advances: progress before, the segments, progress after.
int run_batch_segments(const std::vector<BatchSegment> &items) {
  const uint32_t count = static_cast<uint32_t>(items.size());
  ASP_TRY(asp::bind_device());
  // ---- progress, before: the best tracked energies of every handle that is asked about ----
  bool wanted = false;
  std::vector<ProgressRow> rows(count);
  uint64_t total = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains *c = items[i].chains;
    rows[i] = ProgressRow{c->e_cur.ptr, c->e_best.ptr, total, c->repetitions};
    total += c->repetitions;
    wanted = wanted || items[i].out_tracked_best || items[i].out_improved;
  }
  asp::DeviceBuffer<ProgressRow> d_rows;
  asp::DeviceBuffer<long long> d_progress;  // [3][total] | improved[count] in the words behind
  asp::ScopedStream progress_stream;
  const uint64_t progress_words = 3 * total + (count + 1ull) / 2;
  uint32_t *d_improved = nullptr;
  if (total != 0) {
    ASP_TRY(progress_stream.acquire());
    ASP_TRY(d_rows.alloc(count));
    ASP_TRY(d_progress.alloc(progress_words));
    d_improved = reinterpret_cast<uint32_t *>(d_progress.ptr + 3 * total);
    ASP_TRY(d_rows.upload(rows.data(), count, progress_stream.stream));
    if (wanted) {
      hipLaunchKernelGGL(k_chains_progress, dim3(count), dim3(256), 0, progress_stream.stream, d_rows.ptr, total,
                         false, d_progress.ptr, d_improved);
      ASP_HIP_TRY(hipGetLastError());
    }
    ASP_HIP_TRY(hipStreamSynchronize(progress_stream.stream));
  }
  // ---- the segments: per visiting order, the handles that fit in shared launches ----
  std::vector<std::vector<int64_t>> starts(count);  // entry 0 of every traced row: NOT reset to 0
  std::vector<asp::ChainsSegment> colour, shuffled;
  for (uint32_t i = 0; i < count; ++i) {
    const BatchSegment &it = items[i];
    if (it.out_trace) starts[i] = it.chains->h_e_cur;
    if (it.num_sweeps == 0 || nothing_to_run(it.chains)) {
      if (it.out_trace) {  // (no spins: the energy stays where it is; no sweeps: the single entry below)
        for (uint64_t k = 0; k < static_cast<uint64_t>(it.chains->repetitions) * (it.num_sweeps + 1ull); ++k) {
          it.out_trace[k] = 0;
        }
      }
      continue;
    }
    (it.order == 0 ? colour : shuffled)
        .push_back(asp::ChainsSegment{it.chains, it.betas, it.num_sweeps, it.out_trace, it.chain_betas});
  }
  if (!shuffled.empty()) {
    ASP_TRY(asp::sa_chains_advance_shuffled_batch(shuffled.data(), static_cast<uint32_t>(shuffled.size()),
                                                  &g_chains_batch_ms));
  }
  if (!colour.empty()) {
    ASP_TRY(asp::sa_chains_advance_colour_batch(colour.data(), static_cast<uint32_t>(colour.size()),
                                                &g_chains_batch_ms));
  }
  // ---- progress, after: one gather launch and one copy for the whole batch ----
  std::vector<long long> h_progress(progress_words, 0);
  if (total != 0) {
    hipLaunchKernelGGL(k_chains_progress, dim3(count), dim3(256), 0, progress_stream.stream, d_rows.ptr, total, true,
                       d_progress.ptr, d_improved);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(d_progress.download(h_progress.data(), progress_words, progress_stream.stream));
    ASP_HIP_TRY(hipStreamSynchronize(progress_stream.stream));
  }
  const uint32_t *h_improved = reinterpret_cast<const uint32_t *>(h_progress.data() + 3 * total);
  for (uint32_t i = 0; i < count; ++i) {
    const BatchSegment &it = items[i];
    asp_sa_chains *c = it.chains;
    const uint32_t R = c->repetitions;
    for (uint32_t r = 0; r < R; ++r) c->h_e_cur[r] = h_progress[2 * total + rows[i].at + r];
    if (it.out_tracked_best) {
      for (uint32_t r = 0; r < R; ++r) it.out_tracked_best[r] = h_progress[total + rows[i].at + r];
    }
    if (it.out_improved) *it.out_improved = total != 0 ? h_improved[i] : 0u;
    if (it.out_trace) {
      for (uint32_t r = 0; r < R; ++r) it.out_trace[static_cast<uint64_t>(r) * (it.num_sweeps + 1ull)] = starts[i][r];
    }
    c->sweeps_done += it.num_sweeps;
  }
  return ASP_OK;
}

}  // namespace

extern "C" {

int asp_sa_chains_create(asp_sa_plan *p, uint64_t seed, uint32_t repetitions, uint32_t replica_offset,
                         uint64_t const *x0, uint64_t x0_stride, asp_sa_chains **out) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output pointer");
  const uint64_t K = p->host.num_spins;
  const uint32_t words = static_cast<uint32_t>((K + 63) / 64);
  if (x0 && x0_stride != 0 && x0_stride < words) {
    return asp::set_error(ASP_ERR_INVALID, "x0_stride %llu is neither 0 nor at least the %u words of a configuration",
                          static_cast<unsigned long long>(x0_stride), words);
  }
  if (static_cast<uint64_t>(replica_offset) + repetitions + 8 > 0xFFFFFFFFull) {
    return asp::set_error(ASP_ERR_INVALID, "replica ids exceed 32 bits");
  }
  ASP_TRY(asp::bind_device());
  asp_sa_chains *c = new (std::nothrow) asp_sa_chains;
  if (!c) return asp::set_error(ASP_ERR_ALLOC, "out of host memory");
  c->plan = p;
  c->seed = seed;
  c->repetitions = repetitions;
  c->replica_offset = replica_offset;
  c->words = words;
  c->h_e_cur.assign(repetitions, 0);
  const uint64_t state_words = static_cast<uint64_t>(repetitions) * words;
  hipStream_t s = p->stream;
  std::vector<uint64_t> start;  // (alive until the stream has been waited for)
  auto run = [&]() -> int {
    ASP_TRY(c->x_cur.alloc(state_words));
    ASP_TRY(c->x_best.alloc(state_words));
    ASP_TRY(c->e_cur.alloc(repetitions));
    ASP_TRY(c->e_best.alloc(repetitions));
    ASP_TRY(c->accepted.alloc(repetitions));
    asp::StreamFence fence(s);
    ASP_HIP_TRY(hipMemsetAsync(c->e_cur.ptr, 0, (repetitions ? repetitions : 1) * 8ull, s));
    ASP_HIP_TRY(hipMemsetAsync(c->e_best.ptr, 0, (repetitions ? repetitions : 1) * 8ull, s));
    ASP_HIP_TRY(hipMemsetAsync(c->accepted.ptr, 0, (repetitions ? repetitions : 1) * 8ull, s));
    if (state_words == 0) return ASP_OK;
    if (!x0) {
      const dim3 grid(repetitions, std::min(words / 4u + 1u, 1024u));
      hipLaunchKernelGGL(k_chains_random_start, grid, dim3(256), 0, s, seed, replica_offset,
                         static_cast<uint32_t>(K), words, c->x_cur.ptr);
      ASP_HIP_TRY(hipGetLastError());
    } else {
      start = staged(x0, x0_stride, repetitions, words, K);
      ASP_TRY(c->x_cur.upload(start.data(), state_words, s));
    }
    // (the best configuration so far is the start)
    ASP_HIP_TRY(hipMemcpyAsync(c->x_best.ptr, c->x_cur.ptr, state_words * 8, hipMemcpyDeviceToDevice, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
    return ASP_OK;
  };
  const int rc = run();
  if (rc != ASP_OK) {
    delete c;
    return rc;
  }
  c->live_of_plan = p->live_chains;
  c->live_of_plan->fetch_add(1, std::memory_order_relaxed);
  *out = c;
  return ASP_OK;
}

void asp_sa_chains_destroy(asp_sa_chains *c) {
  // (every entry point waits for its stream before it returns: the buffers are idle; the plan is
  // not touched, so a handle may outlive its plan as long as it is only destroyed)
  if (c && c->live_of_plan) c->live_of_plan->fetch_sub(1, std::memory_order_relaxed);
  delete c;
}

int asp_sa_chains_advance(asp_sa_chains *c, double const *betas, uint32_t num_sweeps, uint32_t order,
                          int64_t *out_trace) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (num_sweeps && !betas) return asp::set_error(ASP_ERR_INVALID, "null betas");
  if (order > 1u) return asp::set_error(ASP_ERR_INVALID, "order must be 0 (colour) or 1 (shuffled)");
  // t = 2^32 - 1 is the counter of the random start, 2^32 - 2 the largest number of sweeps of a closed call
  if (static_cast<uint64_t>(c->sweeps_done) + num_sweeps > 0xFFFFFFFEull) {
    return asp::set_error(ASP_ERR_INVALID, "%u sweeps after %u exceed the 2^32 - 2 sweep indices of a chain",
                          num_sweeps, c->sweeps_done);
  }
  for (uint32_t t = 0; t < num_sweeps; ++t) {
    if (!(betas[t] >= 0.0)) return asp::set_error(ASP_ERR_INVALID, "betas[%u] is not >= 0", t);
  }
  ASP_TRY(asp::bind_device());
  const uint32_t R = c->repetitions;
  const std::vector<int64_t> start = c->h_e_cur;  // entry 0 of every row: NOT reset to 0
  if (num_sweeps != 0 && !nothing_to_run(c)) {
    c->plan->last_sweep_ms = c->plan->last_total_ms = 0.0f;
    ASP_TRY(order == 0 ? asp::sa_chains_advance_colour(c, betas, num_sweeps, out_trace)
                       : asp::sa_chains_advance_shuffled(c, betas, num_sweeps, out_trace));
  } else if (out_trace) {
    // (no spins: the energy stays where it is; no sweeps: the single entry below)
    for (uint64_t k = 0; k < static_cast<uint64_t>(R) * (num_sweeps + 1ull); ++k) out_trace[k] = 0;
  }
  if (out_trace) {
    for (uint32_t r = 0; r < R; ++r) out_trace[static_cast<uint64_t>(r) * (num_sweeps + 1ull)] = start[r];
  }
  c->sweeps_done += num_sweeps;
  return ASP_OK;
}

int asp_sa_chains_advance_ladder(asp_sa_chains *c, double const *chain_betas, uint32_t num_sweeps, uint32_t order,
                                 int64_t *out_trace) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  const uint32_t R = c->repetitions;
  if (R && !chain_betas) return asp::set_error(ASP_ERR_INVALID, "null chain_betas");
  if (order > 1u) return asp::set_error(ASP_ERR_INVALID, "order must be 0 (colour) or 1 (shuffled)");
  if (static_cast<uint64_t>(c->sweeps_done) + num_sweeps > 0xFFFFFFFEull) {
    return asp::set_error(ASP_ERR_INVALID, "%u sweeps after %u exceed the 2^32 - 2 sweep indices of a chain",
                          num_sweeps, c->sweeps_done);
  }
  for (uint32_t r = 0; r < R; ++r) {
    // (an infinite beta times dE = 0 is not a number: the law needs a finite one)
    if (!(chain_betas[r] >= 0.0) || std::isinf(chain_betas[r])) {
      return asp::set_error(ASP_ERR_INVALID, "chain_betas[%u] is not a finite number >= 0", r);
    }
  }
  ASP_TRY(asp::bind_device());
  const std::vector<int64_t> start = c->h_e_cur;  // entry 0 of every row: NOT reset to 0
  if (num_sweeps != 0 && !nothing_to_run(c)) {
    c->plan->last_sweep_ms = c->plan->last_total_ms = 0.0f;
    ASP_TRY(order == 0 ? asp::sa_chains_advance_ladder_colour(c, chain_betas, num_sweeps, out_trace)
                       : asp::sa_chains_advance_ladder_shuffled(c, chain_betas, num_sweeps, out_trace));
  } else if (out_trace) {
    // (no spins: the energy stays where it is; no sweeps: the single entry below)
    for (uint64_t k = 0; k < static_cast<uint64_t>(R) * (num_sweeps + 1ull); ++k) out_trace[k] = 0;
  }
  if (out_trace) {
    for (uint32_t r = 0; r < R; ++r) out_trace[static_cast<uint64_t>(r) * (num_sweeps + 1ull)] = start[r];
  }
  c->sweeps_done += num_sweeps;
  return ASP_OK;
}

float asp_sa_chains_batch_last_ms(void) { return g_chains_batch_ms; }

int asp_sa_chains_advance_batch(asp_sa_chains_item const *items, uint32_t count) {
  asp_clear_error();
  g_chains_batch_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before any device work and before any output is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_item &it = items[i];
    if (!it.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    if (it.num_sweeps && !it.betas) return asp::set_error(ASP_ERR_INVALID, "item %u: null betas", i);
    if (it.order > 1u) return asp::set_error(ASP_ERR_INVALID, "item %u: order must be 0 (colour) or 1 (shuffled)", i);
    if (it.flags != 0) return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    if (static_cast<uint64_t>(it.chains->sweeps_done) + it.num_sweeps > 0xFFFFFFFEull) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: %u sweeps after %u exceed the 2^32 - 2 sweep indices of a chain",
                            i, it.num_sweeps, it.chains->sweeps_done);
    }
    for (uint32_t t = 0; t < it.num_sweeps; ++t) {
      if (!(it.betas[t] >= 0.0)) return asp::set_error(ASP_ERR_INVALID, "item %u: betas[%u] is not >= 0", i, t);
    }
  }
  std::vector<BatchSegment> segments(count);
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_item &it = items[i];
    segments[i] = BatchSegment{it.chains,    it.betas,         nullptr, it.num_sweeps, it.order,
                               it.out_trace, it.out_tracked_best, it.out_improved};
  }
  ASP_TRY(check_distinct_plans(segments));
  return run_batch_segments(segments);
}

int asp_sa_chains_advance_ladder_batch(asp_sa_chains_ladder_item const *items, uint32_t count) {
  asp_clear_error();
  g_chains_batch_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before any device work and before any output is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_ladder_item &it = items[i];
    if (!it.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    const uint32_t R = it.chains->repetitions;
    if (R && !it.chain_betas) return asp::set_error(ASP_ERR_INVALID, "item %u: null chain_betas", i);
    if (it.order > 1u) return asp::set_error(ASP_ERR_INVALID, "item %u: order must be 0 (colour) or 1 (shuffled)", i);
    if (it.flags != 0) return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    if (static_cast<uint64_t>(it.chains->sweeps_done) + it.num_sweeps > 0xFFFFFFFEull) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: %u sweeps after %u exceed the 2^32 - 2 sweep indices of a chain",
                            i, it.num_sweeps, it.chains->sweeps_done);
    }
    for (uint32_t r = 0; r < R; ++r) {
      // (an infinite beta times dE = 0 is not a number: the law needs a finite one)
      if (!(it.chain_betas[r] >= 0.0) || std::isinf(it.chain_betas[r])) {
        return asp::set_error(ASP_ERR_INVALID, "item %u: chain_betas[%u] is not a finite number >= 0", i, r);
      }
    }
  }
  std::vector<BatchSegment> segments(count);
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_ladder_item &it = items[i];
    segments[i] = BatchSegment{it.chains,    nullptr,          it.chain_betas, it.num_sweeps, it.order,
                               it.out_trace, it.out_tracked_best, it.out_improved};
  }
  ASP_TRY(check_distinct_plans(segments));
  return run_batch_segments(segments);
}

int asp_sa_chains_result(asp_sa_chains *c, uint64_t *out_x, double *out_e) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (c->repetitions == 0) return ASP_OK;
  if (!out_x || !out_e) return asp::set_error(ASP_ERR_INVALID, "null argument");
  asp_sa_plan *p = c->plan;
  const uint32_t R = c->repetitions;
  if (p->host.num_spins == 0) {
    for (uint32_t r = 0; r < R; ++r) out_e[r] = 0.0;
    return ASP_OK;
  }
  ASP_TRY(asp::bind_device());
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);
  // the closed calls' report: the energy recomputed from the configuration
  ASP_TRY(p->w_x0_perm.ensure(static_cast<uint64_t>(R) * p->host.num_blocks));
  ASP_TRY(p->w_partial.ensure(static_cast<uint64_t>(R) * p->host.num_blocks));
  ASP_TRY(p->w_e.ensure(R));
  ASP_TRY(asp::sa_permute_bits(p, c->x_best.ptr, R, p->w_x0_perm.ptr));
  ASP_TRY(asp::sa_energies_of_perm(p, p->w_x0_perm.ptr, R, p->w_partial.ptr, p->w_e.ptr));
  ASP_HIP_TRY(hipMemcpyAsync(out_x, c->x_best.ptr, static_cast<uint64_t>(R) * c->words * 8, hipMemcpyDefault, s));
  ASP_HIP_TRY(hipMemcpyAsync(out_e, p->w_e.ptr, R * sizeof(double), hipMemcpyDefault, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  return ASP_OK;
}

int asp_sa_chains_export(asp_sa_chains *c, asp_sa_chains_snapshot *snap) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (!snap) return asp::set_error(ASP_ERR_INVALID, "null snapshot");
  snap->sweeps_done = c->sweeps_done;
  const uint64_t R = c->repetitions, state_words = R * c->words;
  if (R == 0 || !(snap->x_current || snap->x_best || snap->tracked_current || snap->tracked_best || snap->accepted)) {
    return ASP_OK;
  }
  ASP_TRY(asp::bind_device());
  hipStream_t s = c->plan->stream;
  asp::StreamFence fence(s);
  if (snap->x_current && state_words) ASP_TRY(c->x_cur.download(snap->x_current, state_words, s));
  if (snap->x_best && state_words) ASP_TRY(c->x_best.download(snap->x_best, state_words, s));
  if (snap->tracked_current) {
    ASP_TRY(c->e_cur.download(reinterpret_cast<long long *>(snap->tracked_current), R, s));
  }
  if (snap->tracked_best) ASP_TRY(c->e_best.download(reinterpret_cast<long long *>(snap->tracked_best), R, s));
  if (snap->accepted) ASP_TRY(c->accepted.download(reinterpret_cast<unsigned long long *>(snap->accepted), R, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  return ASP_OK;
}

int asp_sa_chains_import(asp_sa_chains *c, asp_sa_chains_snapshot const *snap) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (!snap) return asp::set_error(ASP_ERR_INVALID, "null snapshot");
  if (!snap->x_current || !snap->x_best || !snap->tracked_current || !snap->tracked_best || !snap->accepted) {
    return asp::set_error(ASP_ERR_INVALID, "a snapshot to import needs all five arrays");
  }
  if (snap->sweeps_done > 0xFFFFFFFEu) {
    return asp::set_error(ASP_ERR_INVALID, "sweeps_done 2^32 - 1 is not a number of sweeps (the index is reserved)");
  }
  const uint64_t R = c->repetitions, state_words = R * c->words;
  if (R != 0) {
    ASP_TRY(asp::bind_device());
    hipStream_t s = c->plan->stream;
    asp::StreamFence fence(s);
    const uint64_t K = c->plan->host.num_spins;
    const std::vector<uint64_t> cur = staged(snap->x_current, c->words, c->repetitions, c->words, K);
    const std::vector<uint64_t> best = staged(snap->x_best, c->words, c->repetitions, c->words, K);
    if (state_words) {
      ASP_TRY(c->x_cur.upload(cur.data(), state_words, s));
      ASP_TRY(c->x_best.upload(best.data(), state_words, s));
    }
    ASP_TRY(c->e_cur.upload(reinterpret_cast<long long const *>(snap->tracked_current), R, s));
    ASP_TRY(c->e_best.upload(reinterpret_cast<long long const *>(snap->tracked_best), R, s));
    ASP_TRY(c->accepted.upload(reinterpret_cast<unsigned long long const *>(snap->accepted), R, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(c->h_e_cur.data(), snap->tracked_current, R * sizeof(int64_t));
  }
  c->sweeps_done = snap->sweeps_done;
  return ASP_OK;
}

}  // extern "C"
