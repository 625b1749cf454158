// The colour-order annealer's host side for ONE plan: the plan object and its setters, the closed calls
// (asp_sa_anneal, asp_sa_anneal_trace; run_chains, with the team launch, its mutex and its watchdog
// counters), one segment of a handle (sa_chains_advance_colour, _ladder_colour) and the greedy solver's
// relaxation.  Host code only: no kernel is defined here.  Which kernel runs in which shape is decided in
// csrc/sa_sweep.hip, which hands the kernel over as a pointer; the pass after the sweeps is
// csrc/sa_energy.hip's (prototypes of both: sa_colour.hpp).  A change here leaves the sweep kernels'
// source-set fingerprint alone.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

#include "asp_common.hpp"
#include "greedy.hpp"
#include "sa_colour.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

namespace {

using asp::upload_vector;
using namespace asp::colour;

// team launches of the process that the barrier's watchdog cut short (asp_sa_team_watchdog_trips)
std::atomic<uint64_t> g_team_watchdog_trips{0};

// Barrier polls before the watchdog gives up and the call is repeated without teams: ~ 5 s (a
// barrier normally completes in ~ 5 us; members can only be kept waiting by other kernels
// holding compute units — team launches themselves take turns).
constexpr uint32_t kTeamSpinLimit = 1u << 22;

}  // namespace

namespace asp {

int sa_plan_device_setup(asp_sa_plan *p) {
  const SaHostLayout &L = p->host;
  bool ok = stream_acquire(&p->stream) == ASP_OK;
  for (auto &e : p->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok) set_error(ASP_ERR_HIP, "could not create HIP stream/events");
  int num_cus = 0;
  size_t max_lds = 0;
  if (ok && device_limits(&num_cus, &max_lds) == ASP_OK) {
    p->num_cus = num_cus;
    p->max_lds = max_lds;
  }
  ok = ok && upload_vector(p->color_block_start, L.color_block_start, p->stream) == ASP_OK &&
       upload_vector(p->block_width, L.block_width, p->stream) == ASP_OK &&
       upload_vector(p->ell_off, L.ell_off, p->stream) == ASP_OK &&
       upload_vector(p->ell_col, L.ell_col, p->stream) == ASP_OK &&
       upload_vector(p->ell_val, L.ell_val, p->stream) == ASP_OK &&
       upload_vector(p->spin_of_pos, L.spin_of_pos, p->stream) == ASP_OK &&
       upload_vector(p->pos_of_spin, L.pos_of_spin, p->stream) == ASP_OK &&
       upload_vector(p->field_pos, L.field_pos, p->stream) == ASP_OK;
  if (ok && sweep_lds_bytes(L, kWide) <= p->max_lds) {
    std::vector<uint32_t> scaled(L.ell_col.size());
    for (size_t i = 0; i < scaled.size(); ++i) scaled[i] = L.ell_col[i] * 4u;
    ok = upload_vector(p->ell_col4, scaled, p->stream) == ASP_OK &&
         hipStreamSynchronize(p->stream) == hipSuccess;  // `scaled` dies with this scope
  }
  if (ok && hipStreamSynchronize(p->stream) != hipSuccess) {
    set_error(ASP_ERR_HIP, "plan upload failed");
    ok = false;
  }
  if (ok) return ASP_OK;
  if (error_state().code == ASP_OK) set_error(ASP_ERR_HIP, "plan upload failed");
  return error_state().code;
}

}  // namespace asp

extern "C" {

asp_sa_plan *asp_sa_plan_create(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                                double const *data, double const *field) {
  asp_clear_error();
  if (asp::require_device() != ASP_OK) return nullptr;
  asp_sa_plan *p = new (std::nothrow) asp_sa_plan();
  if (!p) {
    asp::set_error(ASP_ERR_ALLOC, "out of host memory");
    return nullptr;
  }
  if (asp::build_sa_layout(num_spins, indptr, indices, data, field, &p->host) != ASP_OK) {
    delete p;
    return nullptr;
  }
  p->pattern = std::make_shared<asp::SaPattern>();
  if (num_spins > 0) {
    // the pattern, for asp_sa_plan_reweight to compare with (validated above)
    p->pattern->nnz = static_cast<uint64_t>(indptr[num_spins]);
    p->pattern->indptr.assign(indptr, indptr + num_spins + 1);
    p->pattern->indices.assign(indices, indices + p->pattern->nnz);
  }
  // ASP_SA_TEAM=0: no team sweeps in this process — several processes share the device (worker
  // processes or ranks of the pipeline on one GPU), and a team launch needs all its workgroups
  // resident together, which another process's kernels can prevent (the watchdog then costs
  // seconds before the rerun without teams)
  if (const char *env = std::getenv("ASP_SA_TEAM")) {
    const int team = std::atoi(env);
    if (team == 0 || team == 2 || team == 4 || team == 8) p->team_mode = team;
  }
  if (asp::sa_plan_device_setup(p) != ASP_OK) {
    asp_sa_plan_destroy(p);
    return nullptr;
  }
  return p;
}

void asp_sa_plan_destroy(asp_sa_plan *p) {
  if (!p) return;
  for (auto &e : p->ev) {
    if (e) (void)hipEventDestroy(e);
  }
  if (p->stream) {
    (void)hipStreamSynchronize(p->stream);  // idle before it is recycled
    asp::stream_release(p->stream);
  }
  delete p;
}

int asp_sa_plan_info(asp_sa_plan const *p, asp_sa_info *info) {
  if (!p || !info) return asp::set_error(ASP_ERR_INVALID, "null argument");
  const asp::SaHostLayout &L = p->host;
  info->num_spins = L.num_spins;
  info->nnz_offdiag = L.a_col.size();
  info->ell_entries = L.ell_off.back() * 64;
  info->num_colors = L.num_colors;
  info->num_blocks = L.num_blocks;
  info->max_degree = L.max_degree;
  info->energy_scale_exp = L.energy_scale_exp;
  info->diag_sum = L.diag_sum;
  info->beta0_auto = L.beta0_auto;
  info->beta1_auto = L.beta1_auto;
  return ASP_OK;
}

int asp_sa_set_launch(asp_sa_plan *p, int replicas_per_group, int threads) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (replicas_per_group != 0 && !colour_form_listed(replicas_per_group, kBytes)) {
    return asp::set_error(ASP_ERR_INVALID, "replicas_per_group must be 0, 1, 2, 4 or 8");
  }
  if (threads != 0 && (threads < 64 || threads > 1024 || threads % 64 != 0)) {
    return asp::set_error(ASP_ERR_INVALID, "threads must be 0 or a multiple of 64 in [64, 1024]");
  }
  p->force_m = replicas_per_group;
  p->force_threads = threads;
  return ASP_OK;
}

int asp_sa_set_field_cache(asp_sa_plan *p, int enable) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->use_field_cache = enable != 0;
  return ASP_OK;
}

int asp_sa_set_tail(asp_sa_plan *p, int n) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (n < -1) return asp::set_error(ASP_ERR_INVALID, "n must be -1 (auto), 0 (off) or a number of flips");
  p->tail_mode = n;
  return ASP_OK;
}

int asp_sa_last_tail(asp_sa_plan const *p, uint32_t *sweeps_min, uint32_t *sweeps_max, uint32_t *entries_max) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  uint32_t lo = p->last_tail.empty() ? 0u : 0xFFFFFFFFu, hi = 0, entries = 0;
  for (size_t g = 0; g + 1 < p->last_tail.size(); g += 2) {
    lo = std::min(lo, p->last_tail[g]);
    hi = std::max(hi, p->last_tail[g]);
    entries = std::max(entries, p->last_tail[g + 1]);
  }
  if (sweeps_min) *sweeps_min = lo;
  if (sweeps_max) *sweeps_max = hi;
  if (entries_max) *entries_max = entries;
  return ASP_OK;
}

int asp_sa_set_post(asp_sa_plan *p, int enable) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->use_post = enable != 0;
  return ASP_OK;
}

int asp_sa_team_watchdog_trips(asp_sa_plan const *p, uint32_t *of_plan, uint64_t *of_process) {
  if (of_plan) *of_plan = p ? p->team_watchdog_trips : 0u;
  if (of_process) *of_process = g_team_watchdog_trips.load(std::memory_order_relaxed);
  return ASP_OK;
}

int asp_sa_set_team(asp_sa_plan *p, int team) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (team != -1 && team != 0 && team != 2 && team != 4 && team != 8) {
    return asp::set_error(ASP_ERR_INVALID, "team must be -1 (auto), 0 (off), 2, 4 or 8");
  }
  p->team_mode = team;
  return ASP_OK;
}

int asp_sa_set_wide(asp_sa_plan *p, int allow) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->allow_wide = allow != 0;
  return ASP_OK;
}

int asp_sa_last_layout(asp_sa_plan const *p) { return p ? p->last_layout : -1; }

int asp_sa_last_spin_layout(asp_sa_plan const *p) { return p ? p->last_spin_layout : -1; }

int asp_sa_set_lds_limit(asp_sa_plan *p, uint64_t bytes) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->spin_lds_limit = static_cast<size_t>(std::min<uint64_t>(bytes, p->max_lds));  // (0, or >= the device's: the device's)
  return ASP_OK;
}

int asp_sa_set_packed(asp_sa_plan *p, int packed) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->force_packed = packed < 0 ? 0 : (packed > 2 ? 2 : packed);
  return ASP_OK;
}

}  // extern "C"

namespace asp {
namespace colour {

int check_closed_call(const char *prefix, const void *out_x, const void *out_e, const double *betas,
                      uint32_t num_sweeps, uint32_t repetitions, uint32_t replica_offset, uint32_t flags,
                      uint32_t known_flags) {
  if (!out_x || !out_e || (num_sweeps && !betas)) {
    return set_error(ASP_ERR_INVALID, "%snull argument", prefix);
  }
  if (num_sweeps == 0xFFFFFFFFu) {
    return set_error(ASP_ERR_INVALID, "%snum_sweeps 2^32-1 is reserved", prefix);
  }
  if (flags & ~known_flags) return set_error(ASP_ERR_INVALID, "%sunknown flags 0x%x", prefix, flags);
  if (static_cast<uint64_t>(replica_offset) + repetitions + 8 > 0xFFFFFFFFull) {
    return set_error(ASP_ERR_INVALID, "%sreplica ids exceed 32 bits", prefix);
  }
  for (uint32_t t = 0; t < num_sweeps; ++t) {
    if (!(betas[t] >= 0.0)) return set_error(ASP_ERR_INVALID, "%sbetas[%u] is not >= 0", prefix, t);
  }
  return ASP_OK;
}

bool field_cache_fits(DeviceBuffer<double> &cache, uint64_t elems) {
  if (elems * sizeof(double) > (32ull << 30)) return false;
  if (cache.ensure(elems) == ASP_OK) return true;
  asp_clear_error();
  return false;
}

}  // namespace colour
}  // namespace asp

namespace {

// The field cache of `padded` chains (512 B per block and replica), when it fits comfortably in HBM.
void attach_field_cache(asp_sa_plan *p, uint64_t padded, SweepArgs *args) {
  const asp::SaHostLayout &L = p->host;
  if (field_cache_fits(p->w_field_cache, padded * L.num_blocks * 64ull)) {
    args->field_cache = p->w_field_cache.ptr;
    args->cache_enter_flips = cache_enter_flips_of(L);
  }
}

// One launch on the plan's stream with a workgroup per group of chains: what a closed call (run_chains)
// and a segment of a handle (chains_advance_colour) do alike.  The caller queues what is its own between
// these steps — its uploads, the start, ev[0], the pass after the sweeps, ev[3] and its copies.
struct ColourRun {
  asp_sa_plan *p;
  uint32_t repetitions, num_sweeps;
  int64_t *trace;  // HOST [repetitions][num_sweeps + 1] or nullptr
  int m = 1, threads = 64, layout = kBytes;
  size_t lds = 0;
  uint32_t groups = 0;
  uint64_t padded = 0;
  SweepArgs args{};
  bool tail = false;  // a k_sa_sweep_tail launch: no field cache

  int shape(const ColourLaunch &form, size_t lds_bytes) {
    m = form.m, threads = form.threads, layout = form.layout, lds = lds_bytes;
    if (lds > p->max_lds) {
      return asp::set_error(ASP_ERR_TOO_LARGE, "%zu B of LDS needed, %zu B available", lds, p->max_lds);
    }
    groups = (repetitions + m - 1) / m;
    padded = static_cast<uint64_t>(groups) * m;
    return ASP_OK;
  }
  // the work buffers every launch uses; `num_betas` values go up in w_betas
  int ensure_work(uint64_t num_betas) {
    if (layout == kGlobal) ASP_TRY(p->w_spins.ensure(static_cast<uint64_t>(groups) * p->host.num_blocks));
    ASP_TRY(p->w_betas.ensure(num_betas));
    ASP_TRY(p->w_best.ensure(padded * p->host.num_blocks));
    ASP_TRY(p->w_tracked.ensure(padded));
    return p->w_accepted.ensure(padded);
  }
  // the arguments, with the trace buffer and the field cache (both the byte and the wide layout)
  int fill(const double *betas, const uint64_t *x0_perm, uint64_t seed, uint32_t replica_first) {
    args = sweep_args(p, layout, betas, x0_perm, p->w_best.ptr, p->w_tracked.ptr, p->w_accepted.ptr, seed,
                      num_sweeps, replica_first);
    if (trace) {
      ASP_TRY(p->w_trace.ensure(padded * (static_cast<uint64_t>(num_sweeps) + 1)));
      args.trace = p->w_trace.ptr;
    }
    if (p->use_field_cache && !bit_packed(layout) && !tail) attach_field_cache(p, padded, &args);
    return ASP_OK;
  }
  // ev[1], kernel(args, extra...), ev[2]
  template <typename Kernel, typename... Extra>
  int launch(Kernel kernel, Extra... extra) {
    if (!kernel) return asp::set_error(ASP_ERR_INVALID, "no sweep kernel for %d chains per group", m);
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(kernel), lds));
    ASP_HIP_TRY(hipEventRecord(p->ev[1], p->stream));
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(threads), lds, p->stream, args, extra...);
    ASP_HIP_TRY(hipGetLastError());
    ASP_HIP_TRY(hipEventRecord(p->ev[2], p->stream));
    return ASP_OK;
  }
  // the trace rows behind the caller's copies, and the wait for everything queued
  int collect() {
    if (trace) {  // rows of the real chains come first
      ASP_HIP_TRY(hipMemcpyAsync(trace, p->w_trace.ptr,
                                 static_cast<uint64_t>(repetitions) * (num_sweeps + 1ull) * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, p->stream));
    }
    ASP_HIP_TRY(hipStreamSynchronize(p->stream));
    return ASP_OK;
  }
  // what asp_sa_last_launch / _last_layout / _last_*_ms report; ev[0] .. ev[3]: the caller's
  int record(int launch_layout) {
    p->last_m = m;
    p->last_layout = launch_layout;
    p->last_spin_layout = layout;
    p->last_threads = threads;
    p->last_groups = static_cast<int>(groups);
    ASP_HIP_TRY(hipEventElapsedTime(&p->last_sweep_ms, p->ev[1], p->ev[2]));
    ASP_HIP_TRY(hipEventElapsedTime(&p->last_total_ms, p->ev[0], p->ev[3]));
    return ASP_OK;
  }
};

// Two team kernels resident at the same time could each hold CUs the other is waiting for:
// team launches of one process take turns (from launch to completion).
std::mutex g_team_launches;

// The launch of a closed call (ev[0] .. ev[2] and the watchdog's read-back) with every chain spread over
// `team` workgroups; the caller holds g_team_launches.  *refused: the configuration cannot be launched.
int launch_team(ColourRun &run, uint32_t team, bool descent, bool *refused) {
  asp_sa_plan *p = run.p;
  const asp::SaHostLayout &L = p->host;
  const uint32_t repetitions = run.repetitions;
  hipStream_t s = p->stream;
  // wavefronts per member: the widest colour class split over the team, at most 16
  run.threads = static_cast<int>(std::min<uint32_t>(16u, (widest_color(L) + team - 1) / team)) * 64;
  if (p->use_field_cache) {
    // the team's "tracking" of untouched blocks uses the field cache's switch-over threshold
    run.args.cache_enter_flips = cache_enter_flips_of(L);
  }
  TeamArgs ta{};
  ta.s = run.args;
  ta.team_size = team;
  ta.num_teams = repetitions;
  ta.spin_limit = kTeamSpinLimit;
  if (const char *env = std::getenv("ASP_TEAM_SPIN_LIMIT")) {  // test hook: provoke the watchdog
    ta.spin_limit = static_cast<uint32_t>(std::strtoul(env, nullptr, 10));
  }
  const size_t head_bytes = static_cast<size_t>(repetitions) * 8 * 7 + 16;
  const size_t need = head_bytes + static_cast<size_t>(repetitions) * L.num_blocks * 8;
  if (need > p->team_area_bytes) {
    if (p->team_area) (void)hipFree(p->team_area);
    p->team_area = nullptr;
    p->team_area_bytes = 0;
    ASP_HIP_TRY(hipExtMallocWithFlags(&p->team_area, need, hipDeviceMallocFinegrained));
    p->team_area_bytes = need;
  }
  ASP_HIP_TRY(hipMemsetAsync(p->team_area, 0, head_bytes, s));
  uint8_t *area = static_cast<uint8_t *>(p->team_area);
  ta.arrivals = reinterpret_cast<unsigned long long *>(area);
  ta.sums = reinterpret_cast<long long *>(area + static_cast<size_t>(repetitions) * 8);
  ta.abort = reinterpret_cast<uint32_t *>(area + static_cast<size_t>(repetitions) * 8 * 7);
  ta.flips = reinterpret_cast<uint64_t *>(area + head_bytes);
  const TeamKernel team_kernel = team_kernel_of(descent);
  ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(team_kernel), run.lds));
  ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
  ASP_HIP_TRY(hipEventRecord(p->ev[1], s));
  // An ORDINARY launch: team * repetitions <= CUs workgroups, each fitting a CU by itself,
  // are all resident on an otherwise idle device, and the watchdog (with the rerun in run_chains)
  // covers a device that is not idle.  hipLaunchCooperativeKernel would check the same
  // occupancy bound, but a process that has used it once dies in the HIP runtime's exit
  // handler when rocprofv3 is attached (tools/exit_probe.hip: a 40-line program does;
  // profiles/r02_exit_probe.txt).
  hipLaunchKernelGGL(team_kernel, dim3(repetitions * team), dim3(run.threads), run.lds, s, ta);
  *refused = hipGetLastError() != hipSuccess;
  if (*refused) return ASP_OK;
  ASP_HIP_TRY(hipEventRecord(p->ev[2], s));
  ASP_HIP_TRY(hipMemcpyAsync(&p->team_abort_host, ta.abort, sizeof p->team_abort_host, hipMemcpyDeviceToHost, s));
  return ASP_OK;
}

}  // namespace

namespace asp {
namespace colour {

// All chains of one call; descent = strict-descent sweeps (greedy relaxation).
int run_chains(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
               uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0, bool descent,
               uint64_t *out_x, double *out_e, int64_t *out_trace) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  ASP_TRY(asp::bind_device());
  if (repetitions == 0) return ASP_OK;
  ASP_TRY(check_closed_call("", out_x, out_e, betas, num_sweeps, repetitions, replica_offset, 0, 0));
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  const uint32_t words = static_cast<uint32_t>((K + 63) / 64);
  p->last_sweep_ms = p->last_total_ms = 0.0f;
  if (K == 0) {
    for (uint32_t r = 0; r < repetitions; ++r) out_e[r] = 0.0;
    return ASP_OK;
  }
  ColourLaunch form = choose_colour_launch(p, repetitions, descent, out_trace != nullptr);
  const uint32_t team = choose_team(p, form, repetitions, out_trace != nullptr);
  if (team >= 2) form.m = 1, form.layout = kBits;
  ColourRun run{p, repetitions, num_sweeps, out_trace};
  // tail sweeps where the form has them and its LDS has the room: the form itself stays as chosen
  const TailKernel tail_kernel =
      team >= 2 ? nullptr : tail_kernel_of(p, form.m, form.threads, form.layout, descent, replica_offset);
  run.tail = tail_kernel != nullptr;
  ASP_TRY(run.shape(form, team >= 2 ? team_lds_bytes(L)
                                    : sweep_lds_bytes(L, form.layout, run.tail, form.threads)));
  hipStream_t s = p->stream;
  // every exit below, error or not, first waits for what was queued on the stream: copies into
  // the caller's buffers and kernels using the plan's work buffers never outlive the call
  asp::StreamFence fence(s);
  ASP_TRY(run.ensure_work(num_sweeps));
  ASP_TRY(p->w_partial.ensure(static_cast<uint64_t>(repetitions) * L.num_blocks));
  ASP_TRY(p->w_e.ensure(repetitions));
  ASP_TRY(p->w_x.ensure(static_cast<uint64_t>(repetitions) * words));
  ASP_TRY(p->w_betas.upload(betas, num_sweeps, s));
  ASP_HIP_TRY(hipMemsetAsync(p->w_accepted.ptr, 0, run.padded * sizeof(unsigned long long), s));
  if (x0) {
    ASP_TRY(p->w_x0.ensure(words));
    ASP_TRY(p->w_x0_perm.ensure(L.num_blocks));
    ASP_TRY(p->w_x0.upload(x0, words, s));
    ASP_TRY(asp::sa_permute_bits(p, p->w_x0.ptr, 1u, p->w_x0_perm.ptr));
  }
  ASP_TRY(run.fill(p->w_betas.ptr, x0 ? p->w_x0_perm.ptr : nullptr, seed, replica_offset));

  p->team_abort_host = 0;
  std::unique_lock<std::mutex> team_turn(g_team_launches, std::defer_lock);
  if (team >= 2) {
    team_turn.lock();
    bool refused = false;
    ASP_TRY(launch_team(run, team, descent, &refused));
    if (refused) {
      // the configuration cannot be launched: one workgroup per chain instead
      ASP_HIP_TRY(hipStreamSynchronize(s));
      team_turn.unlock();
      p->team_mode = 0;
      return run_chains(p, seed, betas, num_sweeps, repetitions, replica_offset, x0, descent, out_x,
                        out_e, out_trace);
    }
  } else if (run.tail) {
    ASP_TRY(p->w_tail.ensure(2ull * run.groups));
    ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
    const uint32_t enter = p->tail_mode > 0 ? static_cast<uint32_t>(p->tail_mode) : tail_enter_flips_of(L);
    ASP_TRY(run.launch(tail_kernel, TailArgs{enter, p->w_tail.ptr}));
  } else {
    ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
    ASP_TRY(run.launch(closed_kernel_of(run.m, descent, run.layout, replica_offset)));
  }
  p->last_tail.assign(run.tail ? 2ull * run.groups : 0, 0u);
  if (run.tail) {
    ASP_HIP_TRY(hipMemcpyAsync(p->last_tail.data(), p->w_tail.ptr, p->last_tail.size() * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s));
  }
  // the first `repetitions` rows of best_perm are the real replicas
  // ... their reported energies and, in the same pass, their configurations in original order
  ASP_TRY(energies_of_perm(p, p->w_best.ptr, repetitions, p->w_partial.ptr, p->w_e.ptr, p->w_x.ptr));
  ASP_HIP_TRY(hipEventRecord(p->ev[3], s));
  // hipMemcpyDefault: out_x / out_e may be host pointers (the usual call) or device pointers
  // (distributed.py hands over RCCL-ready tensors, so a gather needs no host round trip)
  ASP_HIP_TRY(hipMemcpyAsync(out_x, p->w_x.ptr, static_cast<uint64_t>(repetitions) * words * sizeof(uint64_t),
                             hipMemcpyDefault, s));
  ASP_HIP_TRY(hipMemcpyAsync(out_e, p->w_e.ptr, repetitions * sizeof(double), hipMemcpyDefault, s));
  p->last_tracked.assign(repetitions, 0);
  p->last_accepted.assign(repetitions, 0);
  ASP_HIP_TRY(hipMemcpyAsync(p->last_tracked.data(), p->w_tracked.ptr, repetitions * sizeof(int64_t),
                             hipMemcpyDeviceToHost, s));
  ASP_HIP_TRY(hipMemcpyAsync(p->last_accepted.data(), p->w_accepted.ptr,
                             repetitions * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  ASP_TRY(run.collect());
  if (p->team_abort_host != 0) {
    // The members of a team were not resident together (another process or a long kernel holding
    // compute units — the launch mutex only orders this process's team launches): the partial
    // results are discarded and the call is repeated with one workgroup per chain, the fallback
    // of a refused launch.  Teams stay off for this plan.
    if (team_turn.owns_lock()) team_turn.unlock();
    p->team_mode = 0;
    p->team_watchdog_trips += 1;
    g_team_watchdog_trips.fetch_add(1, std::memory_order_relaxed);
    return run_chains(p, seed, betas, num_sweeps, repetitions, replica_offset, x0, descent, out_x,
                      out_e, out_trace);
  }
  return run.record(team >= 2 ? 4 : run.layout);
}

}  // namespace colour
}  // namespace asp

namespace {

// One segment of a handle in the colour order: the handle's original-order configurations are
// permuted into the plan's block order (current and best, every chain its own), k_sa_sweep_resume
// runs the sweeps from the carried integers with sweep index base c->sweeps_done, and both
// configurations go back.  The launch is run_chains' minus teams: the same choice of chains per
// group and spin layout, honouring asp_sa_set_launch / _set_packed / _set_wide; asp_sa_set_team
// is ignored (a handle runs one workgroup per group of chains).  chain_betas: nullptr, or HOST
// [repetitions] — a ladder segment: `betas` unused, the kernel takes ResumeLadder in place of Resume and
// one beta per (padded) chain lies in w_betas.
int chains_advance_colour(asp_sa_chains *c, double const *betas, double const *chain_betas, uint32_t num_sweeps,
                          int64_t *trace) {
  asp_sa_plan *p = c->plan;
  const asp::SaHostLayout &L = p->host;
  const uint32_t repetitions = c->repetitions;
  const bool ladder = chain_betas != nullptr;
  const ColourLaunch form = choose_colour_launch(p, repetitions, false, trace != nullptr);
  ColourRun run{p, repetitions, num_sweeps, trace};
  ASP_TRY(run.shape(form, sweep_lds_bytes(L, form.layout)));
  const uint64_t padded = run.padded;
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);
  ASP_TRY(run.ensure_work(ladder ? padded : num_sweeps));
  ASP_TRY(p->w_cur_perm.ensure(padded * L.num_blocks));
  ASP_TRY(p->w_e_cur.ensure(padded));
  if (ladder) {
    ASP_TRY(p->w_betas.upload(chain_betas, repetitions, s));
  } else {
    ASP_TRY(p->w_betas.upload(betas, num_sweeps, s));
  }
  // (the chains padding the last group: all spins up, integers 0; their results are never read)
  if (padded > repetitions) {
    if (ladder) ASP_HIP_TRY(hipMemsetAsync(p->w_betas.ptr + repetitions, 0, (padded - repetitions) * 8, s));
    const uint64_t tail = (padded - repetitions) * L.num_blocks * sizeof(uint64_t);
    ASP_HIP_TRY(hipMemsetAsync(p->w_best.ptr + static_cast<uint64_t>(repetitions) * L.num_blocks, 0, tail, s));
    ASP_HIP_TRY(hipMemsetAsync(p->w_cur_perm.ptr + static_cast<uint64_t>(repetitions) * L.num_blocks, 0, tail, s));
    ASP_HIP_TRY(hipMemsetAsync(p->w_tracked.ptr + repetitions, 0, (padded - repetitions) * 8, s));
    ASP_HIP_TRY(hipMemsetAsync(p->w_accepted.ptr + repetitions, 0, (padded - repetitions) * 8, s));
    ASP_HIP_TRY(hipMemsetAsync(p->w_e_cur.ptr + repetitions, 0, (padded - repetitions) * 8, s));
  }
  ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
  ASP_HIP_TRY(hipMemcpyAsync(p->w_e_cur.ptr, c->e_cur.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_HIP_TRY(hipMemcpyAsync(p->w_tracked.ptr, c->e_best.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_HIP_TRY(hipMemcpyAsync(p->w_accepted.ptr, c->accepted.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_TRY(asp::sa_permute_bits(p, c->x_cur.ptr, repetitions, p->w_cur_perm.ptr));
  ASP_TRY(asp::sa_permute_bits(p, c->x_best.ptr, repetitions, p->w_best.ptr));

  // (a ladder segment never reads args.betas)
  ASP_TRY(run.fill(ladder ? nullptr : p->w_betas.ptr, nullptr, c->seed, c->replica_offset));
  if (ladder) {
    ASP_TRY(run.launch(segment_kernel_of<ResumeLadder>(run.m, run.layout),
                       ResumeLadder{p->w_cur_perm.ptr, p->w_e_cur.ptr, c->sweeps_done, p->w_betas.ptr}));
  } else {
    ASP_TRY(run.launch(segment_kernel_of<Resume>(run.m, run.layout),
                       Resume{p->w_cur_perm.ptr, p->w_e_cur.ptr, c->sweeps_done}));
  }
  ASP_TRY(unpermute_bits(p, p->w_cur_perm.ptr, repetitions, c->x_cur.ptr));
  ASP_TRY(unpermute_bits(p, p->w_best.ptr, repetitions, c->x_best.ptr));
  ASP_HIP_TRY(hipMemcpyAsync(c->e_cur.ptr, p->w_e_cur.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_HIP_TRY(hipMemcpyAsync(c->e_best.ptr, p->w_tracked.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_HIP_TRY(hipMemcpyAsync(c->accepted.ptr, p->w_accepted.ptr, repetitions * 8ull, hipMemcpyDeviceToDevice, s));
  ASP_HIP_TRY(hipEventRecord(p->ev[3], s));
  ASP_HIP_TRY(hipMemcpyAsync(c->h_e_cur.data(), p->w_e_cur.ptr, repetitions * 8ull, hipMemcpyDeviceToHost, s));
  ASP_TRY(run.collect());
  return run.record(run.layout);
}

}  // namespace

namespace asp {

int sa_chains_advance_colour(asp_sa_chains *c, double const *betas, uint32_t num_sweeps, int64_t *trace) {
  return chains_advance_colour(c, betas, nullptr, num_sweeps, trace);
}

int sa_chains_advance_ladder_colour(asp_sa_chains *c, double const *chain_betas, uint32_t num_sweeps,
                                    int64_t *trace) {
  return chains_advance_colour(c, nullptr, chain_betas, num_sweeps, trace);
}

}  // namespace asp

extern "C" {

int asp_sa_anneal(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
                  uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0,
                  uint64_t *out_x, double *out_e) {
  asp_clear_error();
  return run_chains(p, seed, betas, num_sweeps, repetitions, replica_offset, x0, false, out_x,
                    out_e);
}

int asp_sa_anneal_trace(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
                        uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0,
                        uint64_t *out_x, double *out_e, int64_t *out_trace) {
  asp_clear_error();
  if (!out_trace) return asp::set_error(ASP_ERR_INVALID, "null trace pointer");
  return run_chains(p, seed, betas, num_sweeps, repetitions, replica_offset, x0, false, out_x,
                    out_e, out_trace);
}

int asp_sa_greedy(asp_sa_plan *p, uint32_t max_sweeps, uint64_t *out_x, double *out_e,
                  uint32_t *out_sweeps) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (!out_x || !out_e) return asp::set_error(ASP_ERR_INVALID, "null argument");
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  const uint32_t words = static_cast<uint32_t>((K + 63) / 64);
  if (out_sweeps) *out_sweeps = 0;
  if (K == 0) {
    *out_e = 0.0;
    return ASP_OK;
  }
  // 1. strongest-coupling-first cluster merging: on the host (O(E log E)), or the same tree on the
  // device (asp_sa_set_greedy_tree, csrc/greedy_tree.hip)
  std::vector<uint64_t> x(words, 0);
  if (p->greedy_tree != 0) {
    ASP_TRY(asp::bind_device());
    const asp::GreedyTreeTarget target{p, nullptr, x.data()};
    float split_ms[3] = {0.0f, 0.0f, 0.0f};
    ASP_TRY(asp::greedy_tree_device(&target, 1, p->stream, split_ms));
    asp::greedy_tree_record_ms(split_ms, false);
  } else {
    ASP_TRY(asp::greedy_tree_signs(L, x.data()));
  }
  return greedy_relax(p, max_sweeps, x, out_x, out_e, out_sweeps, false);
}

}  // extern "C"

namespace asp {
namespace colour {

// The device half of asp_sa_greedy for a plan with K > 0; x: the tree's configuration (consumed).
// exact_sweeps (asp_sa_greedy_batch's items that run alone): *out_sweeps is t, the index of the
// first sweep that flipped nothing (or max_sweeps), as the shared launches report it, instead of
// the whole chunks performed.  The chunks only tell which one flipped last; that chunk is then
// replayed from its start one sweep at a time until the final configuration appears — a fixed
// point of the deterministic sweep, so the first sweep after it is the one that flips nothing.
int greedy_relax(asp_sa_plan *p, uint32_t max_sweeps, std::vector<uint64_t> &x, uint64_t *out_x,
                 double *out_e, uint32_t *out_sweeps, bool exact_sweeps) {
  const uint32_t words = static_cast<uint32_t>(x.size());
  // 2. strict-descent relaxation on the device, in chunks, until a chunk flips nothing
  constexpr uint32_t kChunk = 8;
  std::vector<double> zeros(kChunk, 0.0);
  std::vector<uint64_t> next(words, 0);
  uint32_t done = 0;
  double energy = 0.0;
  if (max_sweeps == 0) {
    ASP_TRY(asp_sa_energy(p, 1, x.data(), &energy));
  }
  const bool replay = exact_sweeps && out_sweeps != nullptr;
  std::vector<uint64_t> flipped_from;  // start of the last chunk that flipped something
  uint32_t flipped_at = 0, flipped_len = 0;
  while (done < max_sweeps) {
    const uint32_t chunk = std::min(kChunk, max_sweeps - done);
    ASP_TRY(run_chains(p, 0, zeros.data(), chunk, 1, 0, x.data(), true, next.data(), &energy));
    const bool still = p->last_accepted.empty() || p->last_accepted[0] == 0;
    if (replay && !still) {
      flipped_from = x;
      flipped_at = done;
      flipped_len = chunk;
    }
    done += chunk;
    x.swap(next);
    if (still) break;
  }
  std::copy(x.begin(), x.end(), out_x);
  *out_e = energy;
  if (out_sweeps) *out_sweeps = done;
  if (replay && max_sweeps != 0) {
    uint32_t t = 1;  // no chunk flipped: the tree's configuration is a local minimum
    if (!flipped_from.empty()) {
      uint32_t u = 0;
      double unused = 0.0;
      while (u < flipped_len) {
        ASP_TRY(run_chains(p, 0, zeros.data(), 1, 1, 0, flipped_from.data(), true, next.data(), &unused));
        ++u;
        if (next == x) break;
        flipped_from.swap(next);
      }
      t = std::min(max_sweeps, flipped_at + u + 1u);
    }
    *out_sweeps = t;
  }
  return ASP_OK;
}

}  // namespace colour
}  // namespace asp

extern "C" {

int asp_sa_last_stats(asp_sa_plan const *p, uint32_t count, int64_t *tracked, uint64_t *accepted) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (count != p->last_tracked.size()) {
    return asp::set_error(ASP_ERR_INVALID, "count does not match the last anneal call");
  }
  if (tracked) std::copy(p->last_tracked.begin(), p->last_tracked.end(), tracked);
  if (accepted) std::copy(p->last_accepted.begin(), p->last_accepted.end(), accepted);
  return ASP_OK;
}

int asp_sa_last_launch(asp_sa_plan const *p, int *replicas_per_group, int *threads, int *groups) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (replicas_per_group) *replicas_per_group = p->last_m;
  if (threads) *threads = p->last_threads;
  if (groups) *groups = p->last_groups;
  return ASP_OK;
}

float asp_sa_last_sweep_ms(asp_sa_plan const *p) { return p ? p->last_sweep_ms : 0.0f; }
float asp_sa_last_total_ms(asp_sa_plan const *p) { return p ? p->last_total_ms : 0.0f; }

}  // extern "C"
