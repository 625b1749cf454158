// The shared launches of the colour-order annealer: many problems (asp_sa_anneal_batch), many segments of
// handles (sa_chains_advance_colour_batch) and many greedy descents (asp_sa_greedy_batch) as the workgroups
// of a few launches, through ClassLauncher.  Host code only: no kernel is defined here.  The class rule and
// the kernels are csrc/sa_sweep.hip's (batch_kernel_of hands a kernel over as a pointer), the pass after
// the sweeps and the state permutes csrc/sa_energy.hip's, the items that run alone csrc/sa_anneal.hip's
// (prototypes: sa_colour.hpp).  A change here leaves the sweep kernels' source-set fingerprint alone.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <type_traits>
#include <utility>
#include <vector>

#include "asp_common.hpp"
#include "greedy.hpp"
#include "sa_colour.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

// ---------------------------------------------------------------------------
// Batched anneal: many problems, one launch per size class
// ---------------------------------------------------------------------------
// The reference's production job is 50 000 sampled clusters of 50-1000 states, extended twice,
// each solved with 64 chains x 5120 sweeps (Makefile:9,115-127,
// experiments/sampled_connected_components.py:764-767, common.py:236-239).  One such problem
// is 64 workgroups of one or two wavefronts that wait on L2 latency at every colour step: a
// launch per problem leaves > 90 % of the chip idle.  Here the groups of ALL problems of a batch
// are the workgroups of a few launches (one per wavefront count), so the chip holds hundreds
// of problems at once and the latency of one hides behind the others.

namespace {

using asp::DeviceBuffer;
using namespace asp::colour;

thread_local float g_batch_sweep_ms = 0.0f;

// ---- the shared launches of a batch ----
// What the three batched entry points below (closed anneals, segments of handles, greedy descents) do
// alike.  A member — a problem of `groups` workgroups taking about `work` each and `lds` bytes — belongs
// to a class of workgroup shape; a class is ONE launch of 8 * slots_per_xcd workgroups over its XCD-aware
// slot table [8][slots_per_xcd] (asp::deal_to_xcds, x-major: the kernels read
// slots[(b & 7) * slots_per_xcd + (b >> 3)]), on a stream of its own so that the classes share the chip.
struct ClassMember {
  int cls;
  double work;
  uint32_t groups;
  size_t lds;
};
struct ClassLaunch {
  uint64_t slot_at = 0;
  uint32_t slots_per_xcd = 0;
  size_t lds = 0;  // the largest of its members
  bool used = false;
  hipEvent_t done = nullptr;  // recorded behind its launch
};
template <typename Problem>
struct ClassKernel {
  BatchKernel<Problem> kernel;
  uint32_t threads;
};

// Declared BEFORE the device buffers of an entry point (h_slots outlives the upload; the streams are
// waited for and released after the buffers' StreamFence).
struct ClassLauncher {
  std::vector<ClassLaunch> launches;
  std::vector<BatchSlot> h_slots;  // the classes' tables one after the other, for ONE upload
  // [class]; an array, destroyed in reverse: the streams go back to the pool last acquired first, so
  // every call leaves the pool — and with it the hardware queues of the next call's streams — as it was
  std::unique_ptr<asp::ScopedStream[]> streams;
  asp::EventPool events;
  hipEvent_t begin = nullptr, end = nullptr;  // on the main stream around the launches, with timing

  // The slot tables, and a stream and an event for every used class.
  int build(const std::vector<ClassMember> &members, int num_classes) {
    launches.assign(num_classes, ClassLaunch{});
    streams.reset(new asp::ScopedStream[num_classes]);
    for (int c = 0; c < num_classes; ++c) {
      std::vector<uint32_t> of_class;
      for (uint32_t k = 0; k < members.size(); ++k) {
        if (members[k].cls != c) continue;
        of_class.push_back(k);
        launches[c].lds = std::max(launches[c].lds, members[k].lds);
      }
      if (of_class.empty()) continue;
      std::vector<BatchSlot> per_xcd[asp::kXcds];
      launches[c].used = true;
      launches[c].slot_at = h_slots.size();
      launches[c].slots_per_xcd = asp::deal_to_xcds(
          of_class, [&](uint32_t k) { return members[k].work; }, [&](uint32_t k) { return members[k].groups; },
          per_xcd);
      for (auto &list : per_xcd) h_slots.insert(h_slots.end(), list.begin(), list.end());
      ASP_TRY(streams[c].acquire());
      ASP_TRY(events.make(&launches[c].done));
    }
    ASP_TRY(events.make(&begin, true));
    return events.make(&end, true);
  }

  // Every used class c: kernel_of(c).kernel({problems, its part of the uploaded slot table}) on the
  // class's stream, between `begin` and `end` on the main stream `s`, which waits for all of them.
  template <typename Problem, typename KernelOf>
  int run(hipStream_t s, const Problem *problems, const BatchSlot *d_slots, KernelOf kernel_of) {
    const int num_classes = static_cast<int>(launches.size());
    // (classes share kernels and run side by side: a kernel's dynamic-LDS limit is set once, to the
    // largest class that uses it, before the first launch)
    std::vector<std::pair<const void *, size_t>> kernel_lds;
    for (int c = 0; c < num_classes; ++c) {
      if (!launches[c].used) continue;
      const void *address = reinterpret_cast<const void *>(kernel_of(c).kernel);
      auto seen = std::find_if(kernel_lds.begin(), kernel_lds.end(), [&](auto &k) { return k.first == address; });
      if (seen == kernel_lds.end()) {
        kernel_lds.emplace_back(address, launches[c].lds);
      } else {
        seen->second = std::max(seen->second, launches[c].lds);
      }
    }
    for (auto &k : kernel_lds) ASP_TRY(asp::allow_dynamic_lds(k.first, k.second));
    const int rc = [&]() -> int {
      ASP_HIP_TRY(hipEventRecord(begin, s));
      for (int c = 0; c < num_classes; ++c) {
        const ClassLaunch &l = launches[c];
        if (!l.used) continue;
        const ClassKernel<Problem> k = kernel_of(c);
        hipStream_t cs = streams[c].stream;
        ASP_HIP_TRY(hipStreamWaitEvent(cs, begin, 0));
        hipLaunchKernelGGL(k.kernel, dim3(8u * l.slots_per_xcd), dim3(k.threads), l.lds, cs,
                           BatchArgs<Problem>{problems, d_slots + l.slot_at, l.slots_per_xcd});
        ASP_HIP_TRY(hipGetLastError());
        ASP_HIP_TRY(hipEventRecord(l.done, cs));
        ASP_HIP_TRY(hipStreamWaitEvent(s, l.done, 0));
      }
      ASP_HIP_TRY(hipEventRecord(end, s));
      return ASP_OK;
    }();
    if (rc != ASP_OK) {
      // the main stream may not have joined every class: wait for them here, so that the caller's
      // buffers, fenced on the main stream alone, do not go back to the pool under a running class
      for (int c = 0; c < num_classes; ++c) {
        if (launches[c].used) (void)hipStreamSynchronize(streams[c].stream);
      }
    }
    return rc;
  }
};

// What asp_sa_last_launch / _last_layout report of a problem that ran in a shared launch; its times are
// the batch's (asp_sa_batch_last_ms, asp_sa_chains_batch_last_ms, asp_sa_greedy_batch_last_ms).
void record_shared_launch(asp_sa_plan *p, int m, int layout, uint32_t waves, uint64_t groups) {
  p->last_m = m;
  p->last_layout = p->last_spin_layout = layout;
  p->last_threads = static_cast<int>(64u * waves);
  p->last_groups = static_cast<int>(groups);
  p->last_sweep_ms = p->last_total_ms = 0.0f;
}

}  // namespace

extern "C" {

float asp_sa_batch_last_ms(void) { return g_batch_sweep_ms; }

int asp_sa_batch_slots_host(uint32_t count, double const *work, uint32_t const *groups, uint32_t *slots_per_xcd,
                            uint32_t *slots, uint64_t capacity) {
  asp_clear_error();
  if (!slots_per_xcd || (count && (!work || !groups))) return asp::set_error(ASP_ERR_INVALID, "null argument");
  const auto too_small = [&] {
    return asp::set_error(ASP_ERR_INVALID, "the table does not fit %llu slots",
                          static_cast<unsigned long long>(slots ? capacity : 0));
  };
  // (the eight lists hold all groups between them: a table that cannot fit is refused before it is built)
  uint64_t all_groups = 0;
  for (uint32_t k = 0; k < count; ++k) all_groups += groups[k];
  if (all_groups > capacity) return too_small();
  std::vector<uint32_t> members(count);
  std::iota(members.begin(), members.end(), 0u);
  std::vector<BatchSlot> per_xcd[asp::kXcds];
  const uint32_t longest = asp::deal_to_xcds(
      members, [&](uint32_t k) { return work[k]; }, [&](uint32_t k) { return groups[k]; }, per_xcd);
  if (uint64_t{asp::kXcds} * longest > capacity || (longest && !slots)) return too_small();
  *slots_per_xcd = longest;
  for (const auto &list : per_xcd) {
    for (const BatchSlot &slot : list) {
      *slots++ = slot.problem;
      *slots++ = slot.group;
    }
  }
  return ASP_OK;
}

int asp_sa_anneal_batch(asp_sa_batch_item const *items, uint32_t count) {
  asp_clear_error();
  g_batch_sweep_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  ASP_TRY(asp::bind_device());
  // ---- validation (the checks of asp_sa_anneal, for every item before anything runs) ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_batch_item &it = items[i];
    if (!it.plan) return asp::set_error(ASP_ERR_INVALID, "item %u: null plan", i);
    if (it.repetitions == 0) continue;
    char prefix[24];
    std::snprintf(prefix, sizeof prefix, "item %u: ", i);
    ASP_TRY(check_closed_call(prefix, it.out_x, it.out_e, it.betas, it.num_sweeps, it.repetitions,
                              it.replica_offset, it.flags, ASP_SA_BATCH_SHUFFLED));
    for (uint32_t j = 0; j < i; ++j) {
      if (items[j].plan == it.plan && items[j].repetitions) {
        return asp::set_error(ASP_ERR_INVALID, "items %u and %u share a plan", j, i);
      }
    }
  }
  // ---- which items go into the shared launches ----
  // Problems whose spins need the bit-packed layouts, plans with a forced launch geometry
  // (tests, measurements) and a batch of one keep the single-problem path (team sweep included);
  // items asking for a fresh visiting order every sweep run concurrently on their plans' own
  // streams (csrc/sa_shuffled.hip).
  std::vector<BatchEntry> entries;
  std::vector<uint32_t> alone, shuffled;
  bool batch_bits = false, batch_nibbles = true;
  if (const char *env = std::getenv("ASP_BATCH_BITS")) batch_bits = std::atoi(env) != 0;  // tests, measurements
  if (const char *env = std::getenv("ASP_BATCH_NIBBLES")) batch_nibbles = std::atoi(env) != 0;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_batch_item &it = items[i];
    if (it.repetitions == 0) continue;
    if (it.flags & ASP_SA_BATCH_SHUFFLED) {
      shuffled.push_back(i);
      continue;
    }
    const asp_sa_plan *p = it.plan;
    const asp::SaHostLayout &L = p->host;
    // A byte per position must fit the LDS, or (up to ~2.4e5 spins) four bits per position with
    // four chains per workgroup.  Beyond that a chain would be one workgroup with a bit per
    // position: as a class of the shared launches it was measured and
    // LOSES against running those problems one after the other as team sweeps, every chain spread
    // over four CUs (a round of 64 clusters of the pipeline, largest model 157 706 spins: 5.9 s
    // against 4.05 s; ASP_BATCH_BITS=1 puts them into the shared launches all the same).
    const bool bytes_fit = L.num_spins > 0 && sweep_lds_bytes(L, kBytes) <= p->spin_lds();
    const bool nibbles_fit = L.num_spins > 0 && sweep_lds_bytes(L, kNibbles) <= p->spin_lds() && batch_nibbles;
    const bool bits_fit = L.num_spins > 0 && sweep_lds_bytes(L, kBits) <= p->spin_lds() && batch_bits;
    if (!(bytes_fit || nibbles_fit || bits_fit) || p->force_m || p->force_threads || p->force_packed) {
      alone.push_back(i);
      continue;
    }
    BatchEntry e{};
    e.item = i;
    e.chains = it.repetitions;
    // Layout and wavefronts per workgroup in a shared launch.  Small problems — several
    // workgroups fit a CU — take the word layout (one-instruction signs) and 4 wavefronts: small
    // workgroups interleave better than the 16 a lone problem wants (cap 16 / 8 / 4 on clusters of
    // 1e2..1e4 spins, 128 problems: 109 / 133 / 152 G flips/s, 512: 152 / 200 / 213).  Larger ones keep a byte per spin — the word layout would leave them
    // one workgroup per CU — and take 16 wavefronts (the sampled-cluster pipeline's order-2 models,
    // 1e4..2e5 spins, cap 4 / 8 / 16: 150 / 234 / 279 G flips/s; profiles/r03_batch_tune_real.txt).
    // (kBatchWideMax, kBatchSmallMax: both 10000)
    e.layout = !bytes_fit ? (nibbles_fit ? kNibbles : kBits) : batch_layout_in_lds(p);
    e.waves = batch_waves(L);
    e.work = static_cast<double>(it.num_sweeps) * static_cast<double>(L.ell_off.back() + L.num_blocks);
    entries.push_back(e);
  }
  if (entries.size() == 1) {
    alone.push_back(entries[0].item);
    entries.clear();
  }
  if (!shuffled.empty()) {
    ASP_TRY(asp::sa_shuffled_batch(items, shuffled.data(), static_cast<uint32_t>(shuffled.size()),
                                   &g_batch_sweep_ms));
  }
  for (uint32_t i : alone) {
    const asp_sa_batch_item &it = items[i];
    ASP_TRY(run_chains(it.plan, it.seed, it.betas, it.num_sweeps, it.repetitions, it.replica_offset,
                       nullptr, false, it.out_x, it.out_e));
    g_batch_sweep_ms += it.plan->last_sweep_ms;
  }
  if (entries.empty()) return ASP_OK;

  const asp_sa_plan *first = items[entries[0].item].plan;
  const int num_cus = first->num_cus;
  const size_t max_lds = first->max_lds;
  // ---- size classes: workgroups of one launch have one thread count ----
  // A launch class = (wavefront count, spin layout): kWaves[c / 4] wavefronts, layout c % 4.
  const auto &kWaves = kBatchWaves;
  static const int kLayouts[] = {kWide, kBytes, kBits, kNibbles};
  constexpr int kNumWaves = kNumBatchWaves;
  constexpr int kNumClasses = 4 * kNumWaves;
  auto class_of = [&](const BatchEntry &e) {
    const int w = batch_waves_index(e.waves);
    return 4 * w + (e.layout == kWide ? 0 : (e.layout == kBytes ? 1 : (e.layout == kBits ? 2 : 3)));
  };
  auto waves_of_class = [&](int c) { return kWaves[c / 4]; };
  auto layout_of_class = [&](int c) { return kLayouts[c % 4]; };
  // ---- replicas per workgroup, per class (batch_chains_per_group) ----
  int m_of_class[kNumClasses];
  {
    const int m = batch_chains_per_group(entries, num_cus);
    for (int c = 0; c < kNumClasses; ++c) m_of_class[c] = m;
    // (fewer replicas per workgroup for the classes of the largest problems, to shorten the
    // batch's longest workgroup, was measured and LOSES: 123 -> 97 G flips/s at 128 problems,
    // 157 -> 120 at 512; the word layout's efficiency outweighs the shorter tail)
    if (const char *env = std::getenv("ASP_BATCH_M")) {  // tuning aid
      const int forced = std::atoi(env);
      if (forced == 1 || forced == 2 || forced == 4 || forced == 8) {
        for (int c = 0; c < kNumClasses; ++c) m_of_class[c] = forced;
      }
    }
    for (int c = 0; c < kNumClasses; ++c) {
      if (layout_of_class(c) == kBits) m_of_class[c] = 1;  // a bit per position: one chain per workgroup
      if (layout_of_class(c) == kNibbles) m_of_class[c] = 4;
      // the word layout exists for four replicas: with another count its problems take bytes
    }
  }
  auto m_of = [&](const BatchEntry &e) { return m_of_class[class_of(e)]; };
  for (BatchEntry &e : entries) {
    if (e.layout == kWide && m_of(e) != 4) e.layout = kBytes;
  }
  // ---- per-problem buffer offsets ----
  struct Offsets {
    uint64_t best, stat, cache, partial, e, x, groups, padded;
  };
  std::vector<Offsets> off(entries.size());
  uint64_t n_best = 0, n_stat = 0, n_cache = 0, n_partial = 0, n_e = 0, n_x = 0, n_betas = 0;
  bool use_cache = true;
  for (size_t k = 0; k < entries.size(); ++k) {
    const asp_sa_batch_item &it = items[entries[k].item];
    const asp::SaHostLayout &L = it.plan->host;
    const uint64_t m = static_cast<uint64_t>(m_of(entries[k]));
    const uint64_t groups = (it.repetitions + m - 1) / m, padded = groups * m;
    const uint64_t words = (L.num_spins + 63) / 64;
    off[k] = Offsets{n_best, n_stat, n_cache, n_partial, n_e, n_x, groups, padded};
    n_best += padded * L.num_blocks;
    n_stat += padded;
    if (entries[k].layout != kBits) n_cache += padded * L.num_blocks * 64ull;
    n_partial += static_cast<uint64_t>(it.repetitions) * L.num_blocks;
    n_e += it.repetitions;
    n_x += static_cast<uint64_t>(it.repetitions) * words;
    entries[k].beta_at = n_betas;
    n_betas += it.num_sweeps;
    use_cache = use_cache && it.plan->use_field_cache;
  }

  asp::ScopedStream main_stream;
  ASP_TRY(main_stream.acquire());
  hipStream_t s = main_stream.stream;
  ClassLauncher launcher;
  DeviceBuffer<double> d_betas, d_partial, d_e, d_cache;
  DeviceBuffer<uint64_t> d_best, d_x;
  DeviceBuffer<long long> d_tracked;
  DeviceBuffer<unsigned long long> d_accepted;
  DeviceBuffer<SweepArgs> d_problems;
  DeviceBuffer<PostProblem> d_post;
  DeviceBuffer<BatchSlot> d_slots, d_chains;
  asp::StreamFence fence(s);
  ASP_TRY(d_betas.alloc(n_betas));
  ASP_TRY(d_best.alloc(n_best));
  ASP_TRY(d_tracked.alloc(n_stat));
  ASP_TRY(d_accepted.alloc(n_stat));
  ASP_TRY(d_partial.alloc(n_partial));
  ASP_TRY(d_e.alloc(n_e));
  ASP_TRY(d_x.alloc(n_x));
  use_cache = use_cache && field_cache_fits(d_cache, n_cache);
  // ---- descriptors ----
  std::vector<double> h_betas(n_betas);
  std::vector<SweepArgs> h_problems(entries.size());
  std::vector<PostProblem> h_post(entries.size());
  std::vector<BatchSlot> h_chains;
  std::vector<ClassMember> members(entries.size());
  h_chains.reserve(n_e);
  size_t energy_lds = 0;
  for (size_t k = 0; k < entries.size(); ++k) {
    const asp_sa_batch_item &it = items[entries[k].item];
    const asp_sa_plan *p = it.plan;
    const asp::SaHostLayout &L = p->host;
    const bool packed = entries[k].layout == kBits;
    std::copy(it.betas, it.betas + it.num_sweeps, h_betas.begin() + entries[k].beta_at);
    // (of the plan's part only the couplings' columns depend on the layout here: kWide or not)
    SweepArgs a = sweep_args(p, entries[k].layout, d_betas.ptr + entries[k].beta_at, nullptr, d_best.ptr + off[k].best,
                             d_tracked.ptr + off[k].stat, d_accepted.ptr + off[k].stat, it.seed, it.num_sweeps,
                             it.replica_offset);
    // (the bit-packed layout runs without the field cache, as in the single-problem launch)
    a.field_cache = use_cache && !packed ? d_cache.ptr + off[k].cache : nullptr;
    a.cache_enter_flips = packed ? 0u : cache_enter_flips_of(L);
    h_problems[k] = a;
    h_post[k] = post_problem_of(p, d_best.ptr + off[k].best, d_partial.ptr + off[k].partial, d_e.ptr + off[k].e,
                                d_x.ptr + off[k].x);
    for (uint32_t r = 0; r < it.repetitions; ++r) {
      h_chains.push_back(BatchSlot{static_cast<uint32_t>(k), r});
    }
    energy_lds = std::max(energy_lds, static_cast<size_t>(L.num_blocks) * sizeof(uint64_t));
    const int c = class_of(entries[k]);
    members[k] = ClassMember{c, entries[k].work, static_cast<uint32_t>(off[k].groups),
                             sweep_lds_bytes(L, layout_of_class(c))};
  }
  // ---- slot tables: per class, problems longest first, dealt to the 8 XCDs ----
  ASP_TRY(launcher.build(members, kNumClasses));
  const std::vector<BatchSlot> &h_slots = launcher.h_slots;
  ASP_TRY(d_problems.alloc(h_problems.size()));
  ASP_TRY(d_post.alloc(h_post.size()));
  ASP_TRY(d_slots.alloc(h_slots.size()));
  ASP_TRY(d_chains.alloc(h_chains.size()));
  ASP_TRY(d_betas.upload(h_betas.data(), h_betas.size(), s));
  ASP_TRY(d_problems.upload(h_problems.data(), h_problems.size(), s));
  ASP_TRY(d_post.upload(h_post.data(), h_post.size(), s));
  ASP_TRY(d_slots.upload(h_slots.data(), h_slots.size(), s));
  ASP_TRY(d_chains.upload(h_chains.data(), h_chains.size(), s));
  ASP_HIP_TRY(hipMemsetAsync(d_accepted.ptr, 0, n_stat * sizeof(unsigned long long), s));
  // ---- one sweep launch per class ----
  ASP_TRY(launcher.run(s, d_problems.ptr, d_slots.ptr, [&](int c) {
    // (a class of words has four chains per workgroup: with another count its problems took bytes)
    return ClassKernel<SweepArgs>{batch_kernel_of<SweepArgs>(m_of_class[c], layout_of_class(c)),
                                  64u * waves_of_class(c)};
  }));
  // ---- energies and original-order bits of every chain's best configuration ----
  ASP_TRY(launch_post_batch(d_post.ptr, d_chains.ptr, static_cast<unsigned>(h_chains.size()), energy_lds, max_lds,
                            s));
  std::vector<uint64_t> h_x(n_x);
  std::vector<double> h_e(n_e);
  std::vector<long long> h_tracked(n_stat);
  std::vector<unsigned long long> h_accepted(n_stat);
  ASP_TRY(d_x.download(h_x.data(), n_x, s));
  ASP_TRY(d_e.download(h_e.data(), n_e, s));
  ASP_TRY(d_tracked.download(h_tracked.data(), n_stat, s));
  ASP_TRY(d_accepted.download(h_accepted.data(), n_stat, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&ms, launcher.begin, launcher.end));
  g_batch_sweep_ms += ms;
  for (size_t k = 0; k < entries.size(); ++k) {
    const asp_sa_batch_item &it = items[entries[k].item];
    asp_sa_plan *p = it.plan;
    const uint64_t words = (p->host.num_spins + 63) / 64;
    std::copy(h_x.begin() + off[k].x, h_x.begin() + off[k].x + it.repetitions * words, it.out_x);
    std::copy(h_e.begin() + off[k].e, h_e.begin() + off[k].e + it.repetitions, it.out_e);
    p->last_tracked.assign(h_tracked.begin() + off[k].stat,
                           h_tracked.begin() + off[k].stat + it.repetitions);
    p->last_accepted.assign(h_accepted.begin() + off[k].stat,
                            h_accepted.begin() + off[k].stat + it.repetitions);
    const int c = class_of(entries[k]);
    record_shared_launch(p, m_of_class[c], layout_of_class(c), waves_of_class(c), off[k].groups);
  }
  return ASP_OK;
}

}  // extern "C"
// ---------------------------------------------------------------------------
// Batched segments of resumable chains, colour order (asp_sa_chains_advance_batch)
// ---------------------------------------------------------------------------
// The launch grouping of asp_sa_anneal_batch — one launch per wavefront count and layout class (a
// word or a byte per position), four or two chains per workgroup when that still fills the chip —
// with ResumeProblem descriptors in place of SweepArgs, and the handles' state permuted in and
// out by one launch each way.  Segments that need the bit-packed layouts, plans with a forced
// geometry or layout, traced segments and a group of one run as sa_chains_advance_colour.
// Two deliberate differences from the closed batch, whose helpers (kBatchWaves, batch_layout_in_lds,
// batch_waves) this shares: a cluster beyond a byte per position runs alone here even where four bits
// per position would fit (the nibble class has no resume form), and the closed batch's tuning aid
// ASP_BATCH_M is not read (chains per workgroup never change a result).

// A batch of LADDER segments (asp_sa_chains_advance_ladder_batch; every segment with chain_betas): the
// same grouping, class rule, LDS limit and state permute, with LadderProblem descriptors; the per-chain
// betas of all handles go up in the one concatenated buffer, every handle's part padded with zeros to
// whole groups; the segments that run alone take
// sa_chains_advance_ladder_colour.

namespace asp {

namespace {

using namespace colour;

template <bool LADDER>
int chains_advance_colour_batch(const ChainsSegment *segs, uint32_t count, float *sweep_ms) {
  using Problem = std::conditional_t<LADDER, LadderProblem, ResumeProblem>;
  std::vector<BatchEntry> entries;  // (item: index into segs)
  std::vector<uint32_t> alone;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_plan *p = segs[i].chains->plan;
    const SaHostLayout &L = p->host;
    const bool bytes_fit = sweep_lds_bytes(L, kBytes) <= p->spin_lds();
    if (segs[i].trace || !bytes_fit || p->force_m || p->force_threads || p->force_packed) {
      alone.push_back(i);
      continue;
    }
    // (layout and wavefronts per workgroup in a shared launch: asp_sa_anneal_batch's, measured there)
    BatchEntry e{};
    e.item = i;
    e.chains = segs[i].chains->repetitions;
    e.layout = batch_layout_in_lds(p);
    e.waves = batch_waves(L);
    e.work = static_cast<double>(segs[i].num_sweeps) * static_cast<double>(L.ell_off.back() + L.num_blocks);
    entries.push_back(e);
  }
  if (entries.size() == 1) {
    alone.push_back(entries[0].item);
    entries.clear();
  }
  for (uint32_t i : alone) {
    asp_sa_plan *p = segs[i].chains->plan;
    p->last_sweep_ms = p->last_total_ms = 0.0f;
    if constexpr (LADDER) {
      ASP_TRY(sa_chains_advance_ladder_colour(segs[i].chains, segs[i].chain_betas, segs[i].num_sweeps, segs[i].trace));
    } else {
      ASP_TRY(sa_chains_advance_colour(segs[i].chains, segs[i].betas, segs[i].num_sweeps, segs[i].trace));
    }
    if (sweep_ms) *sweep_ms += p->last_sweep_ms;
  }
  if (entries.empty()) return ASP_OK;

  const auto &kWaves = kBatchWaves;
  constexpr int kNumClasses = 2 * kNumBatchWaves;  // class = 2 * (index of the wavefront count) + (bytes ? 1 : 0)
  // chains per workgroup for the batch (asp_sa_anneal_batch's rule)
  const int m = batch_chains_per_group(entries, segs[entries[0].item].chains->plan->num_cus);
  for (BatchEntry &e : entries) {
    if (e.layout == kWide && m != 4) e.layout = kBytes;  // (the word layout exists for four chains)
  }
  auto class_of = [&](const BatchEntry &e) { return 2 * batch_waves_index(e.waves) + (e.layout == kWide ? 0 : 1); };
  // ---- per-handle offsets into the launch's buffers ----
  struct Offsets {
    uint64_t perm, stat, cache, groups, padded;
  };
  std::vector<Offsets> off(entries.size());
  uint64_t n_perm = 0, n_stat = 0, n_cache = 0, n_betas = 0, n_chains = 0;
  bool use_cache = true;
  for (size_t k = 0; k < entries.size(); ++k) {
    const asp_sa_chains *c = segs[entries[k].item].chains;
    const SaHostLayout &L = c->plan->host;
    const uint64_t groups = (c->repetitions + static_cast<uint64_t>(m) - 1) / m, padded = groups * m;
    off[k] = Offsets{n_perm, n_stat, n_cache, groups, padded};
    n_perm += padded * L.num_blocks;
    n_stat += padded;
    n_cache += padded * L.num_blocks * 64ull;
    n_chains += c->repetitions;
    entries[k].beta_at = n_betas;
    n_betas += LADDER ? padded : segs[entries[k].item].num_sweeps;  // (a ladder: one beta per padded chain)
    use_cache = use_cache && c->plan->use_field_cache;
  }

  ScopedStream main_stream;
  ASP_TRY(main_stream.acquire());
  hipStream_t s = main_stream.stream;
  ClassLauncher launcher;
  DeviceBuffer<double> d_betas, d_cache;
  DeviceBuffer<uint64_t> d_best, d_cur;
  DeviceBuffer<long long> d_tracked, d_e_cur;
  DeviceBuffer<unsigned long long> d_accepted;
  DeviceBuffer<Problem> d_problems;
  DeviceBuffer<ChainsIo> d_io;
  DeviceBuffer<BatchSlot> d_slots, d_chains_in, d_chains_out;
  StreamFence fence(s);
  ASP_TRY(d_betas.alloc(n_betas));
  ASP_TRY(d_best.alloc(n_perm));
  ASP_TRY(d_cur.alloc(n_perm));
  ASP_TRY(d_tracked.alloc(n_stat));
  ASP_TRY(d_e_cur.alloc(n_stat));
  ASP_TRY(d_accepted.alloc(n_stat));
  use_cache = use_cache && field_cache_fits(d_cache, n_cache);
  // ---- descriptors ----
  std::vector<double> h_betas(n_betas, 0.0);  // (a ladder: the chains padding a last group stay 0)
  std::vector<Problem> h_problems(entries.size());
  std::vector<ChainsIo> h_io(entries.size());
  std::vector<BatchSlot> h_chains_in, h_chains_out;
  std::vector<ClassMember> members(entries.size());
  h_chains_in.reserve(n_stat);
  h_chains_out.reserve(n_chains);
  for (size_t k = 0; k < entries.size(); ++k) {
    const ChainsSegment &seg = segs[entries[k].item];
    asp_sa_chains *c = seg.chains;
    const asp_sa_plan *p = c->plan;
    const SaHostLayout &L = p->host;
    if constexpr (LADDER) {
      std::copy(seg.chain_betas, seg.chain_betas + c->repetitions, h_betas.begin() + entries[k].beta_at);
    } else {
      std::copy(seg.betas, seg.betas + seg.num_sweeps, h_betas.begin() + entries[k].beta_at);
    }
    Problem rp{};
    // (a ladder segment never reads s.betas)
    rp.s = sweep_args(p, entries[k].layout, LADDER ? nullptr : d_betas.ptr + entries[k].beta_at, nullptr,
                      d_best.ptr + off[k].perm, d_tracked.ptr + off[k].stat, d_accepted.ptr + off[k].stat, c->seed,
                      seg.num_sweeps, c->replica_offset);
    rp.s.field_cache = use_cache ? d_cache.ptr + off[k].cache : nullptr;
    rp.s.cache_enter_flips = cache_enter_flips_of(L);
    if constexpr (LADDER) {
      rp.r = ResumeLadder{d_cur.ptr + off[k].perm, d_e_cur.ptr + off[k].stat, c->sweeps_done,
                          d_betas.ptr + entries[k].beta_at};
    } else {
      rp.r = Resume{d_cur.ptr + off[k].perm, d_e_cur.ptr + off[k].stat, c->sweeps_done};
    }
    h_problems[k] = rp;
    ChainsIo io{};
    io.x_cur = c->x_cur.ptr;
    io.x_best = c->x_best.ptr;
    io.e_cur = c->e_cur.ptr;
    io.e_best = c->e_best.ptr;
    io.accepted = c->accepted.ptr;
    io.cur_perm = rp.r.cur_perm;
    io.best_perm = rp.s.best_perm;
    io.w_e_cur = rp.r.e_cur;
    io.w_tracked = rp.s.tracked;
    io.w_accepted = rp.s.accepted;
    io.spin_of_pos = p->spin_of_pos.ptr;
    io.pos_of_spin = p->pos_of_spin.ptr;
    io.num_spins = L.num_spins;
    io.num_blocks = L.num_blocks;
    io.words = c->words;
    io.chains = c->repetitions;
    h_io[k] = io;
    for (uint32_t r = 0; r < off[k].padded; ++r) h_chains_in.push_back(BatchSlot{static_cast<uint32_t>(k), r});
    for (uint32_t r = 0; r < c->repetitions; ++r) h_chains_out.push_back(BatchSlot{static_cast<uint32_t>(k), r});
    const int cl = class_of(entries[k]);
    members[k] = ClassMember{cl, entries[k].work, static_cast<uint32_t>(off[k].groups),
                             sweep_lds_bytes(L, cl % 2 == 0 ? kWide : kBytes)};
  }
  // ---- slot tables: per class, handles longest first, dealt to the 8 XCDs ----
  ASP_TRY(launcher.build(members, kNumClasses));
  const std::vector<BatchSlot> &h_slots = launcher.h_slots;
  ASP_TRY(d_problems.alloc(h_problems.size()));
  ASP_TRY(d_io.alloc(h_io.size()));
  ASP_TRY(d_slots.alloc(h_slots.size()));
  ASP_TRY(d_chains_in.alloc(h_chains_in.size()));
  ASP_TRY(d_chains_out.alloc(h_chains_out.size()));
  ASP_TRY(d_betas.upload(h_betas.data(), h_betas.size(), s));
  ASP_TRY(d_problems.upload(h_problems.data(), h_problems.size(), s));
  ASP_TRY(d_io.upload(h_io.data(), h_io.size(), s));
  ASP_TRY(d_slots.upload(h_slots.data(), h_slots.size(), s));
  ASP_TRY(d_chains_in.upload(h_chains_in.data(), h_chains_in.size(), s));
  ASP_TRY(d_chains_out.upload(h_chains_out.data(), h_chains_out.size(), s));
  ASP_TRY(launch_chains_permute(d_io.ptr, d_chains_in.ptr, static_cast<unsigned>(h_chains_in.size()), s));
  // ---- one sweep launch per class ----
  ASP_TRY(launcher.run(s, d_problems.ptr, d_slots.ptr, [&](int cl) {
    return ClassKernel<Problem>{batch_kernel_of<Problem>(cl % 2 == 0 ? 4 : m, cl % 2 == 0 ? kWide : kBytes),
                                64u * kWaves[cl / 2]};
  }));
  // ---- the state back into the handles (after the attempt: the colour order has no retry) ----
  ASP_TRY(launch_chains_unpermute(d_io.ptr, d_chains_out.ptr, static_cast<unsigned>(h_chains_out.size()), s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&ms, launcher.begin, launcher.end));
  if (sweep_ms) *sweep_ms += ms;
  for (size_t k = 0; k < entries.size(); ++k) {
    asp_sa_plan *p = segs[entries[k].item].chains->plan;
    const int cl = class_of(entries[k]);
    record_shared_launch(p, m, cl % 2 == 0 ? kWide : kBytes, kWaves[cl / 2], off[k].groups);
  }
  return ASP_OK;
}

}  // namespace

int sa_chains_advance_colour_batch(const ChainsSegment *segs, uint32_t count, float *sweep_ms) {
  if (count != 0 && segs[0].chain_betas) return chains_advance_colour_batch<true>(segs, count, sweep_ms);
  return chains_advance_colour_batch<false>(segs, count, sweep_ms);
}

}  // namespace asp

// ---------------------------------------------------------------------------
// Batched greedy solve: many problems' descents in shared launches
// ---------------------------------------------------------------------------
// The reference's production job solves tens of thousands of sampled clusters, three models each,
// with sa.greedy_solve (Makefile:115-127, experiments/sampled_connected_components.py:696-751).
// asp_sa_greedy spends one workgroup, ~25 launches and a host round trip every 8 sweeps on each.
// Here the host trees of all items run on a small thread pool, their signs go up in ONE copy and
// are permuted by ONE launch, every problem is a workgroup of a few shared descent
// launches (one per wavefront count) that decides on the device when it has converged, and the
// energies, configurations and sweep counts come back in one copy each.

namespace {

thread_local float g_greedy_tree_ms = 0.0f, g_greedy_descent_ms = 0.0f;

}  // namespace

extern "C" {

int asp_sa_greedy_batch_last_ms(float *tree_ms, float *descent_ms) {
  if (tree_ms) *tree_ms = g_greedy_tree_ms;
  if (descent_ms) *descent_ms = g_greedy_descent_ms;
  return ASP_OK;
}

int asp_sa_greedy_batch(asp_sa_greedy_item const *items, uint32_t count) {
  asp_clear_error();
  g_greedy_tree_ms = g_greedy_descent_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before anything runs or is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_greedy_item &it = items[i];
    if (!it.plan) return asp::set_error(ASP_ERR_INVALID, "item %u: null plan", i);
    if (!it.out_x || !it.out_e) return asp::set_error(ASP_ERR_INVALID, "item %u: null output", i);
    if (it.flags != 0) return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
  }
  {
    std::vector<std::pair<const asp_sa_plan *, uint32_t>> plans(count);
    for (uint32_t i = 0; i < count; ++i) plans[i] = {items[i].plan, i};
    std::sort(plans.begin(), plans.end());
    for (uint32_t i = 1; i < count; ++i) {
      if (plans[i].first == plans[i - 1].first) {
        return asp::set_error(ASP_ERR_INVALID, "items %u and %u share a plan", plans[i - 1].second,
                              plans[i].second);
      }
    }
  }
  ASP_TRY(asp::bind_device());
  // ---- which items go into the shared launches ----
  // A byte per position must fit the LDS (up to ~1.3e5 spins); problems beyond that, plans with a
  // forced launch geometry, layout or team size, and a batch of one take asp_sa_greedy's device
  // half (team sweep included).  Results never depend on the path.
  std::vector<uint32_t> live, shared, alone;  // live: K > 0, in item order
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_greedy_item &it = items[i];
    const asp_sa_plan *p = it.plan;
    if (it.out_sweeps) *it.out_sweeps = 0;
    if (p->host.num_spins == 0) {
      *it.out_e = 0.0;
      continue;
    }
    live.push_back(i);
    const bool forced = p->force_m || p->force_threads || p->force_packed || p->team_mode >= 2;
    if (forced || sweep_lds_bytes(p->host, kBytes) > p->spin_lds()) {
      alone.push_back(i);
    } else {
      shared.push_back(i);
    }
  }
  if (shared.size() == 1) {
    alone.push_back(shared[0]);
    shared.clear();
  }
  if (live.empty()) return ASP_OK;
  // ---- the trees: the host trees of the live items that ask for them, on the pool (greedy.cpp); the
  // device trees (asp_sa_set_greedy_tree, csrc/greedy_tree.hip) of the items that run alone here, and
  // those of the shared launches below, straight into the buffer the state permute reads ----
  std::vector<uint64_t> tree_at(count, 0);  // offset of item i's words in h_x0
  uint64_t n_words = 0;
  for (uint32_t i : live) {
    tree_at[i] = n_words;
    n_words += (items[i].plan->host.num_spins + 63) / 64;
  }
  std::vector<uint64_t> h_x0(n_words, 0);
  {
    std::vector<const asp::SaHostLayout *> layouts;
    std::vector<uint64_t *> outs;
    for (uint32_t i : live) {
      if (items[i].plan->greedy_tree != 0) continue;
      layouts.push_back(&items[i].plan->host);
      outs.push_back(h_x0.data() + tree_at[i]);
    }
    if (!layouts.empty()) {
      const auto t0 = std::chrono::steady_clock::now();
      asp::greedy_tree_signs_many(layouts.data(), outs.data(), layouts.size());
      g_greedy_tree_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  bool device_trees_ran = false;
  {
    std::vector<asp::GreedyTreeTarget> targets;
    for (uint32_t i : alone) {
      if (items[i].plan->greedy_tree != 0) {
        targets.push_back(asp::GreedyTreeTarget{items[i].plan, nullptr, h_x0.data() + tree_at[i]});
      }
    }
    if (!targets.empty()) {
      asp::ScopedStream tree_stream;
      ASP_TRY(tree_stream.acquire());
      float split_ms[3] = {0.0f, 0.0f, 0.0f};
      ASP_TRY(asp::greedy_tree_device(targets.data(), static_cast<uint32_t>(targets.size()), tree_stream.stream,
                                      split_ms));
      asp::greedy_tree_record_ms(split_ms, false);
      device_trees_ran = true;
      g_greedy_tree_ms += split_ms[0] + split_ms[1] + split_ms[2];
    }
  }
  for (uint32_t i : alone) {
    const asp_sa_greedy_item &it = items[i];
    const uint64_t words = (it.plan->host.num_spins + 63) / 64;
    std::vector<uint64_t> x(h_x0.begin() + tree_at[i], h_x0.begin() + tree_at[i] + words);
    ASP_TRY(greedy_relax(it.plan, it.max_sweeps, x, it.out_x, it.out_e, it.out_sweeps, true));
    g_greedy_descent_ms += it.plan->last_sweep_ms;  // (the last chunk's; see asp_sa_greedy_batch_last_ms)
  }
  if (shared.empty()) return ASP_OK;

  // ---- launch classes: workgroups of one launch have one wavefront count (kBatchWaves) ----
  const size_t n = shared.size();
  struct Offsets {
    uint64_t blocks, cache, x;  // best / x0_perm / partial rows; field cache; packed words
  };
  std::vector<Offsets> off(n);
  std::vector<ClassMember> members(n);
  uint64_t n_blocks = 0, n_cache = 0, n_x = 0;
  size_t energy_lds = 0;
  bool use_cache = true;
  for (size_t k = 0; k < n; ++k) {
    const asp_sa_plan *p = items[shared[k]].plan;
    const asp::SaHostLayout &L = p->host;
    off[k] = Offsets{n_blocks, n_cache, n_x};
    n_blocks += L.num_blocks;
    n_cache += static_cast<uint64_t>(L.num_blocks) * 64ull;
    n_x += (L.num_spins + 63) / 64;
    // one wavefront per block of the widest colour class, at most 16: the single path's choice
    const uint32_t waves = std::min<uint32_t>(widest_color(L), 16u);
    // (every member is one workgroup: the dealing to the XCDs comes out round-robin)
    members[k] = ClassMember{batch_waves_index(waves), static_cast<double>(L.ell_off.back() + L.num_blocks), 1u,
                             sweep_lds_bytes(L, kBytes)};
    energy_lds = std::max(energy_lds, static_cast<size_t>(L.num_blocks) * sizeof(uint64_t));
    use_cache = use_cache && p->use_field_cache;
  }
  const size_t max_lds = items[shared[0]].plan->max_lds;

  // (host arrays of the asynchronous uploads first, so that they outlive the stream's work)
  std::vector<uint64_t> h_x0_shared(n_x);
  std::vector<DescentProblem> h_problems(n);
  std::vector<PostProblem> h_post(n);
  std::vector<BatchSlot> h_chains(n);
  std::vector<uint64_t> h_x(n_x);
  std::vector<double> h_e(n);
  std::vector<uint32_t> h_sweeps(n);
  asp::ScopedStream main_stream;
  ASP_TRY(main_stream.acquire());
  hipStream_t s = main_stream.stream;
  ClassLauncher launcher;
  DeviceBuffer<uint64_t> d_x0, d_x0_perm, d_best, d_x;
  DeviceBuffer<double> d_partial, d_e, d_cache;
  DeviceBuffer<long long> d_tracked;
  DeviceBuffer<unsigned long long> d_accepted;
  DeviceBuffer<uint32_t> d_sweeps;
  DeviceBuffer<DescentProblem> d_problems;
  DeviceBuffer<PostProblem> d_post;
  DeviceBuffer<BatchSlot> d_slots, d_chains;
  asp::StreamFence fence(s);
  ASP_TRY(d_x0.alloc(n_x));
  ASP_TRY(d_x0_perm.alloc(n_blocks));
  ASP_TRY(d_best.alloc(n_blocks));
  ASP_TRY(d_x.alloc(n_x));
  ASP_TRY(d_partial.alloc(n_blocks));
  ASP_TRY(d_e.alloc(n));
  ASP_TRY(d_tracked.alloc(n));
  ASP_TRY(d_accepted.alloc(n));
  ASP_TRY(d_sweeps.alloc(n));
  use_cache = use_cache && field_cache_fits(d_cache, n_cache);
  // ---- descriptors ----
  for (size_t k = 0; k < n; ++k) {
    const asp_sa_greedy_item &it = items[shared[k]];
    const asp_sa_plan *p = it.plan;
    const asp::SaHostLayout &L = p->host;
    const uint64_t words = (L.num_spins + 63) / 64;
    std::copy(h_x0.begin() + tree_at[shared[k]], h_x0.begin() + tree_at[shared[k]] + words,
              h_x0_shared.begin() + off[k].x);
    DescentProblem d{};
    SweepArgs &a = d.s;
    // (betas stay null and the seed 0: the descent reads neither)
    a = sweep_args(p, kBytes, nullptr, d_x0_perm.ptr + off[k].blocks, d_best.ptr + off[k].blocks, d_tracked.ptr + k,
                   d_accepted.ptr + k, 0, it.max_sweeps, 0);
    // the field cache and its inert blocks as in the single path: late sweeps flip little
    a.field_cache = use_cache ? d_cache.ptr + off[k].cache : nullptr;
    a.cache_enter_flips = cache_enter_flips_of(L);
    d.x0 = d_x0.ptr + off[k].x;
    d.x0_perm = d_x0_perm.ptr + off[k].blocks;
    d.sweeps_done = d_sweeps.ptr + k;
    h_problems[k] = d;
    h_post[k] = post_problem_of(p, d_best.ptr + off[k].blocks, d_partial.ptr + off[k].blocks, d_e.ptr + k,
                                d_x.ptr + off[k].x);
    h_chains[k] = BatchSlot{static_cast<uint32_t>(k), 0u};
  }
  // ---- slot tables: per class, problems longest first, dealt to the 8 XCDs ----
  ASP_TRY(launcher.build(members, kNumBatchWaves));
  const std::vector<BatchSlot> &h_slots = launcher.h_slots;
  ASP_TRY(d_problems.alloc(n));
  ASP_TRY(d_post.alloc(n));
  ASP_TRY(d_slots.alloc(h_slots.size()));
  ASP_TRY(d_chains.alloc(n));
  {
    // host trees go up in one copy; device trees are written where the permute reads them (a batch of
    // device trees only moves no tree words over PCIe)
    std::vector<asp::GreedyTreeTarget> targets;
    for (size_t k = 0; k < n; ++k) {
      asp_sa_plan *p = items[shared[k]].plan;
      if (p->greedy_tree != 0) targets.push_back(asp::GreedyTreeTarget{p, d_x0.ptr + off[k].x, nullptr});
    }
    if (targets.size() != n) ASP_TRY(d_x0.upload(h_x0_shared.data(), n_x, s));
    if (!targets.empty()) {
      float split_ms[3] = {0.0f, 0.0f, 0.0f};
      ASP_TRY(asp::greedy_tree_device(targets.data(), static_cast<uint32_t>(targets.size()), s, split_ms));
      asp::greedy_tree_record_ms(split_ms, device_trees_ran);
      g_greedy_tree_ms += split_ms[0] + split_ms[1] + split_ms[2];
    }
  }
  ASP_TRY(d_problems.upload(h_problems.data(), n, s));
  ASP_TRY(d_post.upload(h_post.data(), n, s));
  ASP_TRY(d_slots.upload(h_slots.data(), h_slots.size(), s));
  ASP_TRY(d_chains.upload(h_chains.data(), n, s));
  // every problem's tree signs into block order: one launch
  ASP_TRY(launch_permute_problems(d_problems.ptr, static_cast<unsigned>(n), s));
  // ---- one descent launch per class ----
  ASP_TRY(launcher.run(s, d_problems.ptr, d_slots.ptr, [&](int c) {
    return ClassKernel<DescentProblem>{batch_kernel_of<DescentProblem>(1, kBytes), 64u * kBatchWaves[c]};
  }));
  // ---- energies and original-order bits of every problem's final configuration ----
  ASP_TRY(launch_post_batch(d_post.ptr, d_chains.ptr, static_cast<unsigned>(n), energy_lds, max_lds, s));
  ASP_TRY(d_x.download(h_x.data(), n_x, s));
  ASP_TRY(d_e.download(h_e.data(), n, s));
  ASP_TRY(d_sweeps.download(h_sweeps.data(), n, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&ms, launcher.begin, launcher.end));
  g_greedy_descent_ms += ms;
  for (size_t k = 0; k < n; ++k) {
    const asp_sa_greedy_item &it = items[shared[k]];
    asp_sa_plan *p = it.plan;
    const uint64_t words = (p->host.num_spins + 63) / 64;
    std::copy(h_x.begin() + off[k].x, h_x.begin() + off[k].x + words, it.out_x);
    *it.out_e = h_e[k];
    if (it.out_sweeps) *it.out_sweeps = h_sweeps[k];
    p->last_tracked.clear();  // (the shared launches bring no per-chain statistics back)
    p->last_accepted.clear();
    record_shared_launch(p, 1, kBytes, kBatchWaves[members[k].cls], 1);
  }
  return ASP_OK;
}

}  // extern "C"
