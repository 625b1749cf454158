// The plan object behind asp_sa_plan_create and the host helpers the annealing translation
// units share.  The colour order defines them — csrc/sa_anneal.hip (the plan's device setup, a handle's
// segment), csrc/sa_energy.hip (permute, energies), csrc/sa_batch.hip (batched segments) —, and
// csrc/sa_shuffled.hip, csrc/sa_chains.hip and the others use them.  What only the colour order's own
// units share is in sa_colour.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "asp_common.hpp"
#include "sa_plan.hpp"

namespace asp {

// What asp_sa_plan_reweight needs besides the layout (csrc/sa_reweight.hip): the CSR
// pattern the plan was created from, kept to compare a reweight's pattern with exactly, and — built by
// the family's first reweight, on the host from the pattern and the layout, uploaded once — where every
// entry of A comes from and goes to.  Immutable once built; a plan and its clones share one.
struct SaPattern {
  uint64_t nnz = 0;
  std::vector<int64_t> indptr;   // num_spins + 1 (empty: no spins)
  std::vector<int32_t> indices;  // nnz
  std::mutex build;              // (two clones may ask for the maps at the same time)
  bool built = false;
  static constexpr uint32_t kNone = 0xFFFFFFFFu;
  // per entry e of A (row i, k-th of the row, column j):
  std::vector<uint32_t> src_ij, src_ji;  // positions of J_ij and J_ji in `data`, kNone where absent
  std::vector<uint64_t> ell_slot;        // its element of ell_val
  std::vector<uint32_t> rq_slot;         // its element of rq_val (the rows padded to quads)
  std::vector<int64_t> diag_pos;         // per row: the position of J_ii in `data`, or -1
  // stored off-diagonal pairs that A does NOT hold (J_ij + J_ji was exactly 0 at creation): they must
  // still cancel after a reweight, or a fresh plan would have one more entry; second = -1: one-sided
  std::vector<std::pair<int64_t, int64_t>> dropped;
  DeviceBuffer<uint32_t> d_src_ij, d_src_ji, d_rq_slot;
  DeviceBuffer<uint64_t> d_ell_slot;
  DeviceBuffer<int64_t> d_a_ptr;
};

}  // namespace asp

struct asp_sa_plan {
  asp::SaHostLayout host;
  std::shared_ptr<asp::SaPattern> pattern;  // set by asp_sa_plan_create, shared by asp_sa_plan_clone
  // handles of asp_sa_chains_create that are alive (a handle may outlive its plan, so it holds the
  // counter too): asp_sa_plan_reweight refuses while there is one
  std::shared_ptr<std::atomic<int>> live_chains = std::make_shared<std::atomic<int>>(0);
  // asp_sa_plan_reweight's staging (grown on demand and kept): the new data and field, the merged
  // values of A, per row sum |A_ij| and the smallest non-zero 2 |A_ij|, the count of cancelled entries
  asp::DeviceBuffer<double> rw_data, rw_field, rw_a_val, rw_row_sum, rw_row_min;
  asp::DeviceBuffer<uint32_t> rw_zeros;
  float rw_last_ms = 0.0f;  // asp_sa_plan_reweight_last_ms
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_sweep_ms = 0.0f, last_total_ms = 0.0f;
  int force_m = 0, force_threads = 0;
  int force_packed = 0;  // asp_sa_set_packed: 0 auto, 1 bits in LDS, 2 bits in HBM
  bool allow_wide = true;  // asp_sa_set_wide
  int last_m = 0, last_threads = 0, last_groups = 0;
  std::vector<int64_t> last_tracked;
  std::vector<uint64_t> last_accepted;
  int num_cus = 256;
  size_t max_lds = 160 * 1024;
  // asp_sa_set_lds_limit (0: the device's): the LDS per workgroup the SPIN LAYOUT of a sweep is chosen
  // for, in both orders — spin_lds() wherever bytes / nibbles / bits / HBM is decided; what a launch
  // may ask for, the order build's and the team sweep's LDS stay with max_lds
  size_t spin_lds_limit = 0;
  size_t spin_lds() const { return spin_lds_limit ? std::min(spin_lds_limit, max_lds) : max_lds; }
  asp::DeviceBuffer<uint32_t> color_block_start, block_width, ell_col, spin_of_pos, pos_of_spin;
  asp::DeviceBuffer<uint32_t> ell_col4;  // columns as LDS byte addresses of the wide layout (if it fits)
  int last_layout = 0;
  int last_spin_layout = 0;  // asp_sa_last_spin_layout: the spin layout behind last_layout's 4 and 5 too
  asp::DeviceBuffer<uint64_t> ell_off;
  asp::DeviceBuffer<double> ell_val, field_pos;
  // per-call work buffers, grown on demand and kept (a plan is used by one thread at a time)
  asp::DeviceBuffer<double> w_betas, w_partial, w_e;
  asp::DeviceBuffer<uint64_t> w_best, w_x0, w_x0_perm, w_x;
  asp::DeviceBuffer<long long> w_tracked;
  asp::DeviceBuffer<unsigned long long> w_accepted;
  asp::DeviceBuffer<double> w_field_cache;  // [groups][blocks][M][64], see SweepArgs::field_cache
  asp::DeviceBuffer<uint64_t> w_spins;      // [groups][blocks] sign words of the HBM-resident layout
  asp::DeviceBuffer<long long> w_trace;     // [groups * M][sweeps + 1] tracked energies (asp_sa_anneal_trace)
  asp::DeviceBuffer<uint64_t> w_cur_perm;   // [groups * M][blocks] sign words of a handle's chains (Resume::cur_perm)
  asp::DeviceBuffer<long long> w_e_cur;     // [groups * M] their current tracked energies (Resume::e_cur)
  // team sweep exchange area, FINE-GRAINED device memory (coherent across XCDs without cache
  // maintenance): arrivals u64[teams] | sums i64[teams][6] | abort u32 (+pad) | flips u64[teams][blocks]
  void *team_area = nullptr;
  size_t team_area_bytes = 0;
  ~asp_sa_plan() {
    if (team_area) (void)hipFree(team_area);
  }
  int team_mode = -1;  // asp_sa_set_team: -1 auto, 0 off, G >= 2 forced
  bool use_field_cache = true;
  int tail_mode = -1;  // asp_sa_set_tail: -1 auto, 0 off, n > 0: tail sweeps below n flips per sweep
  asp::DeviceBuffer<uint32_t> w_tail;  // [groups][2] tail sweeps run and entries into them (TailArgs::report)
  std::vector<uint32_t> last_tail;     // its host copy for the last closed call (empty: no tail kernel)
  bool use_post = true;  // asp_sa_set_post: k_sa_post for the pass after a sweep launch
  uint32_t team_abort_host = 0;  // landing place of the watchdog flag's asynchronous read-back
  uint32_t team_watchdog_trips = 0;  // calls of this plan that the team barrier's watchdog cut short (each ~5 s lost)
  // Shuffled sweep (csrc/sa_shuffled.hip; uploaded on first use): rows of A over ORIGINAL
  // indices, padded to whole quads (padding: own index, +0.0) — row i is quads
  // rq_ptr[i] .. rq_ptr[i + 1]; per quad four columns and four values in the interleaving the
  // sweep kernels read (sa_plan.cpp) —, the field in original order and a degree class per spin
  asp::DeviceBuffer<uint32_t> rq_ptr;
  asp::DeviceBuffer<uint32_t> rq_col;   // [quads][4]
  asp::DeviceBuffer<double> rq_val;     // [quads][4]
  asp::DeviceBuffer<double> field_dev;  // [K]
  uint32_t rq_quads = 0, rq_max_quads = 0;
  int shuffled_m = 0, shuffled_waves = 0;  // asp_sa_set_shuffled_launch (0 = automatic)
  int shuffled_teams = 0;                  // asp_sa_set_shuffled_teams (0 = automatic)
  int last_shuffled_levels = 0;            // largest number of levels of the last shuffled call
  uint32_t last_shuffled_log_s = 6, last_shuffled_wgs = 0;  // block size and workgroups of the last shuffled call
  uint32_t last_shuffled_blocks = 0, last_shuffled_quads = 0;  // most blocks / quads of one sweep of that call
  float last_order_ms = 0.0f;              // device time of the last call's order kernels
  // Cluster moves (csrc/sa_cluster.hip; uploaded on first use): rows of A over ORIGINAL indices as a plain
  // CSR (ascending columns, no padding), the field in original order, and the per-pair bit planes of the
  // HBM form ([pairs][3][2 words] 32-bit words)
  asp::DeviceBuffer<uint32_t> cluster_row_ptr, cluster_col;
  asp::DeviceBuffer<double> cluster_val, cluster_field;
  asp::DeviceBuffer<uint32_t> cluster_scratch;
  int greedy_tree = 0;  // asp_sa_set_greedy_tree: 0 host tree, 1 device tree (forest placed by size), 2 forest in HBM
};


// The chains behind asp_sa_chains_create: everything a continuation needs, on the
// device and independent of the sweep order and of every launch choice — configurations packed in
// ORIGINAL spin order (bit = +1) and three integers per chain.  Sized once, at create (the second set
// below: at the handle's first gather).
struct asp_sa_chains {
  asp_sa_plan *plan = nullptr;
  std::shared_ptr<std::atomic<int>> live_of_plan;  // asp_sa_plan::live_chains, counted down at destroy
  uint64_t seed = 0;
  uint32_t repetitions = 0, replica_offset = 0, words = 0;
  uint32_t sweeps_done = 0;
  asp::DeviceBuffer<uint64_t> x_cur, x_best;        // [repetitions][words]
  asp::DeviceBuffer<long long> e_cur, e_best;       // [repetitions] tracked energies (fixed point)
  asp::DeviceBuffer<unsigned long long> accepted;   // [repetitions]
  std::vector<int64_t> h_e_cur;                     // host copy of e_cur (entry 0 of a segment's trace)
  // A second set of the five arrays, allocated by the first asp_sa_chains_gather /
  // _resample of the handle: a gather writes it and the two sets change places.
  asp::DeviceBuffer<uint64_t> x_cur_to, x_best_to;
  asp::DeviceBuffer<long long> e_cur_to, e_best_to;
  asp::DeviceBuffer<unsigned long long> accepted_to;
  int cluster_planes = 0;  // asp_sa_chains_set_cluster_planes: 0 auto, 1 bit planes in LDS, 2 in HBM
};

namespace asp {

// What every batched call over handles checks once its own arguments are valid: the (non-null) handles
// of a batch are distinct handles of distinct plans — a plan's work buffers serve one call at a time; the
// same handle twice is the same plan twice, reported as what it is.  ASP_ERR_INVALID with both indices.
inline int check_distinct_plans(const std::vector<asp_sa_chains *> &handles) {
  const uint32_t count = static_cast<uint32_t>(handles.size());
  std::vector<std::pair<const asp_sa_plan *, uint32_t>> plans(count);
  for (uint32_t i = 0; i < count; ++i) plans[i] = {handles[i]->plan, i};
  std::sort(plans.begin(), plans.end());
  for (uint32_t i = 1; i < count; ++i) {
    if (plans[i].first != plans[i - 1].first) continue;
    const uint32_t a = plans[i - 1].second, b = plans[i].second;
    if (handles[a] == handles[b]) {
      return set_error(ASP_ERR_INVALID, "items %u and %u are the same handle", a, b);
    }
    return set_error(ASP_ERR_INVALID, "items %u and %u are handles of one plan", a, b);
  }
  return ASP_OK;
}

// What asp_sa_plan_create does once p->host is filled — stream, events, device limits and the uploads of
// the layout —, for asp_sa_plan_clone as well (csrc/sa_anneal.hip).  ASP_OK, or the error recorded; the
// caller destroys the plan.
int sa_plan_device_setup(asp_sa_plan *p);

// Rows of A over original indices and the field in original order (asp_sa_plan::cluster_*), uploaded
// on first use; shared by the cluster moves (csrc/sa_cluster.hip) and the device tree (csrc/greedy_tree.hip).
int ensure_rows(asp_sa_plan *p);

template <typename T>
int upload_vector(DeviceBuffer<T> &dst, const std::vector<T> &src, hipStream_t stream) {
  ASP_TRY(dst.alloc(src.size()));
  return dst.upload(src.data(), src.size(), stream);
}

struct EventPool {
  std::vector<hipEvent_t> events;
  ~EventPool() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
  }
  int make(hipEvent_t *out, bool timing = false) {
    ASP_HIP_TRY(hipEventCreateWithFlags(out, timing ? hipEventDefault : hipEventDisableTiming));
    events.push_back(*out);
    return ASP_OK;
  }
};

// XCD-aware slot lists of one shared launch.  Workgroups are dealt round-robin over the chip's eight
// XCDs (blocks b and b + 8 share one, each XCD with an L2 of its own), so the workgroups of ONE member
// get slots of one XCD — what every workgroup of the member reads is then fetched from HBM by one L2
// instead of eight (a placement for speed only: nothing depends on it).  The members (indices, in the
// caller's order) go in descending work_of(member), stable, each whole — groups_of(member) slots
// {member, 0 .. groups - 1} — to the XCD with the fewest slots so far (ties: lowest index): balanced
// and deterministic.  Every list is then padded to the longest with {0xFFFFFFFF, 0}; returns that
// length.  How the eight lists are flattened is the caller's.
constexpr int kXcds = 8;
template <typename Slot, typename WorkOf, typename GroupsOf>
uint32_t deal_to_xcds(std::vector<uint32_t> members, WorkOf work_of, GroupsOf groups_of,
                      std::vector<Slot> (&per_xcd)[kXcds]) {
  std::stable_sort(members.begin(), members.end(), [&](uint32_t a, uint32_t b) { return work_of(a) > work_of(b); });
  for (auto &list : per_xcd) list.clear();
  for (uint32_t k : members) {
    int least = 0;
    for (int x = 1; x < kXcds; ++x) {
      if (per_xcd[x].size() < per_xcd[least].size()) least = x;
    }
    const uint32_t groups = groups_of(k);
    for (uint32_t g = 0; g < groups; ++g) per_xcd[least].push_back(Slot{k, g});
  }
  size_t longest = 0;
  for (auto &list : per_xcd) longest = std::max(longest, list.size());
  for (auto &list : per_xcd) list.resize(longest, Slot{0xFFFFFFFFu, 0u});
  return static_cast<uint32_t>(longest);
}

// perm[c][b] = sign words (bit = 1: s = -1) of configuration c in the plan's block order, from
// packed original-order configurations x[c][ceil(K/64)] (bit = 1: s = +1); on the plan's stream
// (csrc/sa_energy.hip, as the next).
int sa_permute_bits(asp_sa_plan *p, const uint64_t *x, uint32_t count, uint64_t *perm);

// Reported energies of `count` configurations given as block-order sign words;
// partial: count * num_blocks doubles of scratch; on the plan's stream.
int sa_energies_of_perm(asp_sa_plan *p, const uint64_t *perm, uint32_t count, double *partial,
                        double *out_e);

// asp_sa_anneal_batch's items with ASP_SA_BATCH_SHUFFLED set (csrc/sa_shuffled.hip): items[which[k]],
// k < count; adds the device time of their sweeps to *sweep_ms.
int sa_shuffled_batch(asp_sa_batch_item const *items, const uint32_t *which, uint32_t count, float *sweep_ms);

// One segment of asp_sa_chains_advance (arguments validated, num_sweeps > 0, a plan with spins):
// sweeps c->sweeps_done .. + num_sweeps - 1 from and into the handle's state; c->sweeps_done is the
// caller's to advance.  trace: nullptr or HOST [repetitions][num_sweeps + 1], entries 1.. written here.
// Colour order (csrc/sa_anneal.hip; the kernels: csrc/sa_sweep.hip) and shuffled order (csrc/sa_shuffled.hip).
int sa_chains_advance_colour(asp_sa_chains *c, double const *betas, uint32_t num_sweeps, int64_t *trace);
int sa_chains_advance_shuffled(asp_sa_chains *c, double const *betas, uint32_t num_sweeps, int64_t *trace);

// One LADDER segment (asp_sa_chains_advance_ladder; the same contract): chain r runs its num_sweeps sweeps
// at chain_betas[r] (HOST [repetitions], validated).  The launch forms of sa_chains_advance_colour /
// _shuffled (the shuffled order: one team), with the per-chain-beta instantiations of the sweep kernels.
int sa_chains_advance_ladder_colour(asp_sa_chains *c, double const *chain_betas, uint32_t num_sweeps, int64_t *trace);
int sa_chains_advance_ladder_shuffled(asp_sa_chains *c, double const *chain_betas, uint32_t num_sweeps, int64_t *trace);

// The items of asp_sa_chains_advance_batch that run sweeps (validated; distinct handles of distinct
// plans with spins and chains, num_sweeps > 0), one visiting order at a time: every segment is exactly
// its sa_chains_advance_colour / _shuffled call, the handles that fit share launches.  h_e_cur of the
// handles is the caller's to refresh; adds the device time of the sweep launches to *sweep_ms.
// A batch of LADDER segments (asp_sa_chains_advance_ladder_batch): chain_betas set in EVERY segment of
// the call (HOST [repetitions], validated; `betas` unused) — every segment is exactly its
// sa_chains_advance_ladder_colour / _shuffled call, in the shared launches' per-chain-beta forms.
// Ladder and plain segments never share a call.
struct ChainsSegment {
  asp_sa_chains *chains;
  double const *betas;
  uint32_t num_sweeps;
  int64_t *trace;  // nullptr, or HOST [repetitions][num_sweeps + 1]: the segment runs alone
  double const *chain_betas = nullptr;  // a ladder segment: one inverse temperature per chain
};
int sa_chains_advance_colour_batch(const ChainsSegment *segs, uint32_t count, float *sweep_ms);  // csrc/sa_batch.hip
int sa_chains_advance_shuffled_batch(const ChainsSegment *segs, uint32_t count, float *sweep_ms);

}  // namespace asp
