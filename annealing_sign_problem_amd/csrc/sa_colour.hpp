// What the translation units of the colour-order annealer share: the argument types of the kernels, the
// LDS layout of a sweep, and the prototypes of what the units offer each other.  Declarations only.
//   csrc/sa_sweep.hip   the sweep kernels and every decision about which of them runs in which shape
//   csrc/sa_energy.hip  the pass after the sweeps: reported energies, permute / unpermute
//   csrc/sa_anneal.hip  the plan, the closed calls and a handle's segment (host only)
//   csrc/sa_batch.hip   the shared launches of many problems (host only)
// Without relocatable device code a kernel is launched from the unit that defines it; the other units
// get it as a pointer (segment_kernel_of and the like) or through a launch wrapper.
// This header and csrc/sa_sweep.hip are what a profiler counter of k_sa_sweep* can depend on
// (build.KERNEL_SOURCE_SETS["colour"]); the host drivers are not.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sa_device.hpp"
#include "sa_internal.hpp"

namespace asp {
namespace colour {

using dev::kBits;
using dev::kBytes;
using dev::kGlobal;
using dev::kNibbles;
using dev::kWide;

// ---- the kernels' arguments ----
struct SweepArgs {
  const uint32_t *color_block_start;  // num_colors + 1
  const uint32_t *block_width;        // num_blocks
  const uint64_t *ell_off;            // num_blocks + 1 (slabs)
  const uint32_t *ell_col;
  const double *ell_val;
  const uint32_t *spin_of_pos;  // num_blocks * 64
  const double *field_pos;      // num_blocks * 64
  const double *betas;          // num_sweeps
  const uint64_t *x0_perm;      // num_blocks sign-bit words or nullptr
  uint64_t *best_perm;          // [groups * M][num_blocks] sign-bit words
  long long *tracked;           // [groups * M] best tracked energy (fixed point)
  unsigned long long *accepted;  // [groups * M] accepted flips
  uint64_t seed;
  double scale;  // 2^S
  uint32_t num_colors, num_blocks, num_sweeps, replica_first;
  // Field cache (nullptr = off): [group][block][m][lane] local fields (the row sums `acc`) of the
  // last evaluation of every block, valid while the block's dirty byte in LDS is clear.
  double *field_cache;
  uint32_t cache_enter_flips;  // switch the cache on after a sweep with fewer flips than this
  uint64_t *spin_words;        // kGlobal: [groups][num_blocks] sign-bit words in HBM
  long long *trace;            // nullptr or [groups * M][num_sweeps + 1] tracked energy per sweep
};

// How a launch starts and ends.  NoResume: the closed calls — a fresh chain (one shared x0 or the
// counter RNG, tracked energy 0, sweep index 0) whose final state is dropped.  Resume: one segment of
// an asp_sa_chains handle — every chain starts from its OWN sign words, the
// tracked energy, the best threshold and the flip count start from carried values (a.tracked and
// a.accepted are read before they are written), sweep t of the launch draws with sweep index t0 + t,
// and the final configuration and tracked energy are stored beside the best ones.  All of it at the
// head and the tail of the launch; a template parameter, so the closed calls' instantiations stay
// what they were.
struct NoResume {
  static constexpr bool kEnabled = false;
  static constexpr bool kLadder = false;
};
struct Resume {
  static constexpr bool kEnabled = true;
  static constexpr bool kLadder = false;
  uint64_t *cur_perm;  // [groups * M][num_blocks] sign-bit words: start of every chain in, final state out
  long long *e_cur;    // [groups * M] current tracked energy, in and out
  uint32_t t0;         // sweeps the chains have behind them
};
// ResumeLadder: a Resume segment in which every chain runs at its OWN inverse temperature, constant
// over the segment (asp_sa_chains_advance_ladder, DESIGN.md §4.10 "Ladder law"): a.betas is never
// read, replica m of the group reads chain_betas once before the sweep loop.  The inert bytes stay
// valid inside the segment — a certain rejection of replica m was certain at replica m's beta, which
// does not change — and nothing is carried in from the segment before (which may have run colder):
// the control words, the dirty and the inert bytes live in LDS and are set up by every launch, cached mode is
// entered with every block stale, and an inert byte is only read for a block evaluated since.
struct ResumeLadder {
  static constexpr bool kEnabled = true;
  static constexpr bool kLadder = true;
  uint64_t *cur_perm;
  long long *e_cur;
  uint32_t t0;
  const double *chain_betas;  // [groups * M]; the chains padding the last group: 0
};

// What the TAIL form of the body takes beside SweepArgs (k_sa_sweep_tail; a wrapper would change the
// descriptor stride of the batched kernels, so it travels as a kernel argument of its own).
struct TailArgs {
  uint32_t enter_flips;  // tail sweeps after a sweep with fewer flips of the workgroup than this
  uint32_t *report;      // [groups][2]: sweeps run as tail sweeps, entries into tail mode
};
constexpr uint32_t kTailRing = 128;  // rows a wavefront stages: under 64 waiting plus one block's 64

// ---- The dynamic LDS of a one-workgroup colour sweep: the byte offset of every region, for the device
// body's pointers, and the total, for the host (sweep_lds_bytes).  A region is added in this one place. ----
//   spins | delta[8] | book[24] | flag (16 B) | meta[num_blocks] | ctl ...
//   bytes, words, nibbles: ... ctl[4] | dirty[num_blocks] | inert[num_blocks]   (each rounded up to 16 B)
//   TAIL (bytes, words):   ... ctl[8] | todo[num_blocks] | kTailRing staged rows per wavefront
//   bits, global:          no meta (block metadata comes from HBM by scalar loads, the field cache is
//                          not available); ctl[4] and 16 B that nobody uses; global: no spins either
// spins: 64 (a byte per position), 32 (a nibble), 8 (a bit) or 256 (a word) bytes per block: delta is 64-B aligned.
// Per replica m: delta[m] = energy change of the running sweep, book[m] = current tracked energy,
//   book[8 + m] = best, book[16 + m] = accepted flips.  flag: bit m = replica m improved in this sweep;
//   its second word (a segment in words): bit m = replica m improved in this launch.
// meta[b] = {first ELL slab, EXACT width} of block b: its longest row, which the plan's block_width rounds
//   up to whole quads (ColourSweep::start derives it): (width + 3) / 4 quads, the last of width % 4 real
//   terms (0: of four).  ctl: the CtlSlot words below.
// dirty[b]: bit m = replica m's cached fields of block b are stale.  inert[b], meaningful while the dirty
//   byte is clear: at the block's last evaluation every proposal was a certain rejection (beta * dE >= 23
//   -> expneg = 0, or dE >= 0 in descent mode) and beta has not decreased since: the visit can be skipped.
// todo[b] (a u64): bit l = row l of block b is evaluated at the next visit of its colour.
struct SweepLds {
  uint32_t delta = 0, book = 0, flag = 0, meta = 0, ctl = 0, dirty = 0, inert = 0, todo = 0, ring = 0, total = 0;
  __host__ __device__ constexpr SweepLds(uint32_t num_blocks, int layout, bool tail, uint32_t waves) {
    const bool packed = layout == kBits || layout == kGlobal;
    const uint32_t per_block =
        layout == kGlobal ? 0u : (layout == kBits ? 8u : (layout == kWide ? 256u : (layout == kNibbles ? 32u : 64u)));
    delta = num_blocks * per_block;
    book = delta + 8u * 8u;
    flag = book + 24u * 8u;
    meta = flag + 16u;
    ctl = meta + (packed ? 0u : num_blocks * 8u);
    if (tail) {
      todo = ctl + 8u * 4u;
      ring = todo + num_blocks * 8u;
      total = ring + waves * kTailRing * 4u;
    } else if (packed) {
      total = ctl + 32u;
    } else {
      const uint32_t bytes16 = (num_blocks + 15u) & ~15u;
      dirty = ctl + 4u * 4u;
      inert = dirty + bytes16;
      total = inert + bytes16;
    }
  }
};
static_assert(SweepLds(1, kBytes, false, 0).total == 392 && SweepLds(17, kBytes, false, 0).total == 1576 &&
                  SweepLds(17, kWide, false, 0).total == 4840 && SweepLds(17, kNibbles, false, 0).total == 1032 &&
                  SweepLds(17, kBits, false, 0).total == 440 && SweepLds(17, kGlobal, false, 0).total == 304 &&
                  SweepLds(17, kBytes, true, 16).total == 9856 && SweepLds(17, kWide, true, 8).total == 9024,
              "the LDS totals of the sweep kernels");

// Many PROBLEMS in one launch (asp_sa_anneal_batch): workgroup -> (problem, group of M replicas)
// through a slot table, the problem's SweepArgs through a descriptor table in HBM (scalar
// loads: the slot is workgroup-uniform).  Slots are laid out per XCD — workgroup i runs on XCD
// i mod 8 — so that the groups of one problem share that XCD's L2 copy of its couplings, and in
// descending order of work inside an XCD (longest first, the tail stays short).  Every chain is
// bit-identical to the one its own single-problem launch produces: the body is the same and
// results never depend on the launch geometry.
struct BatchSlot {
  uint32_t problem;  // 0xFFFFFFFF: padding slot
  uint32_t group;
};
template <typename Problem>  // SweepArgs, or one of the wrappers below
struct BatchArgs {
  const Problem *problems;
  const BatchSlot *slots;  // [8][slots_per_xcd]
  uint32_t slots_per_xcd;
};

// What a launch needs beyond SweepArgs lives in a wrapper, so that SweepArgs — shared by every
// annealing kernel, whose register assignment follows its layout — stays as it is.
//
// Many DESCENTS in one launch (asp_sa_greedy_batch): every problem is one chain, so its group is
// always 0.  Each problem starts from its own configuration (s.x0_perm), runs strict-descent sweeps
// until one flips nothing or s.num_sweeps (the caller's max_sweeps) are done — decided by the workgroup
// that owns the whole chain, with no host round trip — and leaves the number of sweeps in its own word.
struct DescentProblem {
  SweepArgs s;            // betas: nullptr (never read); num_sweeps: the cap; trace: nullptr
  const uint64_t *x0;     // the tree's configuration, packed in original order (bit = +1)
  uint64_t *x0_perm;      // = s.x0_perm, written by k_permute_bits_problems
  uint32_t *sweeps_done;  // sweeps performed
};
// Many SEGMENTS in one launch (asp_sa_chains_advance_batch, order 0): every handle's SweepArgs and its
// Resume part (its own sign words, tracked energies and sweep index base).  Every chain is the one
// k_sa_sweep_resume advances: the body is the same.
struct ResumeProblem {
  SweepArgs s;  // trace: nullptr (a traced segment runs alone)
  Resume r;
};
// Many LADDER segments in one launch (asp_sa_chains_advance_ladder_batch, order 0): chain_betas points
// at the handle's [groups * M] values inside the batch's one concatenated buffer (the chains padding a
// last group: 0).
struct LadderProblem {
  SweepArgs s;  // betas: nullptr (never read); trace: nullptr (a traced segment runs alone)
  ResumeLadder r;
};

// k_sa_sweep_team: one chain spread over team_size workgroups (csrc/sa_sweep.hip).
struct TeamArgs {
  SweepArgs s;
  uint32_t team_size;            // G
  uint32_t num_teams;            // = chains of the launch
  unsigned long long *arrivals;  // [num_teams] barrier counters (monotone)
  uint64_t *flips;               // [num_teams][num_blocks] flip words of the running colour step
  long long *sums;               // [num_teams][3 rotating slots][2] {dq, accepted} of a sweep
  uint32_t *abort;               // set by the watchdog
  uint32_t spin_limit;           // barrier polls before the watchdog gives up
};

// ---- the pass after the sweeps (csrc/sa_energy.hip) ----
struct EnergyArgs {
  const uint32_t *block_width;
  const uint64_t *ell_off;
  const uint32_t *ell_col;
  const double *ell_val;
  const double *field_pos;
  const uint64_t *perm_words;  // [count][num_blocks] sign bits
  double *partial;             // [count][num_blocks]
  uint32_t num_blocks;
};
// k_sa_post: the block sums and, when `x` is given, the configurations in original order.
struct PostArgs {
  EnergyArgs e;
  const uint32_t *pos_of_spin;
  uint64_t *x;  // nullptr, or [count][words] configurations in original order (bit = +1)
  uint64_t num_spins;
  uint32_t words;
};
// The same for the chains of MANY problems: workgroup -> (problem, chain) through a table of BatchSlot.
struct PostProblem {
  EnergyArgs e;  // perm_words / partial: this problem's rows
  const uint32_t *pos_of_spin;
  uint64_t num_spins;
  uint32_t words;
  double diag_sum;
  double *out_e;    // [repetitions]
  uint64_t *out_x;  // [repetitions][words]
};
// The handles of a batched segment into and out of the form k_sa_sweep_batch runs their segments in
// (k_chains_permute_problems, k_chains_unpermute_problems).
struct ChainsIo {
  uint64_t *x_cur, *x_best;  // the handle: [chains][words], original order, bit = +1
  long long *e_cur, *e_best;
  unsigned long long *accepted;
  uint64_t *cur_perm, *best_perm;  // the launch: [padded][num_blocks] sign words (bit = -1)
  long long *w_e_cur, *w_tracked;  // [padded]
  unsigned long long *w_accepted;
  const uint32_t *spin_of_pos, *pos_of_spin;
  uint64_t num_spins;
  uint32_t num_blocks, words, chains;
};

// ---- launch decisions (csrc/sa_sweep.hip) ----
// Chains per group, threads and spin layout of a launch with one workgroup per group of chains —
// shared by the closed calls (run_chains, which may then spread a chain over a team instead) and by
// the segments of a handle (sa_chains_advance_colour), so that both take the same form.
struct ColourLaunch {
  int m = 1, threads = 64, layout = kBytes;
};
ColourLaunch choose_colour_launch(const asp_sa_plan *p, uint32_t repetitions, bool descent, bool traced);
// Workgroups per chain of a closed call that would otherwise run `form` (k_sa_sweep_team), or 0: no teams.
uint32_t choose_team(const asp_sa_plan *p, const ColourLaunch &form, uint32_t repetitions, bool traced);
bool bit_packed(int layout);
bool colour_form_listed(int m, int layout);  // there are kernels of m chains per group in `layout`
size_t sweep_lds_bytes(const SaHostLayout &L, int layout, bool tail = false, int threads = 0);
size_t team_lds_bytes(const SaHostLayout &L);
uint32_t widest_color(const SaHostLayout &L);
uint32_t tail_enter_flips_of(const SaHostLayout &L);
uint32_t cache_enter_flips_of(const SaHostLayout &L);
SweepArgs sweep_args(const asp_sa_plan *p, int layout, const double *betas, const uint64_t *x0_perm,
                     uint64_t *best_perm, long long *tracked, unsigned long long *accepted, uint64_t seed,
                     uint32_t num_sweeps, uint32_t replica_first);

// The kernel of a launch, or nullptr: no such form.  Launched by whoever asks (ColourRun::launch,
// launch_team, ClassLauncher::run).  Res: Resume, ResumeLadder.  Problem: SweepArgs, DescentProblem,
// ResumeProblem, LadderProblem.
using ClosedKernel = void (*)(SweepArgs);
using TailKernel = void (*)(SweepArgs, TailArgs);
using TeamKernel = void (*)(TeamArgs);
template <typename Res>
using SegmentKernel = void (*)(SweepArgs, Res);
template <typename Problem>
using BatchKernel = void (*)(BatchArgs<Problem>);
ClosedKernel closed_kernel_of(int m, bool descent, int layout, uint32_t replica_first);
TailKernel tail_kernel_of(const asp_sa_plan *p, int m, int threads, int layout, bool descent, uint32_t replica_first);
TeamKernel team_kernel_of(bool descent);
template <typename Res>
SegmentKernel<Res> segment_kernel_of(int m, int layout);
template <typename Problem>
BatchKernel<Problem> batch_kernel_of(int m, int layout);

// The class rule of the shared launches: the wavefront counts of the launch classes, and the layout and
// wavefronts of a problem that fits a byte per position.
constexpr uint32_t kBatchWaves[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int kNumBatchWaves = sizeof kBatchWaves / sizeof kBatchWaves[0];
struct BatchEntry {
  uint32_t item;     // index into the caller's array
  uint32_t chains;   // its chains
  uint32_t waves;    // wavefronts per workgroup this problem wants
  int layout;        // kWide or kBytes; the closed batch: kNibbles or kBits as well
  double work;       // ~ time of one group: sweeps * ELL slabs
  uint64_t beta_at;  // offset of its schedule (a ladder segment: its chains' betas) in the concatenated betas
};
int batch_waves_index(uint32_t waves);
int batch_layout_in_lds(const asp_sa_plan *p);  // kWide or kBytes
uint32_t batch_waves(const SaHostLayout &L);
int batch_chains_per_group(const std::vector<BatchEntry> &entries, int num_cus);

// ---- the pass after the sweeps and the state permutes (csrc/sa_energy.hip) ----
// out_x: nullptr, or [count][ceil(K/64)] — the configurations in original order (bit = +1) as well:
// written by k_sa_post where it runs, by k_unpermute_bits behind the older energy kernels.
int energies_of_perm(asp_sa_plan *p, const uint64_t *perm_words, uint32_t count, double *partial, double *out_e,
                     uint64_t *out_x = nullptr);
// x[c] = configuration c in original order (bit = +1) from its block-order sign words; the plan's stream.
int unpermute_bits(asp_sa_plan *p, const uint64_t *perm_words, uint32_t count, uint64_t *x);
PostProblem post_problem_of(const asp_sa_plan *p, const uint64_t *best, double *partial, double *out_e,
                            uint64_t *out_x);
int launch_post_batch(const PostProblem *d_post, const BatchSlot *d_chains, unsigned chains, size_t energy_lds,
                      size_t max_lds, hipStream_t s);
int launch_permute_problems(const DescentProblem *d_problems, unsigned problems, hipStream_t s);
int launch_chains_permute(const ChainsIo *d_io, const BatchSlot *d_chains, unsigned chains, hipStream_t s);
int launch_chains_unpermute(const ChainsIo *d_io, const BatchSlot *d_chains, unsigned chains, hipStream_t s);

// ---- the single-problem drivers (csrc/sa_anneal.hip), for the items of a batch that run alone ----
// The argument checks of a closed call of `repetitions` > 0 chains, every message behind `prefix`;
// flags outside `known_flags` are refused.
int check_closed_call(const char *prefix, const void *out_x, const void *out_e, const double *betas,
                      uint32_t num_sweeps, uint32_t repetitions, uint32_t replica_offset, uint32_t flags,
                      uint32_t known_flags);
// `elems` doubles of field cache in `cache`, or false: more than 32 GiB, or no memory — the cache is an
// optimisation, the launch runs without it.
bool field_cache_fits(DeviceBuffer<double> &cache, uint64_t elems);
int run_chains(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps, uint32_t repetitions,
               uint32_t replica_offset, uint64_t const *x0, bool descent, uint64_t *out_x, double *out_e,
               int64_t *out_trace = nullptr);
int greedy_relax(asp_sa_plan *p, uint32_t max_sweeps, std::vector<uint64_t> &x, uint64_t *out_x, double *out_e,
                 uint32_t *out_sweeps, bool exact_sweeps);

}  // namespace colour
}  // namespace asp
