// Consensus signs on gfx950 (law ASP-VOTE-1): align the configurations of a model up to
// the global flip and vote per site, for many models at once and for the configurations resident in
// chains handles.  Not in the reference, which keeps the chain of lowest energy and nothing else.
//
// One round is two launches over slot tables that cover every item of the call:
//
// k_vote_align: a workgroup of kThreads threads takes kWaves configurations of one item, a wavefront
// each.  The lanes stride over the words of x_r xor ref (64-bit popcounts, the last word's tail masked),
// the wavefront adds up, lane 0 stores d_r.  flip_r = align && 2 d_r > K is never stored: whoever needs
// it takes it from d_r.
//
// k_vote_sites: a workgroup takes kWaves word columns of one item, a wavefront each, a site per lane,
// and walks r = 0 .. R - 1.  The word x_r[w], d_r and w_r have wave-uniform addresses (the wavefront's
// index goes through readfirstlane): one fetch serves the 64 lanes.  The compiler issues them as flat vector
// loads all the same, because the pointers come out of the item table and are generic; they are not
// scalar loads yet.  A lane picks its bit and adds w_r to
// ONE of its two f64 accumulators — ascending r from +0.0, every add rounded on its own, nothing
// multiplied, so the bits depend on no launch choice.  Without weights nothing is summed in floating
// point: plus = ones and minus = R - ones are what the sums of 1.0 give, exactly (R <= 2^20).  The ballot
// of plus > minus (ties: the reference's bit) is the word of c, one store of lane 0.
//
// Round t reads the reference of buffer t & 1 (round 0: the caller's ref, or x[anchor] where it lies) and
// writes c into buffer (t + 1) & 1; the launches of all rounds are queued at once, with no host round
// trip in between, and a slot of an item with fewer rounds than the call's longest returns at once.  The
// per-site outputs and `changed` are written by an item's last round only.  `changed` is an integer
// atomic add of a word's popcount; there is no floating-point atomic anywhere.
// HBM per round: R W words of x twice (both passes), R (4 + 8) B per word column that stay in L2.
#include <cmath>
#include <cstring>
#include <vector>

#include "asp_common.hpp"
#include "sa_internal.hpp"

namespace {

using asp::DeviceBuffer;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // configurations of an alignment workgroup, word columns of a site
                                       // workgroup (tests/vote_cases.py: WAVES; 64 * kWaves sites: BLOCK)
constexpr uint64_t kMaxSpins = 1ull << 31;
constexpr uint32_t kMaxCount = 1u << 20;
constexpr uint32_t kMaxRounds = 16;

struct Item {  // device pointers
  const uint64_t *x;
  uint64_t x_stride;
  const double *weights;  // [count] or null
  const uint64_t *ref0;   // [words] the reference of round 0
  uint64_t *ref[2];       // [words] each: round t writes c into ref[(t + 1) & 1], round t + 1 reads it
  uint32_t *distance;     // [count]
  uint32_t *ones;         // [num_spins] or null
  double *plus, *minus;   // [num_spins] or null
  uint32_t *changed;      // [1], zero before the first launch
  uint32_t num_spins, count, words, align, rounds, pad;
};

struct Slot {
  uint32_t item, group;  // group: kWaves configurations (alignment) or kWaves word columns (sites)
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
  return v;
}

__device__ __forceinline__ const uint64_t *reference_of(const Item &it, uint32_t round) {
  return round == 0 ? it.ref0 : it.ref[round & 1u];
}

__global__ __launch_bounds__(kThreads) void k_vote_align(const Item *__restrict__ items,
                                                         const Slot *__restrict__ slots, uint32_t round) {
  const Slot slot = slots[blockIdx.x];
  const Item &it = items[slot.item];
  if (round >= it.rounds) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t r = slot.group * kWaves + wave;
  if (r >= it.count) return;  // (no barrier below)
  const uint32_t words = it.words, tail = it.num_spins & 63u;
  const uint64_t *__restrict__ x = it.x + static_cast<uint64_t>(r) * it.x_stride;
  const uint64_t *__restrict__ ref = reference_of(it, round);
  uint32_t d = 0;
  for (uint32_t w = lane; w < words; w += 64u) {
    uint64_t differ = x[w] ^ ref[w];
    if (w == words - 1u && tail) differ &= (1ull << tail) - 1ull;
    d += static_cast<uint32_t>(__builtin_popcountll(differ));
  }
  d = wave_sum_u32(d);
  if (lane == 0) it.distance[r] = d;
}

__global__ __launch_bounds__(kThreads) void k_vote_sites(const Item *__restrict__ items,
                                                         const Slot *__restrict__ slots, uint32_t round) {
  const Slot slot = slots[blockIdx.x];
  const Item &it = items[slot.item];
  if (round >= it.rounds) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w = slot.group * kWaves + wave;
  const uint32_t words = it.words;
  if (w >= words) return;  // (no barrier below)
  const uint32_t K = it.num_spins, R = it.count, align = it.align;
  const uint64_t stride = it.x_stride;
  const uint32_t left = K - w * 64u;  // sites of this column: 1 .. 64 and more
  const uint64_t mask = left < 64u ? (1ull << left) - 1ull : ~0ull;
  const uint64_t ref_word = reference_of(it, round)[w] & mask;
  const bool ref_bit = (ref_word >> lane) & 1ull;
  const uint64_t *__restrict__ x = it.x + w;
  const uint32_t *__restrict__ distance = it.distance;
  const double *__restrict__ weights = it.weights;

  uint32_t ones = 0;
  double plus = 0.0, minus = 0.0;
  if (!weights) {
#pragma unroll 4
    for (uint32_t r = 0; r < R; ++r) {
      const bool flip = align && 2ull * distance[r] > K;
      const uint64_t word = x[static_cast<uint64_t>(r) * stride] ^ (flip ? ~0ull : 0ull);
      ones += static_cast<uint32_t>((word >> lane) & 1ull);
    }
    plus = static_cast<double>(ones);
    minus = static_cast<double>(R - ones);
  } else {
#pragma unroll 4
    for (uint32_t r = 0; r < R; ++r) {
      const bool flip = align && 2ull * distance[r] > K;
      const uint64_t word = x[static_cast<uint64_t>(r) * stride] ^ (flip ? ~0ull : 0ull);
      const double weight = weights[r];
      const bool up = (word >> lane) & 1ull;
      ones += up ? 1u : 0u;
      const double grown_plus = __dadd_rn(plus, weight), grown_minus = __dadd_rn(minus, weight);
      plus = up ? grown_plus : plus;
      minus = up ? minus : grown_minus;
    }
  }
  const bool vote = plus > minus || (plus == minus && ref_bit);
  const uint64_t c = __ballot(vote) & mask;
  const bool last = round + 1u == it.rounds;
  if (lane == 0) {
    it.ref[(round + 1u) & 1u][w] = c;
    const uint32_t moved = static_cast<uint32_t>(__builtin_popcountll(c ^ ref_word));
    if (last && moved) atomicAdd(it.changed, moved);
  }
  const uint32_t site = w * 64u + lane;
  if (last && lane < left) {
    if (it.ones) it.ones[site] = ones;
    if (it.plus) it.plus[site] = plus;
    if (it.minus) it.minus[site] = minus;
  }
}

thread_local float g_last_ms = 0.0f;

inline uint64_t words_of(uint64_t num_spins) { return (num_spins + 63) / 64; }

// One item of a call, checked: x on the host (copied into the upload, packed to W words a configuration)
// or resident on the device with its stride.
struct Job {
  uint64_t num_spins = 0;
  uint32_t count = 0;
  const uint64_t *x = nullptr;
  uint64_t x_stride = 0;
  bool x_on_device = false;
  const double *weights = nullptr;
  const uint64_t *ref = nullptr;
  uint32_t anchor = 0, align = 0, rounds = 1;
  uint32_t *out_distance = nullptr;
  uint8_t *out_flipped = nullptr;
  uint32_t *out_ones = nullptr;
  double *out_plus = nullptr, *out_minus = nullptr;
  uint64_t *out_consensus = nullptr;
  uint32_t *out_changed = nullptr;
};

// The checks of everything but x (which a handle call takes from the handle).  `where` is "item N: ".
int check_vote(uint64_t num_spins, uint32_t count, const double *weights, const uint64_t *ref, uint32_t anchor,
               uint32_t rounds, const char *where) {
  if (num_spins >= kMaxSpins) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%s%llu spins: 2^31 or more", where, (unsigned long long)num_spins);
  }
  if (count > kMaxCount) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%s%u configurations: more than 2^20", where, count);
  }
  if (rounds < 1 || rounds > kMaxRounds) {
    return asp::set_error(ASP_ERR_INVALID, "%srounds = %u: 1 to %u", where, rounds, kMaxRounds);
  }
  if (count > 0 && !ref && anchor >= count) {
    return asp::set_error(ASP_ERR_INVALID, "%sanchor %u of %u configurations and no ref", where, anchor, count);
  }
  if (weights) {
    for (uint32_t r = 0; r < count; ++r) {
      if (!(weights[r] >= 0.0) || std::isinf(weights[r])) {
        return asp::set_error(ASP_ERR_INVALID, "%sweight %u is negative or not finite", where, r);
      }
    }
  }
  return ASP_OK;
}

int check_configurations(uint64_t num_spins, uint32_t count, const uint64_t *x, uint64_t x_stride,
                         const char *where) {
  const uint64_t W = words_of(num_spins);
  if (count > 0 && W > 0 && !x) return asp::set_error(ASP_ERR_INVALID, "%snull configurations", where);
  if (x_stride != 0 && x_stride < W) {
    return asp::set_error(ASP_ERR_INVALID, "%sx_stride %llu is below the %llu words of a configuration", where,
                          (unsigned long long)x_stride, (unsigned long long)W);
  }
  return ASP_OK;
}

// An item without spins: nothing to vote on.
void write_empty(const Job &j) {
  if (j.out_distance) std::memset(j.out_distance, 0, j.count * sizeof(uint32_t));
  if (j.out_flipped) std::memset(j.out_flipped, 0, j.count);
  if (j.out_changed) *j.out_changed = 0;
}

// Jobs with count > 0 and num_spins > 0, all checked: ONE upload (items, the two slot tables and every
// host array, 8-byte units), two launches a round of the longest item, one download; the stream is
// synchronised on return.
int run_votes(const std::vector<Job> &jobs, hipStream_t stream) {
  const size_t n = jobs.size();
  struct Place {
    size_t x, weights, ref;                                                  // in the upload
    size_t changed, ref_a, ref_b, distance, ones, plus, minus;  // in the download
  };
  std::vector<Place> place(n);
  size_t align_slots = 0, site_slots = 0;
  uint32_t rounds = 0;
  for (const Job &j : jobs) {
    align_slots += (static_cast<size_t>(j.count) + kWaves - 1) / kWaves;
    site_slots += (words_of(j.num_spins) + kWaves - 1) / kWaves;
    rounds = std::max(rounds, j.rounds);
  }
  if (align_slots > 0x7FFFFFFFull || site_slots > 0x7FFFFFFFull) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "2^31 workgroups or more in one call");
  }
  const size_t item_units = (n * sizeof(Item) + 7) / 8;  // (a Slot is 8 bytes)
  size_t in_units = item_units + align_slots + site_slots;
  size_t out_units = n;  // every item's `changed` first: the one part that is zeroed
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const size_t W = words_of(j.num_spins), K = j.num_spins;
    place[k].x = in_units;
    if (!j.x_on_device) in_units += static_cast<size_t>(j.count) * W;
    place[k].weights = in_units;
    if (j.weights) in_units += j.count;
    place[k].ref = in_units;
    if (j.ref) in_units += W;
    place[k].changed = k;
    place[k].ref_a = out_units;
    place[k].ref_b = out_units + W;
    out_units += 2 * W;
    place[k].distance = out_units;
    out_units += (static_cast<size_t>(j.count) + 1) / 2;
    place[k].ones = out_units;
    if (j.out_ones) out_units += (K + 1) / 2;
    place[k].plus = out_units;
    if (j.out_plus) out_units += K;
    place[k].minus = out_units;
    if (j.out_minus) out_units += K;
  }
  DeviceBuffer<uint64_t> d_in, d_out;
  std::vector<uint64_t> h_in(in_units, 0), h_out(out_units, 0);  // (before the fence: they outlive the copies)
  asp::StreamFence fence(stream);
  ASP_TRY(d_in.alloc(in_units));
  ASP_TRY(d_out.alloc(out_units));
  Item *items = reinterpret_cast<Item *>(h_in.data());
  Slot *align_slot = reinterpret_cast<Slot *>(h_in.data() + item_units);
  Slot *site_slot = align_slot + align_slots;
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const size_t W = words_of(j.num_spins);
    const uint64_t stride = j.x_stride ? j.x_stride : W;
    Item &it = items[k];
    if (j.x_on_device) {
      it.x = j.x;
      it.x_stride = stride;
    } else {
      it.x = d_in.ptr + place[k].x;
      it.x_stride = W;
      for (uint32_t c = 0; c < j.count; ++c) {
        std::memcpy(h_in.data() + place[k].x + static_cast<size_t>(c) * W, j.x + c * stride, W * 8);
      }
    }
    it.weights = j.weights ? reinterpret_cast<const double *>(d_in.ptr + place[k].weights) : nullptr;
    if (j.weights) std::memcpy(h_in.data() + place[k].weights, j.weights, j.count * sizeof(double));
    if (j.ref) {
      std::memcpy(h_in.data() + place[k].ref, j.ref, W * 8);
      it.ref0 = d_in.ptr + place[k].ref;
    } else {
      it.ref0 = it.x + static_cast<uint64_t>(j.anchor) * it.x_stride;
    }
    it.ref[0] = d_out.ptr + place[k].ref_a;
    it.ref[1] = d_out.ptr + place[k].ref_b;
    it.distance = reinterpret_cast<uint32_t *>(d_out.ptr + place[k].distance);
    it.ones = j.out_ones ? reinterpret_cast<uint32_t *>(d_out.ptr + place[k].ones) : nullptr;
    it.plus = j.out_plus ? reinterpret_cast<double *>(d_out.ptr + place[k].plus) : nullptr;
    it.minus = j.out_minus ? reinterpret_cast<double *>(d_out.ptr + place[k].minus) : nullptr;
    it.changed = reinterpret_cast<uint32_t *>(d_out.ptr + place[k].changed);
    it.num_spins = static_cast<uint32_t>(j.num_spins);
    it.count = j.count;
    it.words = static_cast<uint32_t>(W);
    it.align = j.align ? 1u : 0u;
    it.rounds = j.rounds;
    it.pad = 0;
    const uint32_t align_groups = (j.count + kWaves - 1) / kWaves;
    const uint32_t site_groups = static_cast<uint32_t>((W + kWaves - 1) / kWaves);
    for (uint32_t g = 0; g < align_groups; ++g) *align_slot++ = Slot{static_cast<uint32_t>(k), g};
    for (uint32_t g = 0; g < site_groups; ++g) *site_slot++ = Slot{static_cast<uint32_t>(k), g};
  }
  ASP_TRY(d_in.upload(h_in.data(), in_units, stream));
  ASP_HIP_TRY(hipMemsetAsync(d_out.ptr, 0, n * 8, stream));
  asp::EventPool events;
  hipEvent_t begin = nullptr, end = nullptr;
  ASP_TRY(events.make(&begin, true));
  ASP_TRY(events.make(&end, true));
  ASP_HIP_TRY(hipEventRecord(begin, stream));
  const Item *d_items = reinterpret_cast<const Item *>(d_in.ptr);
  const Slot *d_align = reinterpret_cast<const Slot *>(d_in.ptr + item_units);
  const Slot *d_site = d_align + align_slots;
  for (uint32_t round = 0; round < rounds; ++round) {
    hipLaunchKernelGGL(k_vote_align, dim3(static_cast<unsigned>(align_slots)), dim3(kThreads), 0, stream, d_items,
                       d_align, round);
    ASP_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vote_sites, dim3(static_cast<unsigned>(site_slots)), dim3(kThreads), 0, stream, d_items,
                       d_site, round);
    ASP_HIP_TRY(hipGetLastError());
  }
  ASP_HIP_TRY(hipEventRecord(end, stream));
  ASP_TRY(d_out.download(h_out.data(), out_units, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  (void)hipEventElapsedTime(&g_last_ms, begin, end);
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const size_t W = words_of(j.num_spins), K = j.num_spins;
    const uint32_t *distance = reinterpret_cast<const uint32_t *>(h_out.data() + place[k].distance);
    if (j.out_distance) std::memcpy(j.out_distance, distance, j.count * sizeof(uint32_t));
    if (j.out_flipped) {
      for (uint32_t r = 0; r < j.count; ++r) j.out_flipped[r] = j.align && 2ull * distance[r] > K ? 1 : 0;
    }
    if (j.out_ones) std::memcpy(j.out_ones, h_out.data() + place[k].ones, K * sizeof(uint32_t));
    if (j.out_plus) std::memcpy(j.out_plus, h_out.data() + place[k].plus, K * sizeof(double));
    if (j.out_minus) std::memcpy(j.out_minus, h_out.data() + place[k].minus, K * sizeof(double));
    if (j.out_consensus) {
      std::memcpy(j.out_consensus, h_out.data() + (j.rounds & 1u ? place[k].ref_b : place[k].ref_a), W * 8);
    }
    if (j.out_changed) *j.out_changed = static_cast<uint32_t>(h_out[place[k].changed]);
  }
  return ASP_OK;
}

void outputs_of(const asp_sign_vote_item &a, Job *job) {
  job->out_distance = a.out_distance;
  job->out_flipped = a.out_flipped;
  job->out_ones = a.out_ones;
  job->out_plus = a.out_plus;
  job->out_minus = a.out_minus;
  job->out_consensus = a.out_consensus;
  job->out_changed = a.out_changed;
}

}  // namespace

extern "C" float asp_sign_vote_last_ms(void) { return g_last_ms; }

extern "C" int asp_sign_vote_batch(asp_sign_vote_item const *items, uint32_t count) {
  asp_clear_error();
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  std::vector<Job> jobs, empty;
  jobs.reserve(count);
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sign_vote_item &a = items[i];
    char where[32];
    std::snprintf(where, sizeof where, "item %u: ", i);
    ASP_TRY(check_vote(a.num_spins, a.count, a.weights, a.ref, a.anchor, a.rounds, where));
    ASP_TRY(check_configurations(a.num_spins, a.count, a.x, a.x_stride, where));
    if (a.count == 0) continue;
    Job job;
    job.num_spins = a.num_spins;
    job.count = a.count;
    job.x = a.x;
    job.x_stride = a.x_stride;
    job.weights = a.weights;
    job.ref = a.ref;
    job.anchor = a.anchor;
    job.align = a.align;
    job.rounds = a.rounds;
    outputs_of(a, &job);
    (a.num_spins == 0 ? empty : jobs).push_back(job);
  }
  if (!jobs.empty()) {
    ASP_TRY(asp::require_device());
    asp::ScopedStream scoped;
    ASP_TRY(scoped.acquire());
    ASP_TRY(run_votes(jobs, scoped.stream));
  }
  for (const Job &j : empty) write_empty(j);
  return ASP_OK;
}

extern "C" int asp_sa_chains_vote_batch(asp_sa_chains_vote_item const *items, uint32_t count) {
  asp_clear_error();
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  std::vector<Job> jobs, empty;
  std::vector<asp_sa_plan *> plans;  // of the jobs that run, each once
  jobs.reserve(count);
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_vote_item &a = items[i];
    if (!a.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    if (a.which > 1) return asp::set_error(ASP_ERR_INVALID, "item %u: which = %u: 0 (best) or 1 (current)", i, a.which);
    const asp_sa_chains *c = a.chains;
    char where[32];
    std::snprintf(where, sizeof where, "item %u: ", i);
    ASP_TRY(check_vote(c->plan->host.num_spins, c->repetitions, a.weights, a.ref, a.anchor, a.rounds, where));
    if (c->repetitions == 0) continue;
    Job job;
    job.num_spins = c->plan->host.num_spins;
    job.count = c->repetitions;
    job.x = a.which == 0 ? c->x_best.ptr : c->x_cur.ptr;
    job.x_stride = c->words;
    job.x_on_device = true;
    job.weights = a.weights;
    job.ref = a.ref;
    job.anchor = a.anchor;
    job.align = a.align;
    job.rounds = a.rounds;
    job.out_distance = a.out_distance;
    job.out_flipped = a.out_flipped;
    job.out_ones = a.out_ones;
    job.out_plus = a.out_plus;
    job.out_minus = a.out_minus;
    job.out_consensus = a.out_consensus;
    job.out_changed = a.out_changed;
    if (job.num_spins == 0) {
      empty.push_back(job);
      continue;
    }
    jobs.push_back(job);
    if (std::find(plans.begin(), plans.end(), c->plan) == plans.end()) plans.push_back(c->plan);
  }
  if (!jobs.empty()) {
    ASP_TRY(asp::bind_device());
    if (plans.size() == 1) {
      // the plan's stream: every call that writes the handle's configurations runs on it
      ASP_TRY(run_votes(jobs, plans[0]->stream));
    } else {
      // a stream of the call, which runs after what is pending on the plans' streams (a stream with
      // nothing pending — the usual case: every entry point waits for its stream — needs no event)
      asp::ScopedStream batch;
      ASP_TRY(batch.acquire());
      for (asp_sa_plan *p : plans) {
        const hipError_t pending = hipStreamQuery(p->stream);
        if (pending == hipSuccess) continue;
        if (pending != hipErrorNotReady) ASP_HIP_TRY(pending);
        ASP_HIP_TRY(hipEventRecord(p->ev[0], p->stream));
        ASP_HIP_TRY(hipStreamWaitEvent(batch.stream, p->ev[0], 0));
      }
      ASP_TRY(run_votes(jobs, batch.stream));
    }
  }
  for (const Job &j : empty) write_empty(j);
  return ASP_OK;
}
