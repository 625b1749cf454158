// Sign scores on gfx950 (specification ASP-SCORE-1): what the reference's
//   compute_accuracy_and_overlap                  common.py:211-229   (numpy, one configuration)
// computes, for many configurations of many models at once, for the configurations resident in a
// chains handle, and the matrix of Hamming distances between configurations.
//
// k_sign_scores: one workgroup of kPass threads per (item, configuration) and one more per item for the
// total of its weights.  A pass takes kPass consecutive positions, one per lane (weights coalesced, the
// bit through `select`, or from the XOR word of x and exact, which the 64 lanes of a wavefront share).
// The sum is the pairwise tree of the specification and nothing else: __shfl_down with offsets 1, 2, ...
// 32 IN THAT ORDER inside the wavefront, strides 64 and 128 over the wavefronts' values in LDS, and the
// pass partials merged like a binary counter (partial p is merged with the waiting partial of every
// trailing one bit of p), folded from the lowest level at the end.  No floating-point atomics, no
// multiplication: the bits depend on no launch choice.  Without weights nothing is summed in floating
// point at all: signed = 2 matches - K0 and total = K0 are what the tree of +-1.0 gives, exactly.
// HBM per configuration: W words of x, and K0 * 8 B of weights (+ 4 B of select) that stay in L2 over the
// configurations of an item.
//
// k_sign_distances: one workgroup per kTile x kTile tile of pairs with tile row <= tile column, a 4 x 4
// sub-tile per lane; the two tiles' words staged in LDS kChunk words at a time ([word][row], so a lane's
// four rows are one 32-byte read), the last word's tail masked while staging; 64-bit popcounts; the
// mirror tile written from the same registers.
#include <cmath>
#include <cstring>
#include <vector>

#include "asp_common.hpp"
#include "sa_internal.hpp"

namespace {

using asp::DeviceBuffer;

constexpr int kPass = 256;  // positions of one pass = threads of a workgroup (tests/score_cases.py: PASS)
constexpr int kWaves = kPass / 64;
constexpr int kLevels = 32;  // pass partials waiting: K0 < 2^31 is fewer than 2^23 passes
constexpr int kTile = 64;    // pairs per side of a distance tile (score_cases.py: TILE)
constexpr int kChunk = 16;   // words staged per round (score_cases.py: CHUNK)
constexpr int kRowPad = 2;   // u64 between two words' rows in LDS (keeps 16-byte alignment)
constexpr uint64_t kMaxScored = 1ull << 31;
constexpr uint32_t kMaxDistanceCount = 32768;

struct Item {  // device pointers
  const uint64_t *x;
  uint64_t x_stride;
  const int32_t *select;
  const uint64_t *exact;
  const double *weights;
  unsigned long long *out_matches;  // [count]
  double *out_signed;               // [count]
  double *out_total;                // [1]
  uint64_t num_spins, num_scored;
  uint32_t count;
};

struct Slot {
  uint32_t item, config;  // config == count: the item's total
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
  return v;
}

__global__ __launch_bounds__(kPass) void k_sign_scores(const Item *__restrict__ items,
                                                      const Slot *__restrict__ slots) {
  __shared__ double part[2][kWaves];
  __shared__ double waiting[kLevels];
  __shared__ uint32_t counted[kWaves];
  const Slot slot = slots[blockIdx.x];
  const Item it = items[slot.item];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t K0 = static_cast<uint32_t>(it.num_scored);
  const bool total = slot.config == it.count;
  const uint64_t *__restrict__ x = total ? nullptr : it.x + static_cast<uint64_t>(slot.config) * it.x_stride;

  if (!it.weights) {
    if (total) {
      if (t == 0) *it.out_total = static_cast<double>(K0);
      return;
    }
    uint32_t mine = 0;
    if (it.select) {
      for (uint32_t i = t; i < K0; i += kPass) {
        const uint32_t j = static_cast<uint32_t>(it.select[i]);
        const uint64_t g = (x[j >> 6] >> (j & 63u)) & 1ull, e = (it.exact[i >> 6] >> (i & 63u)) & 1ull;
        mine += g == e ? 1u : 0u;
      }
    } else {
      const uint32_t words = (K0 + 63u) >> 6;
      for (uint32_t w = t; w < words; w += kPass) {
        uint64_t same = ~(x[w] ^ it.exact[w]);
        if (w == words - 1 && (K0 & 63u)) same &= (1ull << (K0 & 63u)) - 1ull;
        mine += static_cast<uint32_t>(__builtin_popcountll(same));
      }
    }
    mine = wave_sum_u32(mine);
    if (lane == 0) counted[wave] = mine;
    __syncthreads();
    if (t == 0) {
      uint32_t m = 0;
      for (int k = 0; k < kWaves; ++k) m += counted[k];
      it.out_matches[slot.config] = m;
      it.out_signed[slot.config] = static_cast<double>(2ll * static_cast<long long>(m) - static_cast<long long>(K0));
    }
    return;
  }

  const uint32_t passes = (K0 + kPass - 1) / kPass;
  uint32_t mine = 0;  // matches this lane saw (select), or lane 0 counted from whole words (no select)
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t i = p * kPass + t;
    double v = 0.0;
    if (total) {
      if (i < K0) v = it.weights[i];
    } else if (it.select) {
      if (i < K0) {
        const uint32_t j = static_cast<uint32_t>(it.select[i]);
        const uint64_t g = (x[j >> 6] >> (j & 63u)) & 1ull, e = (it.exact[i >> 6] >> (i & 63u)) & 1ull;
        const double w = it.weights[i];
        mine += g == e ? 1u : 0u;
        v = g == e ? w : -w;
      }
    } else {
      const uint32_t w0 = i >> 6;  // the wavefront's word: i - lane is a multiple of 64
      if (static_cast<uint64_t>(w0) * 64 < K0) {
        uint64_t same = ~(x[w0] ^ it.exact[w0]);
        const uint32_t left = K0 - w0 * 64;
        if (left < 64) same &= (1ull << left) - 1ull;
        if (lane == 0) mine += static_cast<uint32_t>(__builtin_popcountll(same));
        if (i < K0) {
          const double w = it.weights[i];
          v = (same >> lane) & 1ull ? w : -w;
        }
      }
    }
    // levels 1 .. 6 of the tree: after the step with offset s every lane that is a multiple of 2s holds
    // the node above it (the other lanes hold values nobody reads)
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = __dadd_rn(v, __shfl_down(v, s, 64));
    if (lane == 0) part[p & 1u][wave] = v;
    __syncthreads();  // (one barrier per pass: the next pass writes the other half of `part`)
    if (t == 0) {
      const double *q = part[p & 1u];
      double node = __dadd_rn(__dadd_rn(q[0], q[1]), __dadd_rn(q[2], q[3]));  // strides 64, then 128
      uint32_t level = 0;
      while ((p >> level) & 1u) {
        node = __dadd_rn(waiting[level], node);
        ++level;
      }
      waiting[level] = node;
    }
  }
  if (!total) {
    mine = wave_sum_u32(mine);
    if (lane == 0) counted[wave] = mine;
    __syncthreads();
  }
  if (t == 0) {
    // what is left, from the lowest level up: the node of a set bit is the left child, what was folded
    // so far the right one; where the bit is clear the right child is padding (+0.0: nothing to add)
    double sum = 0.0;
    bool any = false;
    for (uint32_t level = 0; level < kLevels; ++level) {
      if (!((passes >> level) & 1u)) continue;
      sum = any ? __dadd_rn(waiting[level], sum) : waiting[level];
      any = true;
    }
    if (total) {
      *it.out_total = sum;
    } else {
      uint32_t m = 0;
      for (int k = 0; k < kWaves; ++k) m += counted[k];
      it.out_matches[slot.config] = m;
      it.out_signed[slot.config] = sum;
    }
  }
}

// Tile (blockIdx.y, blockIdx.x) of the pairs, rows a of the first and b of the second; lane (ty, tx)
// holds rows 4 ty .. 4 ty + 3 against 4 tx .. 4 tx + 3.
__global__ __launch_bounds__(256) void k_sign_distances(const uint64_t *__restrict__ x, uint64_t x_stride,
                                                       uint32_t count, uint32_t words, uint32_t tail_bits,
                                                       uint32_t *__restrict__ out) {
  if (blockIdx.y > blockIdx.x) return;  // the mirror is written by the tile above the diagonal
  __shared__ __attribute__((aligned(16))) uint64_t tile_a[kChunk][kTile + kRowPad];
  __shared__ __attribute__((aligned(16))) uint64_t tile_b[kChunk][kTile + kRowPad];
  const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
  const uint32_t a0 = blockIdx.y * kTile, b0 = blockIdx.x * kTile;
  const uint64_t tail_mask = tail_bits ? (1ull << tail_bits) - 1ull : ~0ull;
  uint32_t d[4][4] = {};
  for (uint32_t w0 = 0; w0 < words; w0 += kChunk) {
    // stage: 16 consecutive lanes read 16 consecutive words of one row
    const uint32_t k = t & (kChunk - 1), w = w0 + k;
    for (uint32_t r = t / kChunk; r < kTile; r += 256 / kChunk) {
      uint64_t va = 0, vb = 0;
      if (w < words) {
        const uint64_t mask = w == words - 1 ? tail_mask : ~0ull;
        if (a0 + r < count) va = x[static_cast<uint64_t>(a0 + r) * x_stride + w] & mask;
        if (b0 + r < count) vb = x[static_cast<uint64_t>(b0 + r) * x_stride + w] & mask;
      }
      tile_a[k][r] = va;
      tile_b[k][r] = vb;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t kk = 0; kk < kChunk; ++kk) {
      uint64_t a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = tile_a[kk][4 * ty + r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = tile_b[kk][4 * tx + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) d[r][c] += static_cast<uint32_t>(__builtin_popcountll(a[r] ^ b[c]));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t a = a0 + 4 * ty + r;
    if (a >= count) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t b = b0 + 4 * tx + c;
      if (b >= count) continue;
      out[static_cast<uint64_t>(a) * count + b] = d[r][c];
      out[static_cast<uint64_t>(b) * count + a] = d[r][c];
    }
  }
}

thread_local float g_last_ms = 0.0f;

struct Timer {
  hipEvent_t begin = nullptr, end = nullptr;
  hipStream_t stream = nullptr;
  ~Timer() {
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
  int start(hipStream_t s) {
    stream = s;
    ASP_HIP_TRY(hipEventCreate(&begin));
    ASP_HIP_TRY(hipEventCreate(&end));
    ASP_HIP_TRY(hipEventRecord(begin, stream));
    return ASP_OK;
  }
  int mark() {
    ASP_HIP_TRY(hipEventRecord(end, stream));
    return ASP_OK;
  }
  // after the stream was synchronised
  void read() { (void)hipEventElapsedTime(&g_last_ms, begin, end); }
};

inline uint64_t words_of(uint64_t num_spins) { return (num_spins + 63) / 64; }

// K0 of an item; the checks of everything but x (which a handle call takes from the handle).  `where`
// is "" or "item N: ".
int check_scored(uint64_t num_spins, uint64_t num_scored, const int32_t *select, const uint64_t *exact,
                 const double *weights, const char *where, uint64_t *scored_out) {
  const uint64_t K0 = select ? num_scored : num_spins;
  if (K0 >= kMaxScored) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%s%llu scored positions: 2^31 or more", where, (unsigned long long)K0);
  }
  if (K0 > 0 && !exact) return asp::set_error(ASP_ERR_INVALID, "%snull exact signs", where);
  if (select) {
    for (uint64_t i = 0; i < K0; ++i) {
      if (select[i] < 0 || static_cast<uint64_t>(select[i]) >= num_spins) {
        return asp::set_error(ASP_ERR_INVALID, "%sselect[%llu] = %d is outside [0, %llu)", where,
                              (unsigned long long)i, select[i], (unsigned long long)num_spins);
      }
    }
  }
  if (weights) {
    for (uint64_t i = 0; i < K0; ++i) {
      if (!(weights[i] >= 0.0) || std::isinf(weights[i])) {
        return asp::set_error(ASP_ERR_INVALID, "%sweight %llu is negative or not finite", where,
                              (unsigned long long)i);
      }
    }
  }
  *scored_out = K0;
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

// One model of a scoring call: x on the host (x_on_device false: copied into the upload, packed to W
// words a configuration) or resident on the device with its stride.
struct Job {
  uint64_t num_spins = 0, num_scored = 0;
  uint32_t count = 0;
  const uint64_t *x = nullptr;
  uint64_t x_stride = 0;
  bool x_on_device = false;
  const int32_t *select = nullptr;
  const uint64_t *exact = nullptr;
  const double *weights = nullptr;
  uint64_t *out_matches = nullptr;
  double *out_signed = nullptr, *out_total = nullptr;
};

// Jobs with count > 0, all checked: ONE upload (items, slots and every host array, 8-byte units), one
// launch, one download; the stream is synchronised on return.
int run_scores(const std::vector<Job> &jobs, hipStream_t stream) {
  const size_t n = jobs.size();
  struct Place {
    size_t x, select, exact, weights, out;
  };
  std::vector<Place> place(n);
  size_t slots = 0;
  for (const Job &j : jobs) slots += static_cast<size_t>(j.count) + 1;
  if (slots > 0x7FFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "2^31 configurations or more in one call");
  const size_t item_units = (n * sizeof(Item) + 7) / 8, slot_units = slots;  // (a Slot is 8 bytes)
  size_t in_units = item_units + slot_units, out_units = 0;
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const size_t W = words_of(j.num_spins), K0 = j.num_scored;
    place[k].x = in_units;
    if (!j.x_on_device) in_units += static_cast<size_t>(j.count) * W;
    place[k].select = in_units;
    if (j.select) in_units += (K0 + 1) / 2;
    place[k].exact = in_units;
    in_units += words_of(K0);
    place[k].weights = in_units;
    if (j.weights) in_units += K0;
    place[k].out = out_units;
    out_units += 2 * static_cast<size_t>(j.count) + 1;
  }
  DeviceBuffer<uint64_t> d_in, d_out;
  std::vector<uint64_t> h_in(in_units, 0), h_out(out_units, 0);  // (before the fence: they outlive the copies)
  asp::StreamFence fence(stream);
  ASP_TRY(d_in.alloc(in_units));
  ASP_TRY(d_out.alloc(out_units));
  Item *items = reinterpret_cast<Item *>(h_in.data());
  Slot *slot = reinterpret_cast<Slot *>(h_in.data() + item_units);
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const size_t W = words_of(j.num_spins), K0 = j.num_scored;
    const uint64_t stride = j.x_stride ? j.x_stride : W;
    Item &it = items[k];
    if (j.x_on_device) {
      it.x = j.x;
      it.x_stride = stride;
    } else {
      it.x = d_in.ptr + place[k].x;
      it.x_stride = W;
      for (uint32_t c = 0; c < j.count && W; ++c) {
        std::memcpy(h_in.data() + place[k].x + c * W, j.x + c * stride, W * 8);
      }
    }
    it.select = j.select ? reinterpret_cast<const int32_t *>(d_in.ptr + place[k].select) : nullptr;
    if (j.select && K0) std::memcpy(h_in.data() + place[k].select, j.select, K0 * sizeof(int32_t));
    it.exact = d_in.ptr + place[k].exact;
    if (K0) std::memcpy(h_in.data() + place[k].exact, j.exact, words_of(K0) * 8);
    it.weights = j.weights ? reinterpret_cast<const double *>(d_in.ptr + place[k].weights) : nullptr;
    if (j.weights && K0) std::memcpy(h_in.data() + place[k].weights, j.weights, K0 * sizeof(double));
    it.out_matches = reinterpret_cast<unsigned long long *>(d_out.ptr + place[k].out);
    it.out_signed = reinterpret_cast<double *>(d_out.ptr + place[k].out + j.count);
    it.out_total = reinterpret_cast<double *>(d_out.ptr + place[k].out + 2 * static_cast<size_t>(j.count));
    it.num_spins = j.num_spins;
    it.num_scored = K0;
    it.count = j.count;
    for (uint32_t c = 0; c <= j.count; ++c) *slot++ = Slot{static_cast<uint32_t>(k), c};
  }
  ASP_TRY(d_in.upload(h_in.data(), in_units, stream));
  Timer timer;
  ASP_TRY(timer.start(stream));
  hipLaunchKernelGGL(k_sign_scores, dim3(static_cast<unsigned>(slots)), dim3(kPass), 0, stream,
                     reinterpret_cast<const Item *>(d_in.ptr), reinterpret_cast<const Slot *>(d_in.ptr + item_units));
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(timer.mark());
  ASP_TRY(d_out.download(h_out.data(), out_units, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  timer.read();
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[k];
    const uint64_t *o = h_out.data() + place[k].out;
    if (j.out_matches) std::memcpy(j.out_matches, o, j.count * 8ull);
    if (j.out_signed) std::memcpy(j.out_signed, o + j.count, j.count * 8ull);
    if (j.out_total) std::memcpy(j.out_total, o + 2 * static_cast<size_t>(j.count), 8);
  }
  return ASP_OK;
}

int check_distances(uint64_t num_spins, uint32_t count) {
  if (count > kMaxDistanceCount) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "%u configurations: the distance matrix takes at most %u", count,
                          kMaxDistanceCount);
  }
  if (num_spins >= (1ull << 32)) return asp::set_error(ASP_ERR_TOO_LARGE, "2^32 spins or more");
  return ASP_OK;
}

// x on the device; out on the host.  The stream is synchronised on return.
int run_distances(uint64_t num_spins, uint32_t count, const uint64_t *d_x, uint64_t x_stride, uint32_t *out,
                  hipStream_t stream) {
  DeviceBuffer<uint32_t> d_out;
  asp::StreamFence fence(stream);
  const size_t cells = static_cast<size_t>(count) * count;
  ASP_TRY(d_out.alloc(cells));
  const unsigned tiles = (count + kTile - 1) / kTile;
  Timer timer;
  ASP_TRY(timer.start(stream));
  hipLaunchKernelGGL(k_sign_distances, dim3(tiles, tiles), dim3(256), 0, stream, d_x, x_stride, count,
                     static_cast<uint32_t>(words_of(num_spins)), static_cast<uint32_t>(num_spins & 63u), d_out.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(timer.mark());
  ASP_TRY(d_out.download(out, cells, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  timer.read();
  return ASP_OK;
}

int job_of(const asp_sign_scores_item &a, const char *where, Job *job) {
  ASP_TRY(check_configurations(a.num_spins, a.count, a.x, a.x_stride, where));
  uint64_t K0 = 0;
  ASP_TRY(check_scored(a.num_spins, a.num_scored, a.select, a.exact, a.weights, where, &K0));
  job->num_spins = a.num_spins;
  job->num_scored = K0;
  job->count = a.count;
  job->x = a.x;
  job->x_stride = a.x_stride;
  job->select = a.select;
  job->exact = a.exact;
  job->weights = a.weights;
  job->out_matches = a.out_matches;
  job->out_signed = a.out_signed;
  job->out_total = a.out_total;
  return ASP_OK;
}

int run_host_jobs(const std::vector<Job> &jobs) {
  if (jobs.empty()) return ASP_OK;
  ASP_TRY(asp::require_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  return run_scores(jobs, scoped.stream);
}

}  // namespace

extern "C" float asp_sign_scores_last_ms(void) { return g_last_ms; }

extern "C" int asp_sign_scores(uint64_t num_spins, uint32_t count, uint64_t const *x, uint64_t x_stride,
                               uint64_t num_scored, int32_t const *select, uint64_t const *exact,
                               double const *weights, uint64_t *out_matches, double *out_signed,
                               double *out_total) {
  asp_clear_error();
  const asp_sign_scores_item item{num_spins, count,   x,           x_stride,   num_scored, select,
                                  exact,     weights, out_matches, out_signed, out_total};
  std::vector<Job> jobs(1);
  ASP_TRY(job_of(item, "", &jobs[0]));
  if (count == 0) return ASP_OK;
  return run_host_jobs(jobs);
}

extern "C" int asp_sign_scores_batch(asp_sign_scores_item const *items, uint32_t count) {
  asp_clear_error();
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  std::vector<Job> jobs;
  jobs.reserve(count);
  for (uint32_t i = 0; i < count; ++i) {
    char where[32];
    std::snprintf(where, sizeof where, "item %u: ", i);
    Job job;
    ASP_TRY(job_of(items[i], where, &job));
    if (job.count > 0) jobs.push_back(job);
  }
  return run_host_jobs(jobs);
}

extern "C" int asp_sign_distances(uint64_t num_spins, uint32_t count, uint64_t const *x, uint64_t x_stride,
                                  uint32_t *out) {
  asp_clear_error();
  ASP_TRY(check_distances(num_spins, count));
  ASP_TRY(check_configurations(num_spins, count, x, x_stride, ""));
  if (count > 0 && !out) return asp::set_error(ASP_ERR_INVALID, "null output");
  if (count == 0) return ASP_OK;
  ASP_TRY(asp::require_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  const uint64_t W = words_of(num_spins), stride = x_stride ? x_stride : W;
  DeviceBuffer<uint64_t> d_x;
  std::vector<uint64_t> packed;  // (declared before the fence: it outlives the asynchronous copy)
  asp::StreamFence fence(scoped.stream);
  ASP_TRY(d_x.alloc(static_cast<size_t>(count) * W));
  if (stride == W) {
    ASP_TRY(d_x.upload(x, static_cast<size_t>(count) * W, scoped.stream));
  } else {
    packed.resize(static_cast<size_t>(count) * W);
    for (uint32_t r = 0; r < count; ++r) std::memcpy(packed.data() + r * W, x + r * stride, W * 8);
    ASP_TRY(d_x.upload(packed.data(), packed.size(), scoped.stream));
  }
  return run_distances(num_spins, count, d_x.ptr, W, out, scoped.stream);
}

extern "C" int asp_sa_chains_scores(asp_sa_chains *c, uint32_t which, uint64_t num_scored, int32_t const *select,
                                    uint64_t const *exact, double const *weights, uint64_t *out_matches,
                                    double *out_signed, double *out_total) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (which > 1) return asp::set_error(ASP_ERR_INVALID, "which = %u: 0 (best) or 1 (current)", which);
  std::vector<Job> jobs(1);
  Job &job = jobs[0];
  job.num_spins = c->plan->host.num_spins;
  ASP_TRY(check_scored(job.num_spins, num_scored, select, exact, weights, "", &job.num_scored));
  if (c->repetitions == 0) return ASP_OK;
  job.count = c->repetitions;
  job.x = which == 0 ? c->x_best.ptr : c->x_cur.ptr;
  job.x_stride = c->words;
  job.x_on_device = true;
  job.select = select;
  job.exact = exact;
  job.weights = weights;
  job.out_matches = out_matches;
  job.out_signed = out_signed;
  job.out_total = out_total;
  ASP_TRY(asp::bind_device());
  // the plan's stream: every call that writes the handle's configurations runs on it
  return run_scores(jobs, c->plan->stream);
}

extern "C" int asp_sa_chains_distances(asp_sa_chains *c, uint32_t which, uint32_t *out) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  if (which > 1) return asp::set_error(ASP_ERR_INVALID, "which = %u: 0 (best) or 1 (current)", which);
  const uint64_t K = c->plan->host.num_spins;
  ASP_TRY(check_distances(K, c->repetitions));
  if (c->repetitions == 0) return ASP_OK;
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output");
  ASP_TRY(asp::bind_device());
  return run_distances(K, c->repetitions, which == 0 ? c->x_best.ptr : c->x_cur.ptr, c->words, out,
                       c->plan->stream);
}
