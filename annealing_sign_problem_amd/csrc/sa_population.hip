// Population annealing on resumable chains (include/asp.h section 4, DESIGN.md §4.11, law "ASP-PA-1"):
// between two temperatures the chains of a handle are reweighted by exp(-dbeta E) and resampled on the
// device — reported energies of the current configurations (the plan's energy kernels), weights as
// 31-bit integers, one Philox draw, systematic resampling by binary search over the integer prefix
// sums, and a gather of all five state arrays into the handle's second set of buffers, which is then
// swapped in.  Many handles share the selection and the gather launches.  After the weights everything
// is integer arithmetic: no reduction order can change a result.  gfx950 only.
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

constexpr uint32_t kMaxChains = 65536;  // R T <= 2^16 2^16 2^31 = 2^63: every product of the law fits 64 bits
constexpr uint32_t kThreads = 256;

// Row i of the selection table describes live handle i (chains and spins): its chains own entries
// [at, at + chains) of the planes of `total` entries each.
struct SelectRow {
  const double *energy;  // [chains] reported energies of the current configurations
  uint64_t seed;
  double dbeta;
  uint64_t at;
  uint32_t chains, sweeps_done, draw;
};

// Steps 2-5 of ASP-PA-1, a workgroup per handle.  planes: energy[total] | q[total] (64-bit words, what
// the host reads back); prefix[total]: scratch, the INCLUSIVE prefix sums C_{s+1}.
__global__ __launch_bounds__(kThreads) void k_population_select(const SelectRow *table, uint64_t total,
                                                                uint64_t *__restrict__ planes,
                                                                uint64_t *__restrict__ prefix,
                                                                uint32_t *__restrict__ source,
                                                                uint32_t *__restrict__ survivors) {
  const SelectRow row = table[blockIdx.x];
  const uint32_t R = row.chains, tid = threadIdx.x;
  __shared__ double s_min[kThreads];
  __shared__ uint64_t s_sum[kThreads];
  __shared__ uint32_t s_distinct;
  if (tid == 0) s_distinct = 0;
  double lowest = INFINITY;
  for (uint32_t r = tid; r < R; r += kThreads) {
    const double e = row.energy[r];
    lowest = e < lowest ? e : lowest;
  }
  s_min[tid] = lowest;
  __syncthreads();
  for (uint32_t step = kThreads / 2; step != 0; step >>= 1) {
    if (tid < step && s_min[tid + step] < s_min[tid]) s_min[tid] = s_min[tid + step];
    __syncthreads();
  }
  const double e_min = s_min[0];
  // thread t owns the chains [t per, (t + 1) per): their q, then the scan of the 256 segment sums
  const uint32_t per = (R + kThreads - 1) / kThreads;
  const uint32_t first = tid * per < R ? tid * per : R;
  const uint32_t last = first + per < R ? first + per : R;
  uint64_t sum = 0;
  for (uint32_t r = first; r < last; ++r) {
    const double e = row.energy[r];
    const double w = expneg(__dmul_rn(row.dbeta, __dadd_rn(e, -e_min)));
    const uint64_t q = static_cast<uint64_t>(__dmul_rn(w, 0x1p31));  // exact scaling, 0 <= w <= 1
    planes[row.at + r] = static_cast<uint64_t>(__double_as_longlong(e));
    planes[total + row.at + r] = q;
    sum += q;
  }
  s_sum[tid] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    const uint64_t add = tid >= d ? s_sum[tid - d] : 0ull;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  const uint64_t T = s_sum[kThreads - 1];
  uint64_t running = s_sum[tid] - sum;
  for (uint32_t r = first; r < last; ++r) {
    running += planes[total + row.at + r];
    prefix[row.at + r] = running;
  }
  __syncthreads();
  const Philox4 rnd = philox4x32_10(row.sweeps_done, row.draw, 0xFFFFFFFDu, 0u, static_cast<uint32_t>(row.seed),
                                    static_cast<uint32_t>(row.seed >> 32));
  const uint64_t U = __umul64hi(static_cast<uint64_t>(rnd.w[0]) << 32, T);  // floor(v T / 2^32) < T
  for (uint32_t j = tid; j < R; j += kThreads) {
    const uint64_t key = static_cast<uint64_t>(j) * T + U;
    // the number of s with R C_{s+1} <= key: the unique s with R C_s <= key < R C_{s+1}
    uint32_t lo = 0, hi = R;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (static_cast<uint64_t>(R) * prefix[row.at + mid] <= key) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    // (key < R T, so lo < R; energies that are not numbers leave T = 0: stay inside the handle)
    source[row.at + j] = lo < R ? lo : R - 1;
  }
  __syncthreads();
  uint32_t distinct = 0;
  for (uint32_t j = tid; j < R; j += kThreads) {
    distinct += (j == 0 || source[row.at + j] != source[row.at + j - 1]) ? 1u : 0u;  // (source is sorted)
  }
  if (distinct) atomicAdd(&s_distinct, distinct);
  __syncthreads();
  if (tid == 0) survivors[blockIdx.x] = s_distinct;
}

// Step 6: slot j of every state array becomes slot source[at + j], read from the handle's arrays and
// written to its second set (a copy in place would overwrite rows that are still to be read).
struct GatherRow {
  const uint64_t *x_cur, *x_best;
  uint64_t *x_cur_to, *x_best_to;
  const long long *e_cur, *e_best;
  long long *e_cur_to, *e_best_to;
  const unsigned long long *accepted;
  unsigned long long *accepted_to;
  uint64_t at;
  uint32_t chains, words;
};

// blockIdx.x: handle; blockIdx.y strides over (destination chain, word), consecutive lanes along a row.
__global__ __launch_bounds__(kThreads) void k_population_gather_words(const GatherRow *table,
                                                                      const uint32_t *__restrict__ source) {
  const GatherRow row = table[blockIdx.x];
  const uint64_t n = static_cast<uint64_t>(row.chains) * row.words;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.y) * kThreads + threadIdx.x; k < n;
       k += static_cast<uint64_t>(gridDim.y) * kThreads) {
    const uint64_t j = k / row.words, w = k - j * row.words;
    const uint64_t from = static_cast<uint64_t>(source[row.at + j]) * row.words + w;
    row.x_cur_to[k] = row.x_cur[from];
    row.x_best_to[k] = row.x_best[from];
  }
}

__global__ __launch_bounds__(kThreads) void k_population_gather_integers(const GatherRow *table,
                                                                         const uint32_t *__restrict__ source) {
  const GatherRow row = table[blockIdx.x];
  for (uint32_t j = blockIdx.y * kThreads + threadIdx.x; j < row.chains; j += gridDim.y * kThreads) {
    const uint32_t from = source[row.at + j];
    row.e_cur_to[j] = row.e_cur[from];
    row.e_best_to[j] = row.e_best[from];
    row.accepted_to[j] = row.accepted[from];
  }
}

// Steps 2-5 of ASP-PT-1, a thread per pair: thread j owns the pair (k, k + 1),
// k = parity + 2 j, and — where that pair does not exist — the slot k alone (the last slot of an odd
// remainder); thread 0 also owns slot 0 when parity = 1.  Every slot of the handle is written by exactly
// one thread.  back: energy[R] (64-bit words, what the host reads back) | source u32[R] | accepted u32
// (zeroed before the launch).  Plain vector stores and one atomic add per accepted pair.
struct ExchangeArgs {
  const double *energy;  // [R] reported energies of the current configurations
  const double *beta;    // [R] the slots' inverse temperatures
  uint64_t seed;
  uint32_t chains, sweeps_done, parity, draw;
};
__global__ __launch_bounds__(kThreads) void k_exchange_select(ExchangeArgs a, uint64_t *__restrict__ energy_out,
                                                              uint32_t *__restrict__ source,
                                                              uint32_t *__restrict__ accepted) {
  const uint32_t R = a.chains;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t k64 = a.parity + 2ull * j;
  if (j == 0 && a.parity == 1u && R != 0u) {
    energy_out[0] = static_cast<uint64_t>(__double_as_longlong(a.energy[0]));
    source[0] = 0u;
  }
  if (k64 >= R) return;
  const uint32_t k = static_cast<uint32_t>(k64);
  const double e0 = a.energy[k];
  energy_out[k] = static_cast<uint64_t>(__double_as_longlong(e0));
  if (k + 1u >= R) {  // (no partner)
    source[k] = k;
    return;
  }
  const double e1 = a.energy[k + 1u];
  energy_out[k + 1u] = static_cast<uint64_t>(__double_as_longlong(e1));
  const double x = __dmul_rn(__dadd_rn(a.beta[k + 1u], -a.beta[k]), __dadd_rn(e0, -e1));
  bool swap = x <= 0.0;
  if (!swap) {
    const Philox4 rnd = philox4x32_10(k, a.sweeps_done, 0xFFFFFFFCu, a.draw, static_cast<uint32_t>(a.seed),
                                      static_cast<uint32_t>(a.seed >> 32));
    swap = metropolis_accept_word(rnd.w[0], x);
  }
  source[k] = swap ? k + 1u : k;
  source[k + 1u] = swap ? k : k + 1u;
  if (swap) atomicAdd(accepted, 1u);
}

// The same steps for MANY handles in one launch (asp_sa_chains_exchange_batch): row i of `table`
// describes live handle i, whose slots own entries [at, at + chains) of energy_out and of source and
// whose counter is accepted[i] (zeroed before the launch).  blockIdx.x: handle; blockIdx.y strides over
// the handle's pair threads j, each with exactly the ownership and the arithmetic of k_exchange_select.
struct ExchangeRow {
  const double *energy;  // [chains] reported energies of the current configurations
  const double *beta;    // [chains] the slots' inverse temperatures
  uint64_t seed;
  uint64_t at;
  uint32_t chains, sweeps_done, parity, draw;
};
__global__ __launch_bounds__(kThreads) void k_exchange_select_batch(const ExchangeRow *table,
                                                                    uint64_t *__restrict__ energy_out,
                                                                    uint32_t *__restrict__ source,
                                                                    uint32_t *__restrict__ accepted) {
  const ExchangeRow row = table[blockIdx.x];
  const uint32_t R = row.chains;
  uint64_t *row_energy = energy_out + row.at;
  uint32_t *row_source = source + row.at;
  const uint64_t pairs = R / 2u + 1ull;  // threads of the single launch: one more for a parity of 1
  for (uint64_t j = static_cast<uint64_t>(blockIdx.y) * kThreads + threadIdx.x; j < pairs;
       j += static_cast<uint64_t>(gridDim.y) * kThreads) {
    const uint64_t k64 = row.parity + 2ull * j;
    if (j == 0 && row.parity == 1u && R != 0u) {
      row_energy[0] = static_cast<uint64_t>(__double_as_longlong(row.energy[0]));
      row_source[0] = 0u;
    }
    if (k64 >= R) continue;
    const uint32_t k = static_cast<uint32_t>(k64);
    const double e0 = row.energy[k];
    row_energy[k] = static_cast<uint64_t>(__double_as_longlong(e0));
    if (k + 1u >= R) {  // (no partner)
      row_source[k] = k;
      continue;
    }
    const double e1 = row.energy[k + 1u];
    row_energy[k + 1u] = static_cast<uint64_t>(__double_as_longlong(e1));
    const double x = __dmul_rn(__dadd_rn(row.beta[k + 1u], -row.beta[k]), __dadd_rn(e0, -e1));
    bool swap = x <= 0.0;
    if (!swap) {
      const Philox4 rnd = philox4x32_10(k, row.sweeps_done, 0xFFFFFFFCu, row.draw, static_cast<uint32_t>(row.seed),
                                        static_cast<uint32_t>(row.seed >> 32));
      swap = metropolis_accept_word(rnd.w[0], x);
    }
    row_source[k] = swap ? k + 1u : k;
    row_source[k + 1u] = swap ? k : k + 1u;
    if (swap) atomicAdd(accepted + blockIdx.x, 1u);
  }
}

int ensure_second_set(asp_sa_chains *c) {
  const uint64_t state_words = static_cast<uint64_t>(c->repetitions) * c->words;
  ASP_TRY(c->x_cur_to.ensure(state_words));
  ASP_TRY(c->x_best_to.ensure(state_words));
  ASP_TRY(c->e_cur_to.ensure(c->repetitions));
  ASP_TRY(c->e_best_to.ensure(c->repetitions));
  ASP_TRY(c->accepted_to.ensure(c->repetitions));
  return ASP_OK;
}

GatherRow gather_row(const asp_sa_chains *c, uint64_t at) {
  return GatherRow{c->x_cur.ptr, c->x_best.ptr, c->x_cur_to.ptr, c->x_best_to.ptr, c->e_cur.ptr, c->e_best.ptr,
                   c->e_cur_to.ptr, c->e_best_to.ptr, c->accepted.ptr, c->accepted_to.ptr, at, c->repetitions,
                   c->words};
}

// The two gather launches for the handles of `rows` (all with chains), on stream s.
int launch_gather(const std::vector<GatherRow> &rows, const GatherRow *d_rows, const uint32_t *d_source,
                  hipStream_t s) {
  uint64_t most_words = 0;
  uint32_t most_chains = 0;
  for (const GatherRow &row : rows) {
    most_words = std::max(most_words, static_cast<uint64_t>(row.chains) * row.words);
    most_chains = std::max(most_chains, row.chains);
  }
  const unsigned handles = static_cast<unsigned>(rows.size());
  if (most_words != 0) {
    const unsigned y = static_cast<unsigned>(std::min<uint64_t>((most_words + kThreads - 1) / kThreads, 1024));
    hipLaunchKernelGGL(k_population_gather_words, dim3(handles, y), dim3(kThreads), 0, s, d_rows, d_source);
    ASP_HIP_TRY(hipGetLastError());
  }
  const unsigned y = std::min((most_chains + kThreads - 1) / kThreads, 1024u);
  hipLaunchKernelGGL(k_population_gather_integers, dim3(handles, y), dim3(kThreads), 0, s, d_rows, d_source);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

// After the stream was waited for: the second set holds the new state.
void adopt(asp_sa_chains *c, const uint32_t *source) {
  std::swap(c->x_cur.ptr, c->x_cur_to.ptr);
  std::swap(c->x_cur.count, c->x_cur_to.count);
  std::swap(c->x_best.ptr, c->x_best_to.ptr);
  std::swap(c->x_best.count, c->x_best_to.count);
  std::swap(c->e_cur.ptr, c->e_cur_to.ptr);
  std::swap(c->e_cur.count, c->e_cur_to.count);
  std::swap(c->e_best.ptr, c->e_best_to.ptr);
  std::swap(c->e_best.count, c->e_best_to.count);
  std::swap(c->accepted.ptr, c->accepted_to.ptr);
  std::swap(c->accepted.count, c->accepted_to.count);
  const std::vector<int64_t> before = c->h_e_cur;
  for (uint32_t j = 0; j < c->repetitions; ++j) c->h_e_cur[j] = before[source[j]];
}

struct Events {
  hipEvent_t begin = nullptr, end = nullptr;
  ~Events() {
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
};

thread_local float g_resample_ms = 0.0f;
thread_local float g_exchange_ms = 0.0f;

}  // namespace

extern "C" {

int asp_sa_chains_gather(asp_sa_chains *c, uint32_t const *source) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  const uint32_t R = c->repetitions;
  if (R == 0) return ASP_OK;
  if (!source) return asp::set_error(ASP_ERR_INVALID, "null source");
  for (uint32_t j = 0; j < R; ++j) {
    if (source[j] >= R) {
      return asp::set_error(ASP_ERR_INVALID, "source[%u] = %u is not one of the %u chains", j, source[j], R);
    }
  }
  ASP_TRY(asp::bind_device());
  ASP_TRY(ensure_second_set(c));
  const std::vector<GatherRow> rows(1, gather_row(c, 0));
  asp::DeviceBuffer<GatherRow> d_rows;
  asp::DeviceBuffer<uint32_t> d_source;
  hipStream_t s = c->plan->stream;
  asp::StreamFence fence(s);
  ASP_TRY(d_rows.alloc(1));
  ASP_TRY(d_source.alloc(R));
  ASP_TRY(d_rows.upload(rows.data(), 1, s));
  ASP_TRY(d_source.upload(source, R, s));
  ASP_TRY(launch_gather(rows, d_rows.ptr, d_source.ptr, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  adopt(c, source);
  return ASP_OK;
}

float asp_sa_chains_resample_last_ms(void) { return g_resample_ms; }

int asp_sa_chains_exchange(asp_sa_chains *c, double const *chain_betas, uint32_t parity, uint32_t draw,
                           uint32_t *out_source, double *out_energy, uint32_t *out_accepted) {
  asp_clear_error();
  if (!c) return asp::set_error(ASP_ERR_INVALID, "null chains handle");
  const uint32_t R = c->repetitions;
  if (R && !chain_betas) return asp::set_error(ASP_ERR_INVALID, "null chain_betas");
  if (parity > 1u) return asp::set_error(ASP_ERR_INVALID, "parity must be 0 or 1");
  for (uint32_t r = 0; r < R; ++r) {
    if (!(chain_betas[r] >= 0.0) || std::isinf(chain_betas[r])) {
      return asp::set_error(ASP_ERR_INVALID, "chain_betas[%u] is not a finite number >= 0", r);
    }
  }
  asp_sa_plan *p = c->plan;
  if (R == 0 || p->host.num_spins == 0) {
    // no chains or no spins: nothing runs; every energy is 0 and the map the identity
    for (uint32_t r = 0; r < R; ++r) {
      if (out_source) out_source[r] = r;
      if (out_energy) out_energy[r] = 0.0;
    }
    if (out_accepted) *out_accepted = 0u;
    return ASP_OK;
  }
  ASP_TRY(asp::bind_device());
  // what comes back in one copy: energy[R] | source u32[R] | accepted u32
  const uint64_t source_at = R, accepted_at = source_at + (R + 1ull) / 2, back_words = accepted_at + 1;
  std::vector<uint64_t> h_back(back_words, 0);
  asp::DeviceBuffer<uint64_t> d_back;
  asp::DeviceBuffer<double> d_beta;
  asp::DeviceBuffer<GatherRow> d_rows;
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);
  ASP_TRY(ensure_second_set(c));
  ASP_TRY(d_back.alloc(back_words));
  ASP_TRY(d_beta.alloc(R));
  ASP_TRY(d_rows.alloc(1));
  ASP_TRY(p->w_x0_perm.ensure(static_cast<uint64_t>(R) * p->host.num_blocks));
  ASP_TRY(p->w_partial.ensure(static_cast<uint64_t>(R) * p->host.num_blocks));
  ASP_TRY(p->w_e.ensure(R));
  const std::vector<GatherRow> rows(1, gather_row(c, 0));
  ASP_TRY(d_beta.upload(chain_betas, R, s));
  ASP_TRY(d_rows.upload(rows.data(), 1, s));
  uint32_t *d_source = reinterpret_cast<uint32_t *>(d_back.ptr + source_at);
  uint32_t *d_accepted = reinterpret_cast<uint32_t *>(d_back.ptr + accepted_at);
  ASP_HIP_TRY(hipMemsetAsync(d_accepted, 0, sizeof(uint64_t), s));
  ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
  // step 1: the reported energies of the current configurations (step 1 of ASP-PA-1)
  ASP_TRY(asp::sa_permute_bits(p, c->x_cur.ptr, R, p->w_x0_perm.ptr));
  ASP_TRY(asp::sa_energies_of_perm(p, p->w_x0_perm.ptr, R, p->w_partial.ptr, p->w_e.ptr));
  // steps 2-5: a thread per pair (one more for the slot a parity of 1 leaves at the front)
  const ExchangeArgs args{p->w_e.ptr, d_beta.ptr, c->seed, R, c->sweeps_done, parity, draw};
  const uint32_t threads = R / 2u + 1u;
  hipLaunchKernelGGL(k_exchange_select, dim3((threads + kThreads - 1) / kThreads), dim3(kThreads), 0, s, args,
                     d_back.ptr, d_source, d_accepted);
  ASP_HIP_TRY(hipGetLastError());
  // step 6: the gather of asp_sa_chains_gather
  ASP_TRY(launch_gather(rows, d_rows.ptr, d_source, s));
  ASP_HIP_TRY(hipEventRecord(p->ev[3], s));
  ASP_TRY(d_back.download(h_back.data(), back_words, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  p->last_sweep_ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&p->last_total_ms, p->ev[0], p->ev[3]));
  const uint32_t *h_source = reinterpret_cast<const uint32_t *>(h_back.data() + source_at);
  adopt(c, h_source);
  if (out_source) std::memcpy(out_source, h_source, R * sizeof(uint32_t));
  if (out_energy) std::memcpy(out_energy, h_back.data(), R * sizeof(double));
  if (out_accepted) *out_accepted = *reinterpret_cast<const uint32_t *>(h_back.data() + accepted_at);
  return ASP_OK;
}

float asp_sa_chains_exchange_last_ms(void) { return g_exchange_ms; }

int asp_sa_chains_exchange_batch(asp_sa_chains_exchange_item const *items, uint32_t count) {
  asp_clear_error();
  g_exchange_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before any device work and before any output is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_exchange_item &it = items[i];
    if (it.flags != 0) return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    if (!it.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    const uint32_t R = it.chains->repetitions;
    if (R && !it.chain_betas) return asp::set_error(ASP_ERR_INVALID, "item %u: null chain_betas", i);
    if (it.parity > 1u) return asp::set_error(ASP_ERR_INVALID, "item %u: parity must be 0 or 1", i);
    for (uint32_t r = 0; r < R; ++r) {
      if (!(it.chain_betas[r] >= 0.0) || std::isinf(it.chain_betas[r])) {
        return asp::set_error(ASP_ERR_INVALID, "item %u: chain_betas[%u] is not a finite number >= 0", i, r);
      }
    }
  }
  {
    std::vector<asp_sa_chains *> handles(count);
    for (uint32_t i = 0; i < count; ++i) handles[i] = items[i].chains;
    ASP_TRY(asp::check_distinct_plans(handles));
  }
  // ---- the live handles (chains and spins) and their places in the batch's back buffer ----
  std::vector<uint32_t> live;
  std::vector<ExchangeRow> select;
  std::vector<double> h_beta;
  uint64_t total = 0;
  uint32_t most_pairs = 1;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains *c = items[i].chains;
    if (c->repetitions == 0 || c->plan->host.num_spins == 0) continue;
    live.push_back(i);
    select.push_back(ExchangeRow{nullptr, nullptr, c->seed, total, c->repetitions, c->sweeps_done, items[i].parity,
                                 items[i].draw});
    h_beta.insert(h_beta.end(), items[i].chain_betas, items[i].chain_betas + c->repetitions);
    total += c->repetitions;
    most_pairs = std::max(most_pairs, c->repetitions / 2u + 1u);
  }
  const uint32_t n = static_cast<uint32_t>(live.size());
  // what comes back in one copy: energy[total] | source u32[total] | accepted u32[n]
  const uint64_t source_at = total, accepted_at = source_at + (total + 1) / 2;
  const uint64_t back_words = accepted_at + (n + 1ull) / 2;
  std::vector<uint64_t> h_back(back_words, 0);
  if (n != 0) {
    ASP_TRY(asp::bind_device());
    asp::DeviceBuffer<ExchangeRow> d_select;
    asp::DeviceBuffer<GatherRow> d_gather;
    asp::DeviceBuffer<uint64_t> d_back;
    asp::DeviceBuffer<double> d_beta;
    Events ev;
    asp::ScopedStream batch;
    ASP_TRY(batch.acquire());
    hipStream_t s = batch.stream;
    ASP_HIP_TRY(hipEventCreate(&ev.begin));
    ASP_HIP_TRY(hipEventCreate(&ev.end));
    ASP_TRY(d_select.alloc(n));
    ASP_TRY(d_gather.alloc(n));
    ASP_TRY(d_back.alloc(back_words));
    ASP_TRY(d_beta.alloc(total));
    std::vector<GatherRow> gather(n);
    for (uint32_t k = 0; k < n; ++k) {
      asp_sa_chains *c = items[live[k]].chains;
      asp_sa_plan *p = c->plan;
      ASP_TRY(ensure_second_set(c));
      ASP_TRY(p->w_x0_perm.ensure(static_cast<uint64_t>(c->repetitions) * p->host.num_blocks));
      ASP_TRY(p->w_partial.ensure(static_cast<uint64_t>(c->repetitions) * p->host.num_blocks));
      ASP_TRY(p->w_e.ensure(c->repetitions));
      select[k].energy = p->w_e.ptr;
      select[k].beta = d_beta.ptr + select[k].at;
      gather[k] = gather_row(c, select[k].at);
    }
    // (declared after the buffers: on an early return every stream is waited for before they go)
    struct PlanFences {
      std::vector<hipStream_t> streams;
      ~PlanFences() {
        for (hipStream_t stream : streams) (void)hipStreamSynchronize(stream);
      }
    } fences;
    fences.streams.push_back(s);
    ASP_HIP_TRY(hipEventRecord(ev.begin, s));
    // step 1: the reported energies of the current configurations, on every plan's own stream
    for (uint32_t k = 0; k < n; ++k) {
      asp_sa_chains *c = items[live[k]].chains;
      asp_sa_plan *p = c->plan;
      fences.streams.push_back(p->stream);
      ASP_TRY(asp::sa_permute_bits(p, c->x_cur.ptr, c->repetitions, p->w_x0_perm.ptr));
      ASP_TRY(asp::sa_energies_of_perm(p, p->w_x0_perm.ptr, c->repetitions, p->w_partial.ptr, p->w_e.ptr));
      ASP_HIP_TRY(hipEventRecord(p->ev[0], p->stream));
      ASP_HIP_TRY(hipStreamWaitEvent(s, p->ev[0], 0));
    }
    // steps 2-5 and 6: one launch each for the whole batch, then one copy back
    ASP_TRY(d_select.upload(select.data(), n, s));
    ASP_TRY(d_gather.upload(gather.data(), n, s));
    ASP_TRY(d_beta.upload(h_beta.data(), total, s));
    uint32_t *d_source = reinterpret_cast<uint32_t *>(d_back.ptr + source_at);
    uint32_t *d_accepted = reinterpret_cast<uint32_t *>(d_back.ptr + accepted_at);
    ASP_HIP_TRY(hipMemsetAsync(d_accepted, 0, (back_words - accepted_at) * sizeof(uint64_t), s));
    const unsigned y = std::min((most_pairs + kThreads - 1) / kThreads, 1024u);
    hipLaunchKernelGGL(k_exchange_select_batch, dim3(n, y), dim3(kThreads), 0, s, d_select.ptr, d_back.ptr, d_source,
                       d_accepted);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(launch_gather(gather, d_gather.ptr, d_source, s));
    ASP_HIP_TRY(hipEventRecord(ev.end, s));
    ASP_TRY(d_back.download(h_back.data(), back_words, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
    ASP_HIP_TRY(hipEventElapsedTime(&g_exchange_ms, ev.begin, ev.end));
  }
  // ---- the handles' new state and the outputs ----
  const uint32_t *h_source = reinterpret_cast<const uint32_t *>(h_back.data() + source_at);
  const uint32_t *h_accepted = reinterpret_cast<const uint32_t *>(h_back.data() + accepted_at);
  for (uint32_t k = 0; k < n; ++k) {
    const asp_sa_chains_exchange_item &it = items[live[k]];
    const uint64_t at = select[k].at;
    const uint32_t R = it.chains->repetitions;
    adopt(it.chains, h_source + at);
    if (it.out_source) std::memcpy(it.out_source, h_source + at, R * sizeof(uint32_t));
    if (it.out_energy) std::memcpy(it.out_energy, h_back.data() + at, R * sizeof(double));
    if (it.out_accepted) *it.out_accepted = h_accepted[k];
  }
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_exchange_item &it = items[i];
    const uint32_t R = it.chains->repetitions;
    if (R != 0 && it.chains->plan->host.num_spins != 0) continue;
    // no chains or no spins: nothing runs; every energy is 0 and the map the identity
    for (uint32_t r = 0; r < R; ++r) {
      if (it.out_source) it.out_source[r] = r;
      if (it.out_energy) it.out_energy[r] = 0.0;
    }
    if (it.out_accepted) *it.out_accepted = 0u;
  }
  return ASP_OK;
}

int asp_sa_chains_resample_batch(asp_sa_chains_resample_item const *items, uint32_t count) {
  asp_clear_error();
  g_resample_ms = 0.0f;
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  // ---- validation: every item before any device work and before any output is written ----
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_resample_item &it = items[i];
    if (it.flags != 0) return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    if (!it.chains) return asp::set_error(ASP_ERR_INVALID, "item %u: null chains handle", i);
    // (an infinite step times the best chain's gap of 0 is not a number: the law needs a finite one)
    if (!(it.dbeta >= 0.0) || std::isinf(it.dbeta)) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: dbeta is not a finite number >= 0", i);
    }
    if (it.chains->repetitions > kMaxChains) {
      return asp::set_error(ASP_ERR_TOO_LARGE, "item %u: %u chains exceed the %u of a population (64-bit products)",
                            i, it.chains->repetitions, kMaxChains);
    }
  }
  {
    std::vector<asp_sa_chains *> handles(count);
    for (uint32_t i = 0; i < count; ++i) handles[i] = items[i].chains;
    ASP_TRY(asp::check_distinct_plans(handles));
  }
  // ---- the live handles (chains and spins) and their places in the batch's planes ----
  std::vector<uint32_t> live;
  std::vector<SelectRow> select;
  uint64_t total = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains *c = items[i].chains;
    if (c->repetitions == 0 || c->plan->host.num_spins == 0) continue;
    live.push_back(i);
    select.push_back(SelectRow{nullptr, c->seed, items[i].dbeta, total, c->repetitions, c->sweeps_done, items[i].draw});
    total += c->repetitions;
  }
  const uint32_t n = static_cast<uint32_t>(live.size());
  // what comes back in one copy: energy[total] | q[total] | source u32[total] | survivors u32[n]
  const uint64_t source_at = 2 * total, survivors_at = source_at + (total + 1) / 2;
  const uint64_t back_words = survivors_at + (n + 1ull) / 2;
  std::vector<uint64_t> h_back(back_words, 0);
  if (n != 0) {
    ASP_TRY(asp::bind_device());
    asp::DeviceBuffer<SelectRow> d_select;
    asp::DeviceBuffer<GatherRow> d_gather;
    asp::DeviceBuffer<uint64_t> d_back;  // the words above | prefix[total]
    Events ev;
    asp::ScopedStream batch;
    ASP_TRY(batch.acquire());
    hipStream_t s = batch.stream;
    ASP_HIP_TRY(hipEventCreate(&ev.begin));
    ASP_HIP_TRY(hipEventCreate(&ev.end));
    ASP_TRY(d_select.alloc(n));
    ASP_TRY(d_gather.alloc(n));
    ASP_TRY(d_back.alloc(back_words + total));
    std::vector<GatherRow> gather(n);
    for (uint32_t k = 0; k < n; ++k) {
      asp_sa_chains *c = items[live[k]].chains;
      asp_sa_plan *p = c->plan;
      ASP_TRY(ensure_second_set(c));
      ASP_TRY(p->w_x0_perm.ensure(static_cast<uint64_t>(c->repetitions) * p->host.num_blocks));
      ASP_TRY(p->w_partial.ensure(static_cast<uint64_t>(c->repetitions) * p->host.num_blocks));
      ASP_TRY(p->w_e.ensure(c->repetitions));
      select[k].energy = p->w_e.ptr;
      gather[k] = gather_row(c, select[k].at);
    }
    // (declared after the buffers: on an early return every stream is waited for before they go)
    struct PlanFences {
      std::vector<hipStream_t> streams;
      ~PlanFences() {
        for (hipStream_t stream : streams) (void)hipStreamSynchronize(stream);
      }
    } fences;
    ASP_HIP_TRY(hipEventRecord(ev.begin, s));
    // step 1: the reported energies of the current configurations, on every plan's own stream
    for (uint32_t k = 0; k < n; ++k) {
      asp_sa_chains *c = items[live[k]].chains;
      asp_sa_plan *p = c->plan;
      fences.streams.push_back(p->stream);
      ASP_TRY(asp::sa_permute_bits(p, c->x_cur.ptr, c->repetitions, p->w_x0_perm.ptr));
      ASP_TRY(asp::sa_energies_of_perm(p, p->w_x0_perm.ptr, c->repetitions, p->w_partial.ptr, p->w_e.ptr));
      ASP_HIP_TRY(hipEventRecord(p->ev[0], p->stream));
      ASP_HIP_TRY(hipStreamWaitEvent(s, p->ev[0], 0));
    }
    // steps 2-5 and 6: one launch each for the whole batch, then one copy back
    ASP_TRY(d_select.upload(select.data(), n, s));
    ASP_TRY(d_gather.upload(gather.data(), n, s));
    uint32_t *d_source = reinterpret_cast<uint32_t *>(d_back.ptr + source_at);
    uint32_t *d_survivors = reinterpret_cast<uint32_t *>(d_back.ptr + survivors_at);
    hipLaunchKernelGGL(k_population_select, dim3(n), dim3(kThreads), 0, s, d_select.ptr, total, d_back.ptr,
                       d_back.ptr + back_words, d_source, d_survivors);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(launch_gather(gather, d_gather.ptr, d_source, s));
    ASP_HIP_TRY(hipEventRecord(ev.end, s));
    ASP_TRY(d_back.download(h_back.data(), back_words, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
    ASP_HIP_TRY(hipEventElapsedTime(&g_resample_ms, ev.begin, ev.end));
  }
  // ---- the handles' new state and the outputs ----
  const uint32_t *h_source = reinterpret_cast<const uint32_t *>(h_back.data() + source_at);
  const uint32_t *h_survivors = reinterpret_cast<const uint32_t *>(h_back.data() + survivors_at);
  for (uint32_t k = 0; k < n; ++k) {
    const asp_sa_chains_resample_item &it = items[live[k]];
    const uint64_t at = select[k].at;
    const uint32_t R = it.chains->repetitions;
    adopt(it.chains, h_source + at);
    if (it.out_source) std::memcpy(it.out_source, h_source + at, R * sizeof(uint32_t));
    if (it.out_energy) std::memcpy(it.out_energy, h_back.data() + at, R * sizeof(double));
    if (it.out_q) std::memcpy(it.out_q, h_back.data() + total + at, R * sizeof(uint64_t));
    if (it.out_survivors) *it.out_survivors = h_survivors[k];
  }
  for (uint32_t i = 0; i < count; ++i) {
    const asp_sa_chains_resample_item &it = items[i];
    const uint32_t R = it.chains->repetitions;
    if (R != 0 && it.chains->plan->host.num_spins != 0) continue;
    // no chains or no spins: nothing runs; every energy is 0, every weight 1 and the map the identity
    for (uint32_t r = 0; r < R; ++r) {
      if (it.out_source) it.out_source[r] = r;
      if (it.out_energy) it.out_energy[r] = 0.0;
      if (it.out_q) it.out_q[r] = 1ull << 31;
    }
    if (it.out_survivors) *it.out_survivors = R;
  }
  return ASP_OK;
}

int asp_sa_chains_resample(asp_sa_chains *c, double dbeta, uint32_t draw, uint32_t *out_source, double *out_energy,
                           uint64_t *out_q, uint32_t *out_survivors) {
  const asp_sa_chains_resample_item item{c, dbeta, draw, 0u, out_source, out_energy, out_q, out_survivors};
  return asp_sa_chains_resample_batch(&item, 1);
}

}  // extern "C"
