// The pass after the sweeps of the colour-order annealer: the reported energies of
// block-order sign words — k_sa_energy_blocks*, k_sa_energy_fold*, or k_sa_post, which writes the
// configurations in original order in the same pass — and the kernels that permute packed configurations
// into the plan's block order and back, for one plan, for the problems of a batch and for the handles of
// a batched segment.  Every kernel here is launched here: the other units call the wrappers declared in
// sa_colour.hpp.  A change to this file leaves the sweep kernels' source-set fingerprint alone.
#include <algorithm>

#include "asp_common.hpp"
#include "sa_colour.hpp"
#include "sa_colour_kloop.hpp"
#include "sa_device.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

namespace {

using asp::DeviceBuffer;
using asp::kDummySpin;
using namespace asp::dev;
using namespace asp::colour;

constexpr int kMaxThreads = 1024;  // launch bound of k_sa_post, the sweep kernels'

// v with its sign flipped when bit 0 of `neg` is set (energy kernel, not hot).
__device__ __forceinline__ double signed_coupling(double v, uint32_t neg, int m) {
  const unsigned long long flip = static_cast<unsigned long long>((neg >> m) & 1u) << 63;
  return __longlong_as_double(__double_as_longlong(v) ^ static_cast<long long>(flip));
}

// Butterfly sum over the 64 lanes; every lane ends with the balanced-tree total
// ((v0+v1)+(v2+v3))+... (f64 addition commutes, so all lanes agree bitwise).
__device__ __forceinline__ double wave_tree_sum_f64(double v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v = __dadd_rn(v, __shfl_xor(v, step, 64));
  return v;
}

// ---------------------------------------------------------------------------
// Energy of packed configurations: E = D + T, T = radix-64
// pairwise tree over the blocks of t_p = s_p (A_p . s / 2 + h_p).
// ---------------------------------------------------------------------------

// STAGED: the configuration's sign words are copied to LDS first; otherwise (more blocks than the
// LDS holds) they are gathered from HBM/L2 directly.
template <bool STAGED>
__device__ __forceinline__ void energy_blocks_body(const EnergyArgs &a, const uint32_t r) {
  extern __shared__ __align__(16) uint8_t lds[];
  const uint64_t *mine = a.perm_words + static_cast<uint64_t>(r) * a.num_blocks;
  const uint64_t *bits = mine;
  if constexpr (STAGED) {
    uint64_t *staged = reinterpret_cast<uint64_t *>(lds);
    for (uint32_t w = threadIdx.x; w < a.num_blocks; w += blockDim.x) staged[w] = mine[w];
    __syncthreads();
    bits = staged;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = blockDim.x >> 6;
  for (uint32_t b = threadIdx.x >> 6; b < a.num_blocks; b += waves) {
    const uint32_t quads = a.block_width[b] >> 2;
    const uint64_t first_quad = a.ell_off[b] >> 2;
    const uint4 *cptr = reinterpret_cast<const uint4 *>(a.ell_col) + first_quad * 64u + lane;
    const double2 *vptr = reinterpret_cast<const double2 *>(a.ell_val) + first_quad * 128u + lane;
    double acc = 0.0;
    for (uint32_t q = 0; q < quads; ++q) {
      const uint4 c = cptr[q * 64u];
      const double2 v01 = vptr[q * 128u];
      const double2 v23 = vptr[q * 128u + 64u];
      const uint32_t cs[4] = {c.x, c.y, c.z, c.w};
      const double vs[4] = {v01.x, v01.y, v23.x, v23.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t neg = static_cast<uint32_t>((bits[cs[j] >> 6] >> (cs[j] & 63u)) & 1ull);
        acc = __dadd_rn(acc, signed_coupling(vs[j], neg, 0));
      }
    }
    const double g = __dadd_rn(__dmul_rn(0.5, acc), a.field_pos[b * 64u + lane]);
    const bool negative = (bits[b] >> lane) & 1ull;
    const double total = wave_tree_sum_f64(negative ? -g : g);
    if (lane == 0) a.partial[static_cast<uint64_t>(r) * a.num_blocks + b] = total;
  }
}

template <bool STAGED>
__global__ __launch_bounds__(512) void k_sa_energy_blocks(EnergyArgs a) {
  energy_blocks_body<STAGED>(a, blockIdx.x);
}

// R configurations per workgroup: every coupling quad is loaded once and applied to the R staged
// configurations (the chains of one call share the ELL: R times less load traffic than one
// configuration per workgroup).  Per configuration the arithmetic — and so the bits — are those
// of energy_blocks_body.
template <int R>
__global__ __launch_bounds__(512) void k_sa_energy_blocks_multi(EnergyArgs a, uint32_t count) {
  extern __shared__ __align__(16) uint8_t lds[];
  uint64_t *staged = reinterpret_cast<uint64_t *>(lds);  // [R][num_blocks]
  const uint32_t r0 = blockIdx.x * R;
  const uint32_t live = count - r0 < static_cast<uint32_t>(R) ? count - r0 : R;
  const uint64_t *rows = a.perm_words + static_cast<uint64_t>(r0) * a.num_blocks;
  for (uint32_t w = threadIdx.x; w < live * a.num_blocks; w += blockDim.x) staged[w] = rows[w];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = blockDim.x >> 6;
  for (uint32_t b = threadIdx.x >> 6; b < a.num_blocks; b += waves) {
    const uint32_t quads = a.block_width[b] >> 2;
    const uint64_t first_quad = a.ell_off[b] >> 2;
    const uint4 *cptr = reinterpret_cast<const uint4 *>(a.ell_col) + first_quad * 64u + lane;
    const double2 *vptr = reinterpret_cast<const double2 *>(a.ell_val) + first_quad * 128u + lane;
    double acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0;
    for (uint32_t q = 0; q < quads; ++q) {
      const uint4 c = cptr[q * 64u];
      const double2 v01 = vptr[q * 128u];
      const double2 v23 = vptr[q * 128u + 64u];
      const uint32_t cs[4] = {c.x, c.y, c.z, c.w};
      const double vs[4] = {v01.x, v01.y, v23.x, v23.y};
      const uint32_t *halves = reinterpret_cast<const uint32_t *>(staged);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t word = cs[j] >> 5, bit = cs[j] & 31u;  // 32-bit halves: ds_read_b32
#pragma unroll
        for (int k = 0; k < R; ++k) {
          // (rows beyond `live` hold stale LDS: their sums are computed and never stored)
          const uint32_t neg = (halves[k * 2u * a.num_blocks + word] >> bit) & 1u;
          acc[k] = __dadd_rn(acc[k], signed_coupling(vs[j], neg, 0));
        }
      }
    }
    const double field = a.field_pos[b * 64u + lane];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (static_cast<uint32_t>(k) >= live) break;  // workgroup-uniform
      const double g = __dadd_rn(__dmul_rn(0.5, acc[k]), field);
      const bool negative = (staged[k * a.num_blocks + b] >> lane) & 1ull;
      const double total = wave_tree_sum_f64(negative ? -g : g);
      if (lane == 0) a.partial[static_cast<uint64_t>(r0 + k) * a.num_blocks + b] = total;
    }
  }
}

// The pass after a sweep launch in one kernel: the block sums of k_sa_energy_blocks_multi<R> and, when
// `x` is given, the configurations in original order (k_unpermute_bits), from ONE staging of the
// R sign-word rows.  The rows are staged in the sweep's even-bit byte layout (a byte per position,
// configuration k at bit 2k), so the row sums run on the sweep's own k-loop: buffer loads with one
// quad in flight ahead, one ds_read_u8 per term for the R configurations, one v_lshl_or_b32 and one
// f64 FMA per term and configuration.  fma(J, +-1.0, acc) is acc + (+-J) bit for bit (the product
// is exact), the terms arrive in ascending k, and everything after the row sum is
// energy_blocks_body's: the partial sums are the bits of the kernels above.  No quad past the
// block is loaded.  Block metadata comes from scalar loads (the block index is wave-uniform).
template <int R>
__global__ __launch_bounds__(kMaxThreads) void k_sa_post(PostArgs pa, uint32_t count) {
  static_assert(R <= 4, "the even-bit byte holds four configurations");
  extern __shared__ __align__(16) uint8_t lds[];  // [num_blocks * 64] spin bytes
  const EnergyArgs &a = pa.e;
  // accumulate addresses the spin bytes absolutely: the dynamic LDS block must be the first
  // (this kernel declares no static LDS)
  if (reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t *)lds) != 0) {
    __builtin_trap();
  }
  const uint32_t r0 = blockIdx.x * R;
  const uint32_t live = count - r0 < static_cast<uint32_t>(R) ? count - r0 : R;
  const uint64_t *rows = a.perm_words + static_cast<uint64_t>(r0) * a.num_blocks;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  // a wavefront per block: the R words of the block are scalar loads, the lane's bits one byte
  // (rows beyond `live` stay 0: their sums are computed and never stored)
  for (uint32_t b = wave; b < a.num_blocks; b += waves) {
    uint32_t byte = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (static_cast<uint32_t>(k) >= live) break;  // workgroup-uniform
      const uint64_t word = rows[static_cast<uint64_t>(k) * a.num_blocks + b];
      byte |= static_cast<uint32_t>((word >> lane) & 1ull) << (2 * k);
    }
    lds[b * 64u + lane] = static_cast<uint8_t>(byte);
  }
  __syncthreads();  // the bytes are read-only from here on
  double mult[4] = {1.0, 1.0, 1.0, 1.0};  // (kWide's, unused by bytes)
  for (uint32_t b = wave; b < a.num_blocks; b += waves) {
    const uint32_t quads = a.block_width[b] >> 2;
    const uint64_t first_quad = a.ell_off[b] >> 2;
    const uint4 *col = reinterpret_cast<const uint4 *>(a.ell_col) + first_quad * 64u;
    const double2 *val = reinterpret_cast<const double2 *>(a.ell_val) + first_quad * 128u;
    const BlockStream stream{col + lane, block_rsrc(col), block_rsrc(val), lane * 16u};
    const uint32_t p = b * 64u + lane;
    const double field = a.field_pos[p];  // consumed after the row sum
    double acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0;
    // prefetch distance one, scalar loop control, no conditional load inside the loop body; the
    // last one or two quads are an epilogue, so nothing past the block is loaded (an empty
    // block's first load reads the next block's first quad or the plan's tail slabs, unused)
    Quad qa, qb;
    load_quad(qa, stream, 0);
    uint32_t i = 0;
    for (; i + 2 < quads; i += 2) {
      load_quad(qb, stream, i + 1);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<R, kBytes>(qa, lds, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
      load_quad(qa, stream, i + 2);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<R, kBytes>(qb, lds, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (i + 2 == quads) {
      load_quad(qb, stream, i + 1);
      accumulate<R, kBytes>(qa, lds, acc, mult);
      accumulate<R, kBytes>(qb, lds, acc, mult);
    } else if (i < quads) {
      accumulate<R, kBytes>(qa, lds, acc, mult);
    }
    const uint32_t own = lds[p];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (static_cast<uint32_t>(k) >= live) break;  // workgroup-uniform
      const double g = __dadd_rn(__dmul_rn(0.5, acc[k]), field);
      const bool negative = (own >> (2 * k)) & 1u;
      const double total = wave_tree_sum_f64(negative ? -g : g);
      if (lane == 0) a.partial[static_cast<uint64_t>(r0 + k) * a.num_blocks + b] = total;
    }
  }
  if (pa.x == nullptr) return;
  // a wavefront per output word: lane j owns spin 64 w + j, its position is read coalesced, its
  // byte once, and the word of each live configuration is one ballot
  for (uint32_t w = wave; w < pa.words; w += waves) {
    const uint64_t spin = static_cast<uint64_t>(w) * 64u + lane;
    const bool real = spin < pa.num_spins;
    const uint32_t byte = real ? static_cast<uint32_t>(lds[pa.pos_of_spin[spin]]) : 0u;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (static_cast<uint32_t>(k) >= live) break;  // workgroup-uniform
      const uint64_t word = __ballot(real && ((byte >> (2 * k)) & 1u) == 0u);
      if (lane == 0) pa.x[static_cast<uint64_t>(r0 + k) * pa.words + w] = word;
    }
  }
}

// One wavefront per configuration folds its block sums 64 at a time, in place.
__device__ __forceinline__ void energy_fold_body(double *partial, uint32_t num_blocks,
                                                 double diag_sum, double *out_e, const uint32_t r) {
  const uint32_t lane = threadIdx.x;
  double *level = partial + static_cast<uint64_t>(r) * num_blocks;
  uint32_t n = num_blocks;
  while (n > 1) {
    const uint32_t groups = (n + 63u) / 64u;
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t i = g * 64u + lane;
      const double v = i < n ? level[i] : 0.0;
      const double s = wave_tree_sum_f64(v);
      if (lane == 0) level[g] = s;
    }
    n = groups;
  }
  if (lane == 0) out_e[r] = __dadd_rn(diag_sum, num_blocks ? level[0] : 0.0);
}

__global__ __launch_bounds__(64) void k_sa_energy_fold(double *partial, uint32_t num_blocks,
                                                      double diag_sum, double *out_e) {
  energy_fold_body(partial, num_blocks, diag_sum, out_e, blockIdx.x);
}

// The same three steps for the chains of MANY problems in one launch each (asp_sa_anneal_batch):
// workgroup -> (problem, chain) through a table, the problem's pointers through a descriptor.
template <bool STAGED>
__global__ __launch_bounds__(512) void k_sa_energy_blocks_batch(const PostProblem *problems,
                                                               const BatchSlot *chains) {
  const BatchSlot c = chains[blockIdx.x];
  const EnergyArgs a = problems[__builtin_amdgcn_readfirstlane(c.problem)].e;
  energy_blocks_body<STAGED>(a, __builtin_amdgcn_readfirstlane(c.group));
}

__global__ __launch_bounds__(64) void k_sa_energy_fold_batch(const PostProblem *problems,
                                                            const BatchSlot *chains) {
  const BatchSlot c = chains[blockIdx.x];
  const PostProblem &pp = problems[c.problem];
  energy_fold_body(pp.e.partial, pp.e.num_blocks, pp.diag_sum, pp.out_e, c.group);
}

// Packed original-order configurations (bit = +1) -> permuted sign-bit words.
__global__ __launch_bounds__(256) void k_permute_bits(const uint64_t *__restrict__ x,
                                                     uint32_t words,
                                                     const uint32_t *__restrict__ spin_of_pos,
                                                     uint32_t num_blocks, uint32_t count,
                                                     uint64_t *__restrict__ perm_words) {
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<uint64_t>(count) * num_blocks) return;
  const uint32_t r = static_cast<uint32_t>(idx / num_blocks);
  const uint32_t b = static_cast<uint32_t>(idx % num_blocks);
  uint64_t word = 0;
  for (uint32_t l = 0; l < 64; ++l) {
    const uint32_t spin = spin_of_pos[b * 64u + l];
    if (spin == kDummySpin) continue;
    const uint64_t up = (x[static_cast<uint64_t>(r) * words + (spin >> 6)] >> (spin & 63u)) & 1ull;
    word |= (up ^ 1ull) << l;
  }
  perm_words[idx] = word;
}

// Permuted sign-bit words -> packed original-order configurations (bit = +1).  A wavefront per
// output word: lane j owns spin 64 w + j, its position is read once (coalesced) and used for
// kUnpermuteChains configurations; the word of each is one ballot.
constexpr uint32_t kUnpermuteChains = 32;
__global__ __launch_bounds__(256) void k_unpermute_bits(const uint64_t *__restrict__ perm_words,
                                                       uint32_t num_blocks,
                                                       const uint32_t *__restrict__ pos_of_spin,
                                                       uint64_t num_spins, uint32_t words,
                                                       uint32_t count, uint64_t *__restrict__ x) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (w >= words) return;  // whole wavefront
  const uint64_t spin = static_cast<uint64_t>(w) * 64u + lane;
  const bool live = spin < num_spins;
  const uint32_t pos = live ? pos_of_spin[spin] : 0u;
  const uint32_t first = blockIdx.y * kUnpermuteChains;
  const uint32_t last = first + kUnpermuteChains < count ? first + kUnpermuteChains : count;
  for (uint32_t r = first; r < last; ++r) {
    const uint64_t neg =
        (perm_words[static_cast<uint64_t>(r) * num_blocks + (pos >> 6)] >> (pos & 63u)) & 1ull;
    const uint64_t word = __ballot(live && neg == 0ull);
    if (lane == 0) x[static_cast<uint64_t>(r) * words + w] = word;
  }
}

// k_permute_bits for the initial configurations of a batch of descents: a workgroup per problem.
__global__ __launch_bounds__(256) void k_permute_bits_problems(const DescentProblem *problems) {
  const DescentProblem &d = problems[blockIdx.x];
  for (uint32_t b = threadIdx.x; b < d.s.num_blocks; b += blockDim.x) {
    uint64_t word = 0;
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t spin = d.s.spin_of_pos[b * 64u + l];
      if (spin == kDummySpin) continue;
      const uint64_t up = (d.x0[spin >> 6] >> (spin & 63u)) & 1ull;
      word |= (up ^ 1ull) << l;
    }
    d.x0_perm[b] = word;
  }
}

// The handles of a batched segment (asp_sa_chains_advance_batch, order 0) into and out of the form
// k_sa_sweep_batch runs their segments in: what sa_chains_advance_colour does with two permute launches,
// two unpermute launches and six copies PER HANDLE, for all handles in one launch each way.
// in: a workgroup per (handle, chain of the padded groups); the chains padding the last group start
// with every spin up and integers 0, as in the single segment.
__global__ __launch_bounds__(256) void k_chains_permute_problems(const ChainsIo *problems,
                                                                const BatchSlot *chains) {
  const BatchSlot c = chains[blockIdx.x];
  const ChainsIo &io = problems[c.problem];
  const uint64_t r = c.group;
  const bool live = r < io.chains;
  for (uint32_t b = threadIdx.x; b < io.num_blocks; b += blockDim.x) {
    uint64_t cur = 0, best = 0;
    if (live) {
      for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t spin = io.spin_of_pos[b * 64u + l];
        if (spin == kDummySpin) continue;
        const uint64_t at = r * io.words + (spin >> 6);
        cur |= (((io.x_cur[at] >> (spin & 63u)) & 1ull) ^ 1ull) << l;
        best |= (((io.x_best[at] >> (spin & 63u)) & 1ull) ^ 1ull) << l;
      }
    }
    io.cur_perm[r * io.num_blocks + b] = cur;
    io.best_perm[r * io.num_blocks + b] = best;
  }
  if (threadIdx.x == 0) {
    io.w_e_cur[r] = live ? io.e_cur[r] : 0ll;
    io.w_tracked[r] = live ? io.e_best[r] : 0ll;
    io.w_accepted[r] = live ? io.accepted[r] : 0ull;
  }
}
// out: a workgroup per (handle, chain)
__global__ __launch_bounds__(256) void k_chains_unpermute_problems(const ChainsIo *problems,
                                                                  const BatchSlot *chains) {
  const BatchSlot c = chains[blockIdx.x];
  const ChainsIo &io = problems[c.problem];
  const uint64_t r = c.group;
  const uint64_t *cur = io.cur_perm + r * io.num_blocks, *best = io.best_perm + r * io.num_blocks;
  for (uint32_t w = threadIdx.x; w < io.words; w += blockDim.x) {
    uint64_t cur_word = 0, best_word = 0;
    for (uint32_t j = 0; j < 64; ++j) {
      const uint64_t spin = static_cast<uint64_t>(w) * 64u + j;
      if (spin >= io.num_spins) break;
      const uint32_t pos = io.pos_of_spin[spin];
      cur_word |= (((cur[pos >> 6] >> (pos & 63u)) & 1ull) ^ 1ull) << j;
      best_word |= (((best[pos >> 6] >> (pos & 63u)) & 1ull) ^ 1ull) << j;
    }
    io.x_cur[r * io.words + w] = cur_word;
    io.x_best[r * io.words + w] = best_word;
  }
  if (threadIdx.x == 0) {
    io.e_cur[r] = io.w_e_cur[r];
    io.e_best[r] = io.w_tracked[r];
    io.accepted[r] = io.w_accepted[r];
  }
}

__global__ __launch_bounds__(256) void k_unpermute_bits_batch(const PostProblem *problems,
                                                             const BatchSlot *chains) {
  const BatchSlot c = chains[blockIdx.x];
  const PostProblem &pp = problems[c.problem];
  const uint64_t *perm = pp.e.perm_words + static_cast<uint64_t>(c.group) * pp.e.num_blocks;
  for (uint32_t w = threadIdx.x; w < pp.words; w += blockDim.x) {
    uint64_t word = 0;
    for (uint32_t j = 0; j < 64; ++j) {
      const uint64_t spin = static_cast<uint64_t>(w) * 64u + j;
      if (spin >= pp.num_spins) break;
      const uint32_t pos = pp.pos_of_spin[spin];
      const uint64_t neg = (perm[pos >> 6] >> (pos & 63u)) & 1ull;
      word |= (neg ^ 1ull) << j;
    }
    pp.out_x[static_cast<uint64_t>(c.group) * pp.words + w] = word;
  }
}

}  // namespace

namespace asp {
namespace colour {

int unpermute_bits(asp_sa_plan *p, const uint64_t *perm_words, uint32_t count, uint64_t *x) {
  const SaHostLayout &L = p->host;
  const uint32_t words = static_cast<uint32_t>((L.num_spins + 63) / 64);
  hipLaunchKernelGGL(k_unpermute_bits, dim3((words + 3) / 4, (count + kUnpermuteChains - 1) / kUnpermuteChains),
                     dim3(256), 0, p->stream, perm_words, L.num_blocks, p->pos_of_spin.ptr, L.num_spins, words,
                     count, x);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

int energies_of_perm(asp_sa_plan *p, const uint64_t *perm_words, uint32_t count, double *partial,
                     double *out_e, uint64_t *out_x) {
  const asp::SaHostLayout &L = p->host;
  if (count == 0) return ASP_OK;
  EnergyArgs ea{p->block_width.ptr, p->ell_off.ptr, p->ell_col.ptr, p->ell_val.ptr,
                p->field_pos.ptr,   perm_words,     partial,        L.num_blocks};
  const size_t lds = static_cast<size_t>(L.num_blocks) * sizeof(uint64_t);
  const uint32_t words = static_cast<uint32_t>((L.num_spins + 63) / 64);
  constexpr int kShare = 4;  // configurations per workgroup sharing the coupling loads
  const size_t post_lds = static_cast<size_t>(L.num_blocks) * 64;  // a byte per position
  if (count >= 2 * kShare && p->use_post && post_lds <= p->max_lds) {
    // (asp_sa_set_post; plans whose bytes do not fit the LDS keep the kernels below)
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_sa_post<kShare>), post_lds));
    const PostArgs pa{ea, p->pos_of_spin.ptr, out_x, L.num_spins, words};
    const uint32_t waves = std::min<uint32_t>(16u, L.num_blocks);
    hipLaunchKernelGGL(k_sa_post<kShare>, dim3((count + kShare - 1) / kShare), dim3(64 * waves),
                       post_lds, p->stream, pa, count);
    out_x = nullptr;  // done
  } else if (count >= 2 * kShare && lds * kShare <= p->max_lds) {
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_sa_energy_blocks_multi<kShare>), lds * kShare));
    hipLaunchKernelGGL(k_sa_energy_blocks_multi<kShare>, dim3((count + kShare - 1) / kShare),
                       dim3(512), lds * kShare, p->stream, ea, count);
  } else if (lds > p->max_lds) {
    hipLaunchKernelGGL(k_sa_energy_blocks<false>, dim3(count), dim3(512), 0, p->stream, ea);
  } else {
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_sa_energy_blocks<true>), lds));
    hipLaunchKernelGGL(k_sa_energy_blocks<true>, dim3(count), dim3(512), lds, p->stream, ea);
  }
  hipLaunchKernelGGL(k_sa_energy_fold, dim3(count), dim3(64), 0, p->stream, partial, L.num_blocks,
                     L.diag_sum, out_e);
  ASP_HIP_TRY(hipGetLastError());
  return out_x != nullptr ? unpermute_bits(p, perm_words, count, out_x) : ASP_OK;
}

// The pass after the sweeps of a batch — reported energies (the kernels and so the reduction order of
// energies_of_perm) and original-order bits of every chain's best configuration: a problem's descriptor,
// and the three launches over (problem, chain) slots.
PostProblem post_problem_of(const asp_sa_plan *p, const uint64_t *best, double *partial, double *out_e,
                            uint64_t *out_x) {
  const asp::SaHostLayout &L = p->host;
  PostProblem pp{};
  pp.e = EnergyArgs{p->block_width.ptr, p->ell_off.ptr, p->ell_col.ptr, p->ell_val.ptr,
                    p->field_pos.ptr,   best,           partial,        L.num_blocks};
  pp.pos_of_spin = p->pos_of_spin.ptr;
  pp.num_spins = L.num_spins;
  pp.words = static_cast<uint32_t>((L.num_spins + 63) / 64);
  pp.diag_sum = L.diag_sum;
  pp.out_e = out_e;
  pp.out_x = out_x;
  return pp;
}
// energy_lds: the sign words of the largest problem (num_blocks * 8 bytes), staged in LDS when they fit
int launch_post_batch(const PostProblem *d_post, const BatchSlot *d_chains, unsigned chains, size_t energy_lds,
                      size_t max_lds, hipStream_t s) {
  if (energy_lds > max_lds) {
    hipLaunchKernelGGL(k_sa_energy_blocks_batch<false>, dim3(chains), dim3(512), 0, s, d_post, d_chains);
  } else {
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_sa_energy_blocks_batch<true>), energy_lds));
    hipLaunchKernelGGL(k_sa_energy_blocks_batch<true>, dim3(chains), dim3(512), energy_lds, s, d_post, d_chains);
  }
  hipLaunchKernelGGL(k_sa_energy_fold_batch, dim3(chains), dim3(64), 0, s, d_post, d_chains);
  hipLaunchKernelGGL(k_unpermute_bits_batch, dim3(chains), dim3(256), 0, s, d_post, d_chains);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

// The state permutes of the shared launches: a workgroup per problem (the descents' start configurations),
// per (handle, chain of the padded groups) in, per (handle, chain) out.
int launch_permute_problems(const DescentProblem *d_problems, unsigned problems, hipStream_t s) {
  hipLaunchKernelGGL(k_permute_bits_problems, dim3(problems), dim3(256), 0, s, d_problems);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}
int launch_chains_permute(const ChainsIo *d_io, const BatchSlot *d_chains, unsigned chains, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_permute_problems, dim3(chains), dim3(256), 0, s, d_io, d_chains);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}
int launch_chains_unpermute(const ChainsIo *d_io, const BatchSlot *d_chains, unsigned chains, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_unpermute_problems, dim3(chains), dim3(256), 0, s, d_io, d_chains);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}
}  // namespace colour

int sa_permute_bits(asp_sa_plan *p, const uint64_t *x, uint32_t count, uint64_t *perm) {
  const SaHostLayout &L = p->host;
  const uint64_t total = static_cast<uint64_t>(count) * L.num_blocks;
  if (total == 0) return ASP_OK;
  const uint32_t words = static_cast<uint32_t>((L.num_spins + 63) / 64);
  hipLaunchKernelGGL(k_permute_bits, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                     p->stream, x, words, p->spin_of_pos.ptr, L.num_blocks, count, perm);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

int sa_energies_of_perm(asp_sa_plan *p, const uint64_t *perm, uint32_t count, double *partial,
                        double *out_e) {
  return colour::energies_of_perm(p, perm, count, partial, out_e);
}

}  // namespace asp

extern "C" {

int asp_sa_energy(asp_sa_plan *p, uint32_t count, uint64_t const *x, double *out_e) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  ASP_TRY(asp::bind_device());
  if (count == 0) return ASP_OK;
  if (!x || !out_e) return asp::set_error(ASP_ERR_INVALID, "null argument");
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  if (K == 0) {
    for (uint32_t r = 0; r < count; ++r) out_e[r] = 0.0;
    return ASP_OK;
  }
  const uint32_t words = static_cast<uint32_t>((K + 63) / 64);
  hipStream_t s = p->stream;
  DeviceBuffer<uint64_t> d_x, d_perm;
  DeviceBuffer<double> d_partial, d_e;
  ASP_TRY(d_x.alloc(static_cast<uint64_t>(count) * words));
  ASP_TRY(d_perm.alloc(static_cast<uint64_t>(count) * L.num_blocks));
  ASP_TRY(d_partial.alloc(static_cast<uint64_t>(count) * L.num_blocks));
  ASP_TRY(d_e.alloc(count));
  ASP_TRY(d_x.upload(x, static_cast<uint64_t>(count) * words, s));
  ASP_TRY(asp::sa_permute_bits(p, d_x.ptr, count, d_perm.ptr));
  ASP_TRY(asp::colour::energies_of_perm(p, d_perm.ptr, count, d_partial.ptr, d_e.ptr));
  ASP_TRY(d_e.download(out_e, count, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  return ASP_OK;
}

}  // extern "C"
