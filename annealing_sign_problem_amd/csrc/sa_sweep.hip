// Metropolis single-spin-flip annealing sweep on gfx950 (specification ASP-SA-1,
// DESIGN.md §4): replaces ising_glass_annealer.anneal at the reference's call
// sites annealing_sign_problem/common.py:242-248 and
// experiments/full_hilbert_space.py:212-218.
//
// Mapping to the machine
//   * one workgroup = one GROUP of M replicas (M in {1,2,4,8}); the whole anneal (all sweeps) is ONE
//     launch, the spins never leave LDS;
//   * LDS: one byte per (padded) spin position, bit 2m (M <= 4) or bit m (M = 8) = sign bit of replica m
//     (1 means s = -1), so one ds_read_u8 serves all M replicas of a neighbour (kBytes); a 32-bit word per
//     position for M = 4 on small clusters, where the sign of a term is one SDWA instruction (kWide);
//     beyond the capacity of bytes a nibble (kNibbles) or one BIT per position and one replica per
//     workgroup, flips applied by a wavefront ballot (kBits), and beyond 1.3e6 spins the same bit words in
//     HBM (kGlobal);
//   * a wavefront owns a 64-row block of one colour class: lane = spin.  Same colour means no couplings
//     inside the block, so the 64 x M proposals of a block are independent and are decided at once;
//   * couplings stream from the quad-interleaved sliced ELL: per four terms a lane issues three 16-byte
//     buffer loads (every wavefront instruction covers 1 KiB of contiguous memory; the quad is a scalar
//     offset), shared by M replicas, one quad prefetched ahead;
//   * dE is an f64 sum in fixed row order (bit-exact against the oracle), the acceptance uses a
//     counter-based Philox4x32-10 word per (spin, sweep, replica) and a fixed-sequence exp reached through
//     a hardware-exp filter, accepted flips are XOR-ed into LDS;
//   * the running energy of each replica is tracked exactly in 2^-S fixed point (integer adds commute, so
//     the parallel reduction is deterministic); the best configuration is snapshotted to HBM per sweep
//     (kWide: kept as a difference from the current one in a spare bit of the word, written once);
//   * frozen sweeps: row sums cached in HBM and re-used while no neighbour of a block flipped (dirty
//     bytes), blocks whose proposals are all certain rejections skipped outright (inert bytes); or (TAIL)
//     only the rows listed in a bitmap evaluated, compacted into visits of 64;
//   * DESCENT: strict-descent sweeps without random numbers (the greedy solver's relaxation);
//   * few chains on a large cluster: k_sa_sweep_team spreads ONE chain over 2-8 workgroups.
// Every one-workgroup kernel is sa_sweep_body: ColourSweep::start, then per sweep tail_sweep (visit_rows
// over listed_row_sums) or colour_sweep (visit_block over block_row_sums), reduce and end_of_sweep, then
// epilogue.  Said once each: where the LDS regions start (SweepLds, CtlSlot), which Philox word replica m
// gets (for_replica_words), when a proposal needs a draw (ColourSweep::accept, both visits'), when the
// field cache or tail mode is entered and left (end_of_sweep_mode).
// f64-VALU- and vector-memory-bound integer+f64 work: no MFMA.
//
// This file holds the sweep kernels and, behind them, every decision about which kernel runs in which
// shape: the form table and the kernel families, the LDS sizes, choose_colour_launch, the team size, the
// cache and tail thresholds, the class rule of the shared launches and sweep_args — what a profiler
// counter of k_sa_sweep* can depend on (build.KERNEL_SOURCE_SETS["colour"]).  What only allocates,
// copies, validates or records is host code elsewhere: csrc/sa_anneal.hip (plan, closed calls, segments),
// csrc/sa_batch.hip (shared launches); the pass after the sweeps is csrc/sa_energy.hip.  The argument
// types and the prototypes: sa_colour.hpp.
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "asp_common.hpp"
#include "sa_colour.hpp"
#include "sa_colour_kloop.hpp"
#include "sa_device.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

namespace {

using asp::kDummySpin;
using namespace asp::dev;  // Philox, the accept filter, the spin layouts (sa_device.hpp)
using namespace asp::colour;  // the kernels' argument types, SweepLds (sa_colour.hpp); the k-loop (sa_colour_kloop.hpp)

constexpr int kMaxThreads = 1024;  // launch bound of the sweep kernel (VGPR budget = 512 / waves per SIMD)
constexpr int kTeamSleep = 4;  // s_sleep argument between two polls of the team barrier (0/1/4/16/64 scanned)

// One 64-spin word of the bit-packed layouts; device-scope accesses when it lives in HBM and
// other wavefronts of the workgroup read it after the colour barrier.
template <bool GLOBAL>
__device__ __forceinline__ uint64_t load_word(const uint64_t *p) {
  if constexpr (GLOBAL) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    return *p;
  }
}
template <bool GLOBAL>
__device__ __forceinline__ void store_word(uint64_t *p, uint64_t v) {
  if constexpr (GLOBAL) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    *p = v;
  }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
  return v;
}

// The same sum modulo 2^64 with the total in lane 63 ONLY (the other lanes end with partial sums),
// by data-parallel-primitive moves between registers: no LDS round trip.  Shifts by 1, 2, 4 and 8
// inside every row of 16 lanes leave the row's sum in its last lane (a lane the shift has no source
// for adds the `old` operand, 0); row_bcast 15 adds that lane to rows 1 and 3, row_bcast 31 adds lane
// 31 to rows 2 and 3.  Every lane of the wavefront must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_add_u64(unsigned long long v) {
  const uint32_t lo = static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v)), CTRL, ROW_MASK, 0xF, false));
  const uint32_t hi = static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v >> 32)), CTRL, ROW_MASK, 0xF, false));
  return v + ((static_cast<unsigned long long>(hi) << 32) | lo);
}
__device__ __forceinline__ unsigned long long wave_sum_lane63_u64(unsigned long long v) {
  v = dpp_add_u64<0x111, 0xF>(v);  // row_shr:1
  v = dpp_add_u64<0x112, 0xF>(v);  // row_shr:2
  v = dpp_add_u64<0x114, 0xF>(v);  // row_shr:4
  v = dpp_add_u64<0x118, 0xF>(v);  // row_shr:8
  v = dpp_add_u64<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add_u64<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return v;
}

// Collect bit m of each of the four bytes of d into a nibble (byte 0 -> bit 0).
__device__ __forceinline__ uint32_t gather_bit4(uint32_t d, int m) {
  const uint32_t t = (d >> m) & 0x01010101u;
  return ((t * 0x00204081u) >> 21) & 0xFu;
}

// What snapshot() reads of its arguments, for another target than the best words: the final words of a
// segment (the resume epilogue).
struct FinalWords {
  uint64_t *best_perm;
  uint32_t num_blocks;
};
// (`Args` is SweepArgs, SweepArgs in the constant address space — see k_sa_sweep_batch — or FinalWords)
template <int M, int LAYOUT, typename Args>
__device__ __forceinline__ void snapshot(const uint8_t *spins, const Args &a, uint32_t group,
                                         uint32_t mask) {
  if constexpr (LAYOUT == kWide || LAYOUT == kNibbles) {  // a wavefront per block: one ballot per replica
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t b = threadIdx.x >> 6; b < a.num_blocks; b += blockDim.x >> 6) {
      // the position's word (replica m's sign at bit 8m + 7) or nibble (at bit m)
      const uint32_t own = LAYOUT == kWide
                               ? reinterpret_cast<const uint32_t *>(spins)[b * 64u + lane]
                               : static_cast<uint32_t>(spins[b * 32u + (lane >> 1)]) >> ((lane & 1u) << 2);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if (!((mask >> m) & 1u)) continue;  // workgroup-uniform
        const uint64_t word = __ballot((own >> (LAYOUT == kWide ? 8 * m + 7 : m)) & 1u);
        if (lane == 0) {
          a.best_perm[(static_cast<uint64_t>(group) * M + m) * a.num_blocks + b] = word;
        }
      }
    }
    return;
  }
  if constexpr (LAYOUT == kBits || LAYOUT == kGlobal) {  // the words already are the sign bits
    const uint64_t *words = reinterpret_cast<const uint64_t *>(spins);
    for (uint32_t w = threadIdx.x; w < a.num_blocks; w += blockDim.x) {
      uint64_t word;
      if constexpr (LAYOUT == kGlobal) {
        word = __hip_atomic_load(words + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        word = words[w];
      }
      a.best_perm[static_cast<uint64_t>(group) * a.num_blocks + w] = word;
    }
    return;
  }
  for (uint32_t w = threadIdx.x; w < a.num_blocks; w += blockDim.x) {
    const uint4 *src = reinterpret_cast<const uint4 *>(spins + 64u * w);
    uint4 q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = src[j];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (!((mask >> m) & 1u)) continue;
      const int bit = replica_bit<M, LAYOUT>(m);
      uint64_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t nib = gather_bit4(q[j].x, bit) | (gather_bit4(q[j].y, bit) << 4) |
                             (gather_bit4(q[j].z, bit) << 8) | (gather_bit4(q[j].w, bit) << 12);
        word |= static_cast<uint64_t>(nib) << (16 * j);
      }
      a.best_perm[(static_cast<uint64_t>(group) * M + m) * a.num_blocks + w] = word;
    }
  }
}

// ---- kWide keeps no copy of the best configuration during the launch: bit 8m of a position's word
// says whether replica m's spin there differs from its best one (sa_device.hpp).  An anneal that cools
// improves in nearly every sweep, so nearly every snapshot would be overwritten one sweep later. ----
// The replicas in `improved` (workgroup-uniform) are at their best: their d bits go, at every position.
// The whole workgroup, a uint4 per thread and iteration; between the barriers snapshot() runs between.
__device__ __forceinline__ void clear_differs(uint8_t *spins, uint32_t num_blocks, uint32_t improved) {
  const uint32_t keep = ~differs_mask(improved);
  uint4 *words = reinterpret_cast<uint4 *>(spins);
  for (uint32_t i = threadIdx.x; i < num_blocks * 16u; i += blockDim.x) {
    uint4 w = words[i];
    w.x &= keep;
    w.y &= keep;
    w.z &= keep;
    w.w &= keep;
    words[i] = w;
  }
}
// The best configurations of the replicas in `mask` (workgroup-uniform) from the words, once per launch:
// snapshot()'s wavefront per block and ballot per replica, over s ^ d.
template <int M, typename Args>
__device__ __forceinline__ void materialise_best(const uint8_t *spins, const Args &a, uint32_t group,
                                                 uint32_t mask) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t b = threadIdx.x >> 6; b < a.num_blocks; b += blockDim.x >> 6) {
    const uint32_t best = best_signs(reinterpret_cast<const uint32_t *>(spins)[b * 64u + lane]);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (!((mask >> m) & 1u)) continue;
      const uint64_t word = __ballot((best >> (8 * m + 7)) & 1u);
      if (lane == 0) {
        a.best_perm[(static_cast<uint64_t>(group) * M + m) * a.num_blocks + b] = word;
      }
    }
  }
}

// How a descent ends (DESCENT only).  NoEarlyStop: all num_sweeps sweeps run (the annealer; the
// chunks of asp_sa_greedy, whose host looks at the flip count between chunks).  StopWhenStill:
// the workgroup leaves after the first sweep that flipped nothing and reports the number of
// sweeps it performed (k_sa_sweep_batch over DescentProblem).
struct NoEarlyStop {
  static constexpr bool kEnabled = false;
};
struct StopWhenStill {
  static constexpr bool kEnabled = true;
  uint32_t *sweeps_done;  // this problem's word
};

// The inverse temperature of replica m: the sweep's shared one, or (ResumeLadder) the replica's own —
// workgroup-uniform, so scalar registers.  One or two replicas read theirs once before the sweep loop
// and hold them.  Four and eight read them where they are used, once per visit of a block (scalar loads
// of one cache line that stays in the scalar cache): those instantiations have no scalar register to
// spare, and 2 M more held for the whole launch went to scratch (M = 8 bytes: 160 B against the 32 B of
// k_sa_sweep_resume, M = 4 words: 36 B against none; read at the point of use: 84 B and 12 B, spilled
// around the accept phase of a visit, not in the k-loop).
template <int M, bool LADDER>
struct LadderBetas {
  template <typename Res>
  __device__ __forceinline__ LadderBetas(const Res &, uint32_t) {}
  __device__ __forceinline__ double of(int, double beta) const { return beta; }
};
template <int M>
struct LadderBetas<M, true> {
  static constexpr bool kHeld = M <= 2;
  double own[kHeld ? M : 1];
  const double *mine;  // the group's M values
  __device__ __forceinline__ LadderBetas(const ResumeLadder &res, uint32_t group)
      : mine(res.chain_betas + static_cast<uint64_t>(group) * M) {
    if constexpr (kHeld) {
#pragma unroll
      for (int m = 0; m < M; ++m) own[m] = mine[m];
    }
  }
  __device__ __forceinline__ double of(int m, double) const {
    if constexpr (kHeld) {
      return own[m];
    } else {
      return mine[m];
    }
  }
};

// The words of ctl.  One mode per kernel: the field cache, or (TAIL) tail sweeps.
enum CtlSlot : uint32_t {
  kCtlFlips = 0,        // flips of the workgroup in the running sweep
  kCtlModeOn = 1,       // 1 while the mode is on: cached fields are in use / sweeps run as tail sweeps
  kCtlModeEntered = 2,  // 1 when the mode was just entered: every dirty byte / todo bit must be set
  kCtlTicket = 3,       // the ticket counter that hands a colour's blocks to the wavefronts
  kCtlTailSweeps = 4,   // TAIL: sweeps run as tail sweeps
  kCtlTailEntries = 5,  // TAIL: entries into tail mode
};

// ---- Which Philox word replica m gets (RNG contract: DESIGN.md section 4.3) ----
struct ChainKey {
  uint32_t r0, key0, key1;  // the group's first replica, the seed's halves
};
// use(m, word) for m = 0 .. M - 1: replica r = r0 + m takes word r & 3 of the call with the counter
// (spin, sweep, r >> 2, 0); sweep = 0xFFFFFFFF is the start configuration.
// ALIGNED (M = 4 only): the host promises r0 % 4 == 0 (aligned_replicas()), so the group is one whole
// call and replica m takes word m of it, known at compile time.  Without the promise the first replica's
// place in its call is a run-time value: a group that straddles two calls makes the second when it
// reaches it, and every word is selected with pick_word (three v_cndmask_b32 on scalar masks per
// replica).  Same counters, same words.
template <int M, bool ALIGNED, typename Use>
__device__ __forceinline__ void for_replica_words(uint32_t spin, uint32_t sweep, const ChainKey &k, Use &&use) {
  Philox4 rnd{};
  if constexpr (ALIGNED) {
    rnd = philox4x32_10(spin, sweep, k.r0 >> 2, 0u, k.key0, k.key1);
#pragma unroll
    for (int m = 0; m < M; ++m) use(m, rnd.w[m]);
  } else {
    uint32_t have = 0xFFFFFFFFu;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const uint32_t r = k.r0 + m;
      if (m == 0 || (r >> 2) != have) {
        have = r >> 2;
        rnd = philox4x32_10(spin, sweep, have, 0u, k.key0, k.key1);
      }
      use(m, pick_word(rnd, r & 3u));
    }
  }
}

// ---- The row sums of a visit: two k-loops, side by side ----
// The block visit (lane = row of ONE block): prefetch distance one — the next quad's three 16-byte
// loads are in flight while the current quad is gathered from LDS and accumulated, in the oracle's
// order k = 0, 1, 2, ...  Loop control is scalar and the body has no conditional loads (hipcc would
// otherwise drain the queue with vmcnt(0) at the loop header); sched_barrier keeps each load group
// ahead of the accumulate it overlaps.  `width`: the block's EXACT width, its longest row (meta[b].y;
// the rounded width where a kernel has no meta): (width + 3) / 4 quads, the last of width & 3 real terms
// (0: of four).
//   EXACT (exact_kloop() below says which kernels): the loop runs only while both of its loads lie inside
//     the block, and the block's last quad goes through accumulate_last, which stops at the longest row's
//     last term.  No load is issued for a quad the block does not have, nothing for a block of width 0.
//     The parity of the quad count is settled in FRONT of the loop — an even count loads quads 0 and 1 and
//     accumulates quad 0 first —, so that the last quad is in qa whatever the count: with the last one or
//     two quads behind the loop hipcc merged the two accumulate_last and copied a quad (+10 VGPRs, scratch
//     in words).
//   otherwise the loop every kernel had: every quad in full, and for an even quad count (and for none)
//     a last load that reads one quad past the block — the next block's first slabs or the tail padding
//     the plan appends — and is never consumed.
// Either way acc[m] receives the row's real terms in ascending k, and the same bits (accumulate_last).
template <int M, int LAYOUT, bool EXACT>
__device__ __forceinline__ void block_row_sums(const BlockStream &stream, uint32_t width, const uint8_t *spins,
                                               double (&acc)[M], double (&mult)[4]) {
  const uint32_t quads = (width + 3u) >> 2;
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
  Quad qa, qb;
  if constexpr (EXACT) {
    if (quads == 0u) return;
    uint32_t i = 0;  // qa holds quad i, and quads - i is odd
    if (quads & 1u) {
      load_quad(qa, stream, 0);
    } else {
      // (the barrier in front keeps hipcc from merging this load of quad 0 with the other branch's: it
      // then copied quad 1 into qa behind a vmcnt(0))
      __builtin_amdgcn_sched_barrier(0);
      load_quad(qb, stream, 0);
      load_quad(qa, stream, 1);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<M, LAYOUT>(qb, spins, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
      i = 1;
    }
    for (; i + 2 < quads; i += 2) {
      load_quad(qb, stream, i + 1);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<M, LAYOUT>(qa, spins, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
      load_quad(qa, stream, i + 2);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<M, LAYOUT>(qb, spins, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
    }
    accumulate_last<M, LAYOUT>(qa, width & 3u, spins, acc, mult);
  } else {
    load_quad(qa, stream, 0);
    uint32_t i = 0;
    for (; i + 2 <= quads; i += 2) {
      load_quad(qb, stream, i + 1);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<M, LAYOUT>(qa, spins, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
      load_quad(qa, stream, i + 2);
      __builtin_amdgcn_sched_barrier(0);
      accumulate<M, LAYOUT>(qb, spins, acc, mult);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (i < quads) accumulate<M, LAYOUT>(qa, spins, acc, mult);
  }
}
// The tail visit (every lane its OWN row of `row_quads` quads, at col_at / val_at bytes from the start of
// the arrays): a lane streams the quads of its row and never the next block's — from its width on it
// reads the first 48 bytes of the arrays instead (one cache line for all such lanes) and accumulates
// nothing.  Every load is issued unconditionally — a load under a lane mask makes hipcc drain the queue
// in front of each accumulate —, so the quad is part of the lane's offset and the k-loop keeps the block
// visit's prefetch distance of one.  The sums are accumulate()'s in ascending k: the block visit's f64
// values bit for bit.
template <int M, int LAYOUT>
__device__ __forceinline__ void listed_row_sums(BufferRsrc col_rsrc, BufferRsrc val_rsrc, uint32_t row_quads,
                                                uint32_t col_at, uint32_t val_at, const uint8_t *spins,
                                                double (&acc)[M], double (&mult)[4]) {
  auto load_row_quad = [&](Quad &q, uint32_t quad) {
    const bool mine = quad < row_quads;
    const uint32_t c_at = mine ? col_at + quad * 1024u : 0u;
    const uint32_t v_at = mine ? val_at + quad * 2048u : 0u;
    q.c = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(col_rsrc, c_at, 0, 0));
    q.v01 = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(val_rsrc, v_at, 0, 0));
    q.v23 = __builtin_bit_cast(double2,
                               __builtin_amdgcn_raw_buffer_load_b128(val_rsrc, v_at + (mine ? 1024u : 16u), 0, 0));
  };
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
  Quad qa, qb;
  load_row_quad(qa, 0u);
  for (uint32_t q = 0; __ballot(q < row_quads) != 0ull; q += 2u) {
    load_row_quad(qb, q + 1u);
    __builtin_amdgcn_sched_barrier(0);
    if (q < row_quads) accumulate<M, LAYOUT>(qa, spins, acc, mult);
    __builtin_amdgcn_sched_barrier(0);
    load_row_quad(qa, q + 2u);
    __builtin_amdgcn_sched_barrier(0);
    if (q + 1u < row_quads) accumulate<M, LAYOUT>(qb, spins, acc, mult);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- The lane's own spin at position p of block b (block visit: b is wave-uniform), per layout: read in
// front of the accept phase (ColourSweep::accept), flipped behind it ----
template <int LAYOUT>
__device__ __forceinline__ uint32_t load_own(const uint8_t *spins, uint32_t p, uint32_t b) {
  if constexpr (LAYOUT == kBits || LAYOUT == kGlobal) {
    return static_cast<uint32_t>(
        (load_word<LAYOUT == kGlobal>(reinterpret_cast<const uint64_t *>(spins) + b) >> (p & 63u)) & 1ull);
  } else if constexpr (LAYOUT == kWide) {
    return reinterpret_cast<const uint32_t *>(spins)[p];
  } else if constexpr (LAYOUT == kNibbles) {
    return (static_cast<uint32_t>(spins[p >> 1]) >> ((p & 1u) << 2)) & 15u;
  } else {
    return spins[p];
  }
}

// What a lane gathers over a sweep.  q[m]: the fixed-point energy changes of its accepted flips, modulo
// 2^64 (lean bookkeeping: plus 0x4338000000000000 per visit); n[m]: its accepted flips (< 2^32 blocks per
// sweep); visits: the lean bookkeepings of this wavefront in this sweep (wave-uniform).
template <int M>
struct SweepSums {
  unsigned long long q[M];
  uint32_t n[M];
  uint32_t visits;
};

// The replicas in `flip` change sign.  Every lane of the wavefront calls it.
template <int M, int LAYOUT>
__device__ __forceinline__ void store_flip(uint8_t *spins, uint32_t p, uint32_t b, uint32_t own, uint32_t flip) {
  if constexpr (LAYOUT == kBits || LAYOUT == kGlobal) {
    // the block's 64 proposals decided: one XOR of the ballot into the block's word
    const uint64_t flips = __ballot(flip != 0);
    if ((p & 63u) == 0 && flips != 0) {
      uint64_t *word = reinterpret_cast<uint64_t *>(spins) + b;
      store_word<LAYOUT == kGlobal>(word, load_word<LAYOUT == kGlobal>(word) ^ flips);
    }
  } else if constexpr (LAYOUT == kWide) {
    // sign and "differs from the best" bit alike (sa_device.hpp)
    if (flip) reinterpret_cast<uint32_t *>(spins)[p] = own ^ flip_mask(flip);
  } else if constexpr (LAYOUT == kNibbles) {
    // the neighbouring lane owns the other nibble of the byte and may flip in the same
    // instruction: an LDS atomic on the word (eight positions) instead of a byte store
    if (flip) atomicXor(reinterpret_cast<uint32_t *>(spins) + (p >> 3), flip << ((p & 7u) << 2));
  } else {
    // positions of a visit are distinct: plain stores
    if (flip) spins[p] = static_cast<uint8_t>(own ^ encode_replicas<M, LAYOUT>(flip));
  }
}

// ---- When the field cache or tail mode is entered and left (thread 0, end of a sweep) ----
// Either mode pays while a sweep's flips touch a fraction of the rows only: enter after a sweep with
// fewer than `enter` flips of the workgroup, leave above twice that — the field cache at 2 * enter
// itself, tail mode not — or when the caller says so (leave_now: tail mode in front of a sweep at a
// lower beta).  Resets the flip count; TAIL counts the sweeps run in the mode and the entries.
template <bool TAIL>
__device__ __forceinline__ void end_of_sweep_mode(uint32_t *ctl, uint32_t enter, bool leave_now) {
  const uint32_t flips = ctl[kCtlFlips];
  ctl[kCtlFlips] = 0;
  const bool was = ctl[kCtlModeOn] != 0;
  bool now = was ? (TAIL ? flips <= 2ull * enter : flips < 2u * enter) : flips < enter;
  if (leave_now) now = false;
  ctl[kCtlModeOn] = now ? 1u : 0u;
  ctl[kCtlModeEntered] = (now && !was) ? 1u : 0u;
  if constexpr (TAIL) {
    if (was) ctl[kCtlTailSweeps] += 1u;
    if (now && !was) ctl[kCtlTailEntries] += 1u;
  }
}
// Every block's entry of a per-block LDS array (dirty, inert, todo), by the whole workgroup.
template <typename T>
__device__ __forceinline__ void fill_blocks(T *per_block, uint32_t num_blocks, T value) {
  for (uint32_t b = threadIdx.x; b < num_blocks; b += blockDim.x) per_block[b] = value;
}

// ---- Which kernels' block visit takes the k-loop that ends on the block's last real term (block_row_sums,
// EXACT) ----
// The forms of four chains per group in bytes, words and nibbles.  Every other kernel keeps the loop it had:
// the switch at the loop's end is code a visit has to hold registers across (DESIGN.md section 6 has the
// resource table of both loops).  Every kernel reads the exact width from meta[] all the same.
template <int M, bool DESCENT, int LAYOUT, typename Args, typename Res>
constexpr bool exact_kloop() {
  if (M != 4 || DESCENT) return false;
  return LAYOUT == kBytes || LAYOUT == kWide || LAYOUT == kNibbles;
}

// The whole anneal of one group of M replicas by one workgroup, in the phases sa_sweep_body() below runs in
// order; `group` = index of the group inside its problem (k_sa_sweep: the workgroup id; k_sa_sweep_batch:
// looked up in a table).
// DESCENT = true: strict-descent sweeps (accept iff dE < 0, no random numbers, no beta: a.betas is
// never read), used by the greedy solver's relaxation; the final configuration is snapshotted
// after every sweep.
// ALIGNED (M = 4 only): see for_replica_words.
// TAIL (the closed call's M = 4 kernels in bytes and words): once a sweep flips fewer spins than
// tail.enter_flips the workgroup keeps one `todo` bit per position in LDS and a sweep evaluates only the
// listed rows, compacted into visits of 64 rows with lane = row.  These
// instantiations have no field cache and no inert bytes.
// (`Args` is SweepArgs, or SweepArgs in the constant address space: see k_sa_sweep_batch)
template <int M, bool DESCENT, int LAYOUT, typename Args, typename Stop, typename Res, bool ALIGNED, bool TAIL>
struct ColourSweep {
  static_assert(!TAIL || (M == 4 && !DESCENT && !Res::kEnabled && (LAYOUT == kBytes || LAYOUT == kWide)),
                "tail sweeps: the closed call of four chains in bytes or words");
  static_assert(DESCENT || !Stop::kEnabled, "only a descent can stop early");
  static_assert(!ALIGNED || (!DESCENT && M == 4), "an aligned group is one whole Philox call");
  static_assert(!DESCENT || !Res::kEnabled, "a descent is never resumed");
  static constexpr bool GLOBAL = LAYOUT == kGlobal;
  static constexpr bool PACKED = LAYOUT == kBits || GLOBAL;  // one bit per position
  static constexpr bool WIDE = LAYOUT == kWide;
  static constexpr bool NIBBLES = LAYOUT == kNibbles;
  static constexpr bool kLeanBook = M <= 4 && !(Res::kLadder && WIDE);  // see accept()
  // the best configuration lives in the words' d bits until the epilogue (clear_differs, materialise_best)
  static constexpr bool kLazyBest = WIDE;
  // the block visit's k-loop ends on the block's last real term (block_row_sums)
  static constexpr bool kExactLoop = exact_kloop<M, DESCENT, LAYOUT, Args, Res>();
  static_assert(!PACKED || M == 1, "the bit-packed layouts hold one replica");
  static_assert(!NIBBLES || (M <= 4 && !DESCENT), "the nibble layout holds up to four replicas");
  static_assert(!WIDE || (M <= 4 && !DESCENT), "the wide layout holds up to four replicas");

  const Args &a;
  const uint32_t group;
  const Stop stop;  // (what the launch takes beside SweepArgs: see NoEarlyStop, NoResume, TailArgs)
  const Res res;
  const TailArgs tail;
  const uint32_t tid = threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const ChainKey key;
  // ResumeLadder: the replicas' own betas (workgroup-uniform: scalar registers)
  const LadderBetas<M, Res::kLadder> ladder;
  const bool cache_available;
  // the LDS regions (SweepLds); kGlobal: this workgroup's bit words live in HBM
  uint8_t *spins, *dirty, *inert;
  long long *delta, *book;
  uint32_t *improved_flag, *ctl, *rings;  // TAIL: wavefront w's ring at rings + w * kTailRing
  uint2 *meta;
  uint64_t *todo;
  double mult[4] = {1.0, 1.0, 1.0, 1.0};  // kWide's multipliers (low words stay 0)
  uint32_t ticket_base = 0;  // ctl[kCtlTicket] at the start of the running colour (workgroup-uniform)
  // StopWhenStill: sweeps performed, and the chain's accepted flips before the running sweep
  uint32_t sweeps_done;
  long long flips_before = 0;

  __device__ __forceinline__ ColourSweep(const Args &a_, uint32_t group_, const Stop &stop_, const Res &res_,
                                         const TailArgs &tail_)
      : a(a_), group(group_), stop(stop_), res(res_), tail(tail_),
        key{a_.replica_first + group_ * M, static_cast<uint32_t>(a_.seed), static_cast<uint32_t>(a_.seed >> 32)},
        ladder(res_, group_), cache_available(!TAIL && !PACKED && a_.field_cache != nullptr),
        sweeps_done(a_.num_sweeps) {
    extern __shared__ __align__(16) uint8_t lds[];
    // accumulate addresses the spin bytes absolutely: the dynamic LDS block must be the first
    // (this kernel declares no static LDS)
    if (reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t *)lds) != 0) __builtin_trap();
    const SweepLds at(a.num_blocks, LAYOUT, TAIL, waves);
    spins = GLOBAL ? reinterpret_cast<uint8_t *>(a.spin_words + static_cast<uint64_t>(group) * a.num_blocks) : lds;
    delta = reinterpret_cast<long long *>(lds + at.delta);
    book = reinterpret_cast<long long *>(lds + at.book);
    improved_flag = reinterpret_cast<uint32_t *>(lds + at.flag);
    meta = reinterpret_cast<uint2 *>(lds + at.meta);
    ctl = reinterpret_cast<uint32_t *>(lds + at.ctl);
    dirty = lds + at.dirty;
    inert = lds + at.inert;
    todo = reinterpret_cast<uint64_t *>(lds + at.todo);
    rings = reinterpret_cast<uint32_t *>(lds + at.ring);
  }

  // ---- Start: the configuration (a wavefront initialises whole 64-position blocks), the books, the
  // first snapshot ----
  __device__ __forceinline__ void start() {
    for (uint32_t b0 = wave; b0 < a.num_blocks; b0 += waves) {
      const uint32_t p = b0 * 64u + lane;
      const uint32_t spin = a.spin_of_pos[p];
      uint32_t byte = 0;  // replica m's sign bit at replica_bit(m)
      if constexpr (Res::kEnabled) {
        // every chain's own words (a padding lane's bit is whatever the words hold: never read back)
        if (spin != kDummySpin) {
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const uint64_t word = res.cur_perm[(static_cast<uint64_t>(group) * M + m) * a.num_blocks + b0];
            byte |= static_cast<uint32_t>((word >> lane) & 1ull) << replica_bit<M, LAYOUT>(m);
          }
        }
      } else if (spin != kDummySpin) {
        if (a.x0_perm != nullptr) {
          byte = ((a.x0_perm[p >> 6] >> (p & 63u)) & 1ull) ? encode_replicas<M, LAYOUT>((1u << M) - 1u)
                                                           : 0u;  // every replica
        } else {
          for_replica_words<M, ALIGNED>(spin, 0xFFFFFFFFu, key, [&](int m, uint32_t word) {
            const uint32_t up = word & 1u;  // 1 -> s = +1 -> sign bit 0
            byte |= (up ^ 1u) << replica_bit<M, LAYOUT>(m);
          });
        }
      }
      if constexpr (PACKED) {
        const uint64_t word = __ballot(byte & 1u);
        if (lane == 0) store_word<GLOBAL>(reinterpret_cast<uint64_t *>(spins) + b0, word);
      } else if constexpr (WIDE) {
        reinterpret_cast<uint32_t *>(spins)[p] = spread_mask(byte);
      } else if constexpr (NIBBLES) {
        const uint32_t upper = __shfl_xor(byte, 1);  // the odd lane's nibble, for the even lane
        if ((tid & 1u) == 0) spins[p >> 1] = static_cast<uint8_t>(byte | (upper << 4));
      } else {
        spins[p] = static_cast<uint8_t>(byte);
      }
      if constexpr (!PACKED) {
        // meta[b0] = {first slab, EXACT width}.  The plan rounds a block's width up to whole quads and
        // pads every row with entries that point at the row's own position (A has no diagonal: no real
        // entry does), so the padding the 64 rows share is, in the block's last quad, the smallest count
        // of trailing own-position columns over the lanes (a dummy lane is all padding: it never lowers
        // it).  Once per launch and block; the plan's arrays stay what they are.
        const uint32_t first_slab = static_cast<uint32_t>(a.ell_off[b0]);
        const uint32_t rounded = a.block_width[b0];  // wave-uniform
        uint32_t shared = 0;
        if (rounded != 0u) {
          const uint64_t last_quad = static_cast<uint64_t>((first_slab >> 2) + (rounded >> 2) - 1u);
          const uint4 c4 = reinterpret_cast<const uint4 *>(a.ell_col)[last_quad * 64u + lane];
          const uint32_t own = WIDE ? p * 4u : p;  // (wide columns are byte addresses)
          const bool pad3 = c4.w == own, pad2 = pad3 && c4.z == own, pad1 = pad2 && c4.y == own;
          shared = (__ballot(pad3) == ~0ull ? 1u : 0u) + (__ballot(pad2) == ~0ull ? 1u : 0u) +
                   (__ballot(pad1) == ~0ull ? 1u : 0u);
        }
        if (lane == 0) meta[b0] = make_uint2(first_slab, rounded - shared);
      }
    }
    // delta[8] | book[24]: every entry is written once, by one lane — 0, or (a segment) for book[] of a
    // live chain the carried value (current tracked energy, best, accepted flips)
    if (tid < 32) {
      long long v = 0;
      if constexpr (Res::kEnabled) {
        const uint32_t which = tid >> 3, m = tid & 7u;
        if (which >= 1u && m < static_cast<uint32_t>(M)) {
          const uint64_t chain = static_cast<uint64_t>(group) * M + m;
          v = which == 1u ? res.e_cur[chain]
                          : (which == 2u ? a.tracked[chain] : static_cast<long long>(a.accepted[chain]));
        }
      }
      delta[tid] = v;
    }
    if (tid == 0) {
      *improved_flag = 0;
      if constexpr (kLazyBest && Res::kEnabled) improved_flag[1] = 0;
      ctl[kCtlFlips] = ctl[kCtlModeOn] = ctl[kCtlModeEntered] = ctl[kCtlTicket] = 0;
      if constexpr (TAIL) ctl[kCtlTailSweeps] = ctl[kCtlTailEntries] = 0;
    }
    __syncthreads();
    if constexpr (!Res::kEnabled && !kLazyBest) {
      // (a segment's best configuration so far is in a.best_perm already and stays unless the segment
      // improves on it: no initial snapshot.  kLazyBest: the start has d = 0 for every replica, it IS
      // the best so far)
      snapshot<M, LAYOUT>(spins, a, group, (1u << M) - 1u);
      __syncthreads();
    }
    if (a.trace != nullptr && tid < M) {
      long long first = 0;
      if constexpr (Res::kEnabled) first = book[tid];  // (not reset: relative to the chain's very first state)
      a.trace[(static_cast<uint64_t>(group) * M + tid) * (a.num_sweeps + 1ull)] = first;
    }
  }

  // ---- The accept phase of a visit, for the lane's position: propose, decide, book.  Returns the
  // replicas that flip; open: some proposal of the lane was not a certain rejection.  The positions of a
  // visit are of one colour, so their proposals are independent and are decided at once. ----
  __device__ __forceinline__ uint32_t accept(const double (&acc)[M], double h, uint32_t own, uint32_t spin,
                                             uint32_t t_draw, double beta, SweepSums<M> &sums, bool &open) {
    const bool valid = spin != kDummySpin;
    // Propose: de[m] = replica m's energy change of flipping the lane's spin.
    open = false;
    bool need = false;  // some proposal of this lane needs a random number
    double de[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double g = __dadd_rn(acc[m], h);
      const bool negative = (own >> (WIDE ? 8 * m + 7 : replica_bit<M, LAYOUT>(m))) & 1u;  // s = -1
      de[m] = __dmul_rn(negative ? 2.0 : -2.0, g);
      if constexpr (DESCENT) {
        open = open || (valid && de[m] < 0.0);
      } else {
        const bool maybe = valid && !(__dmul_rn(ladder.of(m, beta), de[m]) >= 23.0);  // not a certain rejection
        open = open || maybe;
        need = need || (maybe && !(de[m] <= 0.0));
      }
    }
    // Decide.  Random numbers only when some proposal of the wavefront is undecided without one
    // (dE <= 0 is accepted, beta * dE >= 23 rejected, whatever the draw; a descent accepts dE < 0 and
    // nothing else): a wave-uniform branch around the 10 Philox rounds and the exp filter.
    // Counter-based RNG: skipping a draw changes nothing downstream.
    // The accepted proposals: bit m of accept_mask, or (kLeanBook) all ones in took[m].
    uint32_t accept_mask = 0;
    [[maybe_unused]] uint32_t took[M];
    auto decided = [&](int m, bool accepted) {
      if constexpr (kLeanBook) {
        took[m] = accepted ? 0xFFFFFFFFu : 0u;
      } else {
        accept_mask |= (accepted ? 1u : 0u) << m;
      }
    };
    if (!DESCENT && __ballot(need) != 0ull) {
      for_replica_words<M, ALIGNED>(spin, t_draw, key, [&](int m, uint32_t word) {
        decided(m, valid && (de[m] <= 0.0 || metropolis_accept_word(word, __dmul_rn(ladder.of(m, beta), de[m]))));
      });
    } else {
#pragma unroll
      for (int m = 0; m < M; ++m) decided(m, valid && (DESCENT ? de[m] < 0.0 : de[m] <= 0.0));
    }
    // Book.  rint(dE * 2^S) as int64: |dE * 2^S| < 2^51 by the plan's choice of S, so adding 1.5 * 2^52
    // leaves the rounded integer in the mantissa (ties to even, = rint): the sum's bit pattern is
    // 0x4338000000000000 + rint(dE * 2^S).
    uint32_t flip = 0;
    if constexpr (kLeanBook) {
      // Lean (up to four replicas): no branch and no selection.  EVERY replica adds the bit pattern of
      // dE * scale_m + 1.5 * 2^52, where scale_m is 2^S for an accepted proposal and 0 otherwise (2^S is a
      // power of two: its low word is 0 and the high word is masked) — dE is finite, so a proposal that
      // is not accepted adds the bare constant.  The `visits` constants come off once per sweep, in front
      // of the reduction, modulo 2^64.  One fma is the multiply followed by the add: dE * 2^S is exact —
      // the fma then rounds the very sum the add rounds — or it underflows, to something below 2^-1022
      // either way, and both sums round to 1.5 * 2^52.  v_fma_f64 reads one scalar operand, so the
      // constant is put in vector registers here, after the k-loop: held for the whole launch it costs
      // every instantiation two registers more.
      double round_bias = 0x1.8p52;
      asm volatile("" : "+v"(round_bias));
      const uint32_t scale_hi = static_cast<uint32_t>(__double2hiint(a.scale));
#pragma unroll
      for (int m = 0; m < M; ++m) {
        flip |= took[m] & (1u << m);
        const double scale_m = __hiloint2double(static_cast<int>(scale_hi & took[m]), 0);
        sums.q[m] += static_cast<unsigned long long>(__double_as_longlong(__builtin_fma(de[m], scale_m, round_bias)));
        sums.n[m] -= took[m];  // + 1 when accepted
      }
      sums.visits += 1;
    } else {
      // Per flip: eight replicas and the ladder segment of four in words have no vector register to
      // spare in the accept phase, and the lean form's two more sent them to scratch.
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if ((accept_mask >> m) & 1u) {
          flip |= 1u << m;
          sums.q[m] += static_cast<unsigned long long>(
              __double_as_longlong(__dadd_rn(__dmul_rn(de[m], a.scale), 0x1.8p52)) - 0x4338000000000000ll);
          sums.n[m] += 1;
        }
      }
    }
    return flip;
  }

  // ---- A tail sweep (workgroup-uniform: false when tail mode is off): only the rows listed in `todo` ----
  // Per colour a wavefront takes every waves-th block of the colour, 64 of them at a time (lane i
  // reads and clears the word of its i-th), and stages the listed rows of the non-empty ones,
  // block by block, in its ring at their mbcnt ranks.  As soon as 64 rows wait they are one visit
  // with lane = row (visit_rows).  Rows of a colour are independent, the random words are keyed by
  // (spin, sweep, replica) and the energy sums are integers: which rows share a visit changes no result.
  __device__ __forceinline__ bool tail_sweep(uint32_t t_draw, double beta, SweepSums<M> &sums) {
    if (__builtin_amdgcn_readfirstlane(ctl[kCtlModeOn]) == 0) return false;
    const uint32_t wave_u = __builtin_amdgcn_readfirstlane(wave);
    uint32_t *ring = rings + wave_u * kTailRing;
    const BufferRsrc col_rsrc = block_rsrc(a.ell_col), val_rsrc = block_rsrc(a.ell_val);
    for (uint32_t c = 0; c < a.num_colors; ++c) {
      const uint32_t b_begin = a.color_block_start[c];
      const uint32_t nb = a.color_block_start[c + 1] - b_begin;
      uint32_t fill = 0, drained = 0;  // rows staged and rows visited so far (wave-uniform)
      uint32_t base = 0, next_base = wave_u;
      uint64_t w = 0, nonempty = 0;  // the lane's word of the running 64 blocks, and which lanes' are left
      for (;;) {
        while (fill - drained < 64u) {
          if (nonempty == 0ull) {
            if (next_base >= nb) break;
            base = next_base;
            next_base += waves * 64u;
            const uint32_t i = base + lane * waves;
            w = 0;
            if (i < nb) {
              // nobody marks a block during its own colour step but the wavefront that took it
              w = todo[b_begin + i];
              if (w != 0ull) todo[b_begin + i] = 0ull;
            }
            nonempty = __ballot(w != 0ull);
            continue;
          }
          const uint32_t src = static_cast<uint32_t>(__builtin_ctzll(nonempty));
          nonempty &= nonempty - 1ull;
          const uint32_t w_lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(w), src);
          const uint32_t w_hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(w >> 32), src);
          const uint32_t rank = __builtin_amdgcn_mbcnt_hi(w_hi, __builtin_amdgcn_mbcnt_lo(w_lo, 0u));
          const uint32_t mine = lane < 32u ? w_lo >> lane : w_hi >> (lane - 32u);
          if (mine & 1u) ring[(fill + rank) & (kTailRing - 1u)] = (b_begin + base + src * waves) * 64u + lane;
          fill += static_cast<uint32_t>(__builtin_popcount(w_lo) + __builtin_popcount(w_hi));
        }
        const uint32_t count = min(64u, fill - drained);
        if (count == 0u) break;
        // (LDS operations of one wavefront complete in order; the fence keeps the compiler's order)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        visit_rows(ring, drained, count, col_rsrc, val_rsrc, t_draw, beta, sums);
        drained += count;
      }
      __syncthreads();
    }
    return true;
  }

  // One visit of the `count` rows staged in the ring from `drained` on; the other lanes behave like
  // dummy lanes.
  __device__ __forceinline__ void visit_rows(const uint32_t *ring, uint32_t drained, uint32_t count,
                                             BufferRsrc col_rsrc, BufferRsrc val_rsrc, uint32_t t_draw,
                                             double beta, SweepSums<M> &sums) {
    uint32_t *todo32 = reinterpret_cast<uint32_t *>(todo);
    const bool live = lane < count;
    uint32_t p = 0, row_quads = 0, col_at = 0, val_at = 0;
    if (live) {
      p = ring[(drained + lane) & (kTailRing - 1u)];
      const uint2 info = meta[p >> 6];
      row_quads = (info.y + 3u) >> 2;  // (info.y: the exact width)
      // the lane's row in the arrays, from their start (the host launches this form only while
      // both arrays stay below 4 GiB): columns 1024 B and values 2048 B per quad of a block
      col_at = (info.x >> 2) * 1024u + (p & 63u) * 16u;
      val_at = (info.x >> 2) * 2048u + (p & 63u) * 16u;
    }
    // The row's spin and field: in bytes issued now and consumed behind the row sum, like the
    // block visit's.  In words they are read behind the k-loop: a lane of this visit holds more
    // of its own (its position, width and offsets) than a lane of a block visit, and the word
    // layout has no register left for them (held across the loop they went to scratch).
    uint32_t spin = kDummySpin;
    double h = 0.0;
    if (!WIDE && live) {
      spin = a.spin_of_pos[p];
      h = a.field_pos[p];
    }
    double acc[M];
    listed_row_sums<M, LAYOUT>(col_rsrc, val_rsrc, row_quads, col_at, val_at, spins, acc, mult);
    uint32_t own = 0;
    if (WIDE && live) {
      spin = a.spin_of_pos[p];
      h = a.field_pos[p];
    }
    if (live) {
      own = load_own<LAYOUT>(spins, p, p >> 6);
    }
    bool open;
    const uint32_t flip = accept(acc, h, own, spin, t_draw, beta, sums, open);
    // the row comes back while a proposal of it is open (an accepted one was)
    if (open) atomicOr(&todo32[p >> 5], 1u << (p & 31u));
    if (flip) {
      store_flip<M, LAYOUT>(spins, p, p >> 6, own, flip);
      // every neighbour's field changed: list it (the neighbours are of other colours; the
      // row's columns only, its padding entries point at the row itself)
      const uint4 *cols4 =
          reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.ell_col) + col_at);
      for (uint32_t q = 0; q < row_quads; ++q) {
        const uint4 c4 = cols4[q * 64u];
        const uint32_t cols[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t at = WIDE ? cols[j] >> 2 : cols[j];
          if (at != p) atomicOr(&todo32[at >> 5], 1u << (at & 31u));
        }
      }
    }
  }

  // ---- A full sweep: every colour, every block (but those the field cache calls inert) ----
  __device__ __forceinline__ void colour_sweep(uint32_t t, uint32_t t_draw, double beta, SweepSums<M> &sums) {
    // wave-uniform: cached fields are in use during this sweep
    const bool cached = cache_available && __builtin_amdgcn_readfirstlane(ctl[kCtlModeOn]) != 0;
    if constexpr (!DESCENT && !Res::kLadder) {
      if (cached && t > 0 && beta < a.betas[t - 1]) {
        // certain rejections are only certain for non-decreasing beta (workgroup-uniform branch)
        fill_blocks(inert, a.num_blocks, uint8_t{0});
        __syncthreads();
      }
    }
    for (uint32_t c = 0; c < a.num_colors; ++c) {
      const uint32_t b_begin = a.color_block_start[c];
      const uint32_t b_end = a.color_block_start[c + 1];
      // The colour's blocks go to the wavefronts in ascending order (widest rows first, the plan
      // sorts a colour by descending degree), each to the first wavefront that is free: the first
      // `waves` blocks one per wavefront, every later one by a ticket drawn from ctl[kCtlTicket].  The
      // ticket of the NEXT block is drawn before the visit of this one and read after it, so no
      // visit ends on a wait for the atomic (the visit's first LDS read returns in order behind it
      // and does wait for it); every wavefront that visits a block therefore ends the
      // colour on one ticket past b_end, and the colour draws exactly b_end - b_begin tickets in
      // all.  The counter is never reset: when the colour barrier is passed it stands at
      // ticket_base + (b_end - b_begin) in every wavefront's books (mod 2^32).
      uint32_t ticket = 0;
      for (uint32_t b = b_begin + wave; b < b_end;
           b = b_begin + waves + (__builtin_amdgcn_readfirstlane(ticket) - ticket_base)) {
        // (atomicInc, not atomicAdd: hipcc rewrites an LDS atomicAdd into a wave reduction and one more
        // dependent wait in front of every visit; measured slower)
        if (lane == 0) ticket = atomicInc(&ctl[kCtlTicket], 0xFFFFFFFFu);
        visit_block(b, cached, t_draw, beta, sums);
      }
      ticket_base += b_end - b_begin;
      __syncthreads();
    }
  }

  // One visit of block b: lane = row.
  __device__ __forceinline__ void visit_block(uint32_t b, bool cached, uint32_t t_draw, double beta,
                                              SweepSums<M> &sums) {
    const uint32_t p = b * 64u + lane;
    bool reuse = false;
    if (cached) {
      reuse = (__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(dirty[b])) & ((1u << M) - 1u)) == 0u;
      // fields unchanged and every proposal certain to be rejected again: nothing to do
      if (reuse && __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(inert[b])) != 0u) return;
    }
    // {first slab, exact width}: one broadcast LDS read (bit-packed: two scalar loads, the rounded width)
    const uint2 info = PACKED ? make_uint2(static_cast<uint32_t>(a.ell_off[b]), a.block_width[b]) : meta[b];
    // wave-uniform by construction; readfirstlane makes the loop control scalar
    const uint32_t width = __builtin_amdgcn_readfirstlane(info.y);
    const uint32_t quads = (width + 3u) >> 2;
    // info.x = first slab of the block (a multiple of 4): quad index = slab / 4
    const uint64_t first_quad = __builtin_amdgcn_readfirstlane(info.x) >> 2;
    const uint4 *col = reinterpret_cast<const uint4 *>(a.ell_col) + first_quad * 64u;
    const double2 *val = reinterpret_cast<const double2 *>(a.ell_val) + first_quad * 128u;
    const BlockStream stream{col + lane, block_rsrc(col), block_rsrc(val), lane * 16u};
    // issued now, consumed after the row sum: their latency hides under the k-loop
    const uint32_t spin = a.spin_of_pos[p];
    const double h = a.field_pos[p];
    double acc[M];
    // Field cache: when the workgroup is in cached mode and no neighbour of this block's
    // spins has flipped since the block was last evaluated (dirty byte clear), the row
    // sums are read back from HBM — the very same f64 values the k-loop would produce.
    double *cache_row = nullptr;
    if (cached) {
      cache_row = a.field_cache + ((static_cast<uint64_t>(group) * a.num_blocks + b) * M) * 64u + lane;
    }
    if (reuse) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m] = cache_row[m * 64];
    } else {
      block_row_sums<M, LAYOUT, kExactLoop>(stream, width, spins, acc, mult);
      if (cached) {
#pragma unroll
        for (int m = 0; m < M; ++m) cache_row[m * 64] = acc[m];
        if (lane == 0) dirty[b] = 0;  // nobody marks a block during its own colour step
      }
    }
    const uint32_t own = load_own<LAYOUT>(spins, p, b);
    bool open;
    const uint32_t flip = accept(acc, h, own, spin, t_draw, beta, sums, open);
    store_flip<M, LAYOUT>(spins, p, b, own, flip);
    if (cached) {
      const bool none_open = __ballot(open) == 0ull;
      if (lane == 0) inert[b] = none_open ? 1 : 0;
    }
    if (cached && __ballot(flip != 0) != 0ull) {
      // Every neighbour of a flipped spin sits in a block of ANOTHER colour: mark those
      // blocks stale for the replicas that flipped.  The row's columns are streamed again
      // (columns only); in cached mode flips are rare by construction.
      uint32_t *dirty_words = reinterpret_cast<uint32_t *>(dirty);
      for (uint32_t q = 0; q < quads; ++q) {
        const uint4 c4 = stream.cptr[q * 64u];
        if (flip) {
          const uint32_t cols[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // padding entries point at the lane itself; wide columns are byte addresses
            if (cols[j] == (WIDE ? p * 4u : p)) continue;
            const uint32_t blk = cols[j] >> (WIDE ? 8 : 6);
            atomicOr(&dirty_words[blk >> 2], flip << (8u * (blk & 3u)));
          }
        }
      }
    }
  }

  // ---- The exact (integer) reduction of the sweep's energy change ----
  // Sums between registers with the totals in lane 63, and only in a wavefront some lane of which
  // accepted a flip in this sweep: in every other one each lane holds 0 flips and an energy
  // change of 0 (kLeanBook: q = visits * 0x4338000000000000 exactly, a proposal that is not
  // accepted adds the bare constant), and nothing would be added below.  The flip counts travel two
  // to a 64-bit sum: a lane accepts at most one flip per block, so the low count's total stays
  // below 64 * num_blocks < 2^32 and never carries into the high one.
  __device__ __forceinline__ void reduce(const SweepSums<M> &sums) {
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) any |= sums.n[m];
    if (__ballot(any != 0) != 0ull) {
#pragma unroll
      for (int m0 = 0; m0 < M; m0 += 2) {
        unsigned long long v[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 2 && m0 + j < M; ++j) {
          // kLeanBook: the visits' constants off, modulo 2^64 (the true sum fits: the plan's S)
          v[j] = wave_sum_lane63_u64(kLeanBook ? sums.q[m0 + j] - sums.visits * 0x4338000000000000ull
                                               : sums.q[m0 + j]);
        }
        const unsigned long long n2 = wave_sum_lane63_u64(
            sums.n[m0] |
            (m0 + 1 < M ? static_cast<unsigned long long>(sums.n[m0 + 1 < M ? m0 + 1 : m0]) << 32 : 0ull));
        if (lane == 63) {
#pragma unroll
          for (int j = 0; j < 2 && m0 + j < M; ++j) {
            const uint32_t n = static_cast<uint32_t>(n2 >> (32 * j));
            if (n != 0) {
              atomicAdd(reinterpret_cast<unsigned long long *>(&delta[m0 + j]), v[j]);
              atomicAdd(reinterpret_cast<unsigned long long *>(&book[16 + m0 + j]),
                        static_cast<unsigned long long>(n));
              if (TAIL || cache_available) atomicAdd(&ctl[kCtlFlips], n);
            }
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- End of sweep t: the mode of the next sweep, the books, the snapshot of what improved.  True
  // when the launch ends here (StopWhenStill). ----
  __device__ __forceinline__ bool end_of_sweep(uint32_t t, double beta) {
    if ((TAIL || cache_available) && tid == 0) {
      bool leave_now = false;
      if constexpr (TAIL) {
        // a certain rejection is only certain for non-decreasing beta, and the rows that are not
        // listed rest on it
        leave_now = t + 1u < a.num_sweeps && a.betas[t + 1u] < beta;
      }
      end_of_sweep_mode<TAIL>(ctl, TAIL ? tail.enter_flips : a.cache_enter_flips, leave_now);
    }
    if (tid < M) {
      const long long e = book[tid] + delta[tid];
      book[tid] = e;
      delta[tid] = 0;
      if (a.trace != nullptr) {
        a.trace[(static_cast<uint64_t>(group) * M + tid) * (a.num_sweeps + 1ull) + t + 1u] = e;
      }
      if (e < book[8 + tid]) {
        book[8 + tid] = e;
        atomicOr(improved_flag, 1u << tid);
        // (a segment's epilogue writes the best of those that improved at least once in the launch)
        if constexpr (kLazyBest && Res::kEnabled) atomicOr(improved_flag + 1, 1u << tid);
      }
    }
    __syncthreads();
    if constexpr (DESCENT && Stop::kEnabled) {
      // book[16]: flips of the chain so far — complete since the barrier after the reduction, next
      // written in the following sweep's reduction (colour barriers away).  Workgroup-uniform.
      // A sweep without a flip left the configuration as the last snapshot holds it.
      static_assert(M == 1, "one chain decides when the workgroup stops");
      const long long flips = book[16];
      if (flips == flips_before) {
        sweeps_done = t + 1u;
        return true;
      }
      flips_before = flips;
    }
    if constexpr (kLazyBest) {
      const uint32_t improved = __builtin_amdgcn_readfirstlane(*improved_flag);
      if (improved) clear_differs(spins, a.num_blocks, improved);
    } else {
      const uint32_t improved = DESCENT ? ((1u << M) - 1u) : *improved_flag;
      if (improved) snapshot<M, LAYOUT>(spins, a, group, improved);
    }
    // entering the mode: every block starts stale / every row is listed
    if ((TAIL || cache_available) && ctl[kCtlModeEntered] != 0) {
      if constexpr (TAIL) {
        fill_blocks(todo, a.num_blocks, ~uint64_t{0});
      } else {
        fill_blocks(dirty, a.num_blocks, uint8_t{0xFF});
      }
    }
    __syncthreads();
    if (tid == 0) {
      *improved_flag = 0;  // next write to it is two barriers away
      if (TAIL || cache_available) ctl[kCtlModeEntered] = 0;
    }
    return false;
  }

  // ---- Epilogue: what the launch reports ----
  __device__ __forceinline__ void epilogue() {
    if (TAIL && tid == 0) {
      tail.report[2ull * group] = ctl[kCtlTailSweeps];
      tail.report[2ull * group + 1u] = ctl[kCtlTailEntries];
    }
    if (tid < M) {
      a.tracked[static_cast<uint64_t>(group) * M + tid] = book[8 + tid];
      a.accepted[static_cast<uint64_t>(group) * M + tid] = static_cast<unsigned long long>(book[16 + tid]);
    }
    if constexpr (DESCENT && Stop::kEnabled) {
      if (tid == 0) *stop.sweeps_done = sweeps_done;
    }
    if constexpr (kLazyBest) {
      // The best configurations, from the words (last written before the final barriers).  A closed call
      // reports every replica's — one that never improved has d = start against current, its start
      // configuration —; a segment only those it improved on: the others' stand in a.best_perm already.
      uint32_t mask = (1u << M) - 1u;
      if constexpr (Res::kEnabled) mask = __builtin_amdgcn_readfirstlane(improved_flag[1]);
      materialise_best<M>(spins, a, group, mask);
    }
    if constexpr (Res::kEnabled) {
      // the state the next segment starts from (the spins were last written before the final barriers)
      if (tid < M) res.e_cur[static_cast<uint64_t>(group) * M + tid] = book[tid];
      snapshot<M, LAYOUT>(spins, FinalWords{res.cur_perm, a.num_blocks}, group, (1u << M) - 1u);
    }
  }
};

template <int M, bool DESCENT, int LAYOUT, typename Args, typename Stop = NoEarlyStop,
          typename Res = NoResume, bool ALIGNED = false, bool TAIL = false>
__device__ __forceinline__ void sa_sweep_body(const Args &a, const uint32_t group,
                                              const Stop stop = Stop{}, const Res res = Res{},
                                              const TailArgs tail = TailArgs{}) {
  ColourSweep<M, DESCENT, LAYOUT, Args, Stop, Res, ALIGNED, TAIL> sweep(a, group, stop, res, tail);
  sweep.start();
  for (uint32_t t = 0; t < a.num_sweeps; ++t) {
    uint32_t t_draw = t;  // the sweep index of the random words: global over the segments of a handle
    if constexpr (Res::kEnabled) t_draw += res.t0;
    double beta = 0.0;  // (a descent — dE >= 0 is a certain rejection at any beta — and a ladder segment read none)
    if constexpr (!DESCENT && !Res::kLadder) beta = a.betas[t];
    SweepSums<M> sums{};
    bool listed_only = false;
    if constexpr (TAIL) listed_only = sweep.tail_sweep(t_draw, beta, sums);
    if (!listed_only) sweep.colour_sweep(t, t_draw, beta, sums);
    sweep.reduce(sums);
    if (sweep.end_of_sweep(t, beta)) break;
  }
  sweep.epilogue();
}

template <int M, bool DESCENT, int LAYOUT, bool ALIGNED = false>
__global__ __launch_bounds__(kMaxThreads) void k_sa_sweep(SweepArgs a) {
  sa_sweep_body<M, DESCENT, LAYOUT, SweepArgs, NoEarlyStop, NoResume, ALIGNED>(a, blockIdx.x);
}

// The closed call of four chains per group with tail sweeps (the TAIL form of the body), in bytes and words.
template <int LAYOUT, bool ALIGNED>
__global__ __launch_bounds__(kMaxThreads) void k_sa_sweep_tail(SweepArgs a, TailArgs tail) {
  sa_sweep_body<4, false, LAYOUT, SweepArgs, NoEarlyStop, NoResume, ALIGNED, true>(a, blockIdx.x, NoEarlyStop{},
                                                                                    NoResume{}, tail);
}

// One segment of an asp_sa_chains handle in the colour order: Res = Resume (asp_sa_chains_advance, order 0)
// or ResumeLadder (asp_sa_chains_advance_ladder, order 0).
template <int M, int LAYOUT, typename Res>
__global__ __launch_bounds__(kMaxThreads) void k_sa_sweep_resume(SweepArgs a, Res r) {
  sa_sweep_body<M, false, LAYOUT, SweepArgs, NoEarlyStop, Res>(a, blockIdx.x, NoEarlyStop{}, r);
}

// Many problems in one launch, by descriptor (BatchArgs, sa_colour.hpp).
template <int M, int LAYOUT, typename Problem>
__global__ __launch_bounds__(kMaxThreads) void k_sa_sweep_batch(BatchArgs<Problem> b) {
  const BatchSlot slot = b.slots[(blockIdx.x & 7u) * b.slots_per_xcd + (blockIdx.x >> 3)];
  const uint32_t problem = __builtin_amdgcn_readfirstlane(slot.problem);
  if (problem == 0xFFFFFFFFu) return;
  // The descriptor is read through the CONSTANT address space, like kernel arguments: the
  // compiler may then re-load a field where it needs it instead of keeping all forty of them in
  // registers (as a by-value copy it spilled SGPRs into VGPR lanes and VGPRs to scratch:
  // 128 VGPRs + 68 B of scratch against the single-problem kernel's 112 and none; +8 %).
  using ConstProblem = const Problem __attribute__((address_space(4)));
  ConstProblem *d = reinterpret_cast<ConstProblem *>(reinterpret_cast<uintptr_t>(b.problems + problem));
  // how the body runs each descriptor
  if constexpr (std::is_same_v<Problem, SweepArgs>) {
    sa_sweep_body<M, false, LAYOUT>(*d, __builtin_amdgcn_readfirstlane(slot.group));
  } else if constexpr (std::is_same_v<Problem, DescentProblem>) {
    sa_sweep_body<M, true, LAYOUT>(d->s, 0u, StopWhenStill{d->sweeps_done});
  } else if constexpr (std::is_same_v<Problem, ResumeProblem>) {
    sa_sweep_body<M, false, LAYOUT>(d->s, __builtin_amdgcn_readfirstlane(slot.group), NoEarlyStop{},
                                    Resume{d->r.cur_perm, d->r.e_cur, d->r.t0});
  } else {
    sa_sweep_body<M, false, LAYOUT>(d->s, __builtin_amdgcn_readfirstlane(slot.group), NoEarlyStop{},
                                    ResumeLadder{d->r.cur_perm, d->r.e_cur, d->r.t0, d->r.chain_betas});
  }
}

// ---------------------------------------------------------------------------
// Team sweep: ONE chain spread over G workgroups (few chains on a large cluster)
// ---------------------------------------------------------------------------
// With fewer chains than compute units a chain bound to one workgroup leaves most of the chip
// idle and pays ceil(blocks of a colour / 16) rounds per colour step.  Here the G workgroups of a
// team each keep the whole configuration (bit-packed, LDS), visit every G-th slice of a colour's
// blocks, publish the 64-bit flip word of each block they visited, meet at a device-scope
// barrier and XOR the other members' flip words into their own copy.  Energy bookkeeping is
// summed over the team through parity-buffered atomics.  All workgroups must be resident together
// (the launcher keeps the grid within the CU count and serialises team launches); the barrier
// carries a watchdog so that neither a bug nor a busy device can hang the GPU — on a timeout
// the call is repeated without teams.  Chains are bit-identical to k_sa_sweep's.  (TeamArgs: sa_colour.hpp.)

__device__ __forceinline__ void team_barrier(const TeamArgs &ta, unsigned long long *counter,
                                             unsigned long long &target) {
  // The exchange buffers are fine-grained (uncached, coherent across XCDs) and only touched with
  // device-scope atomics, so no cache write-back/invalidate is needed — a release/acquire fence
  // at agent scope flushes the whole L2 of the XCD on this chip and costs ~20 us.  Ordering:
  // every wavefront first waits for the acknowledgement of its own outstanding stores and
  // atomics (a workgroup-scope barrier alone does not: within a CU the vector L1 is shared, so
  // hipcc emits no vmcnt wait for it), then the workgroup barrier, then thread 0 announces the
  // arrival.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  target += ta.team_size;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t polls = 0;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (__hip_atomic_load(ta.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
      if (++polls > ta.spin_limit) {
        __hip_atomic_store(ta.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(kTeamSleep);
    }
  }
  __syncthreads();
}

// DESCENT as in k_sa_sweep: accept iff dE < 0, no random numbers, snapshot after every sweep.
template <bool DESCENT>
__global__ __launch_bounds__(1024) void k_sa_sweep_team(TeamArgs ta) {
  const SweepArgs &a = ta.s;
  extern __shared__ __align__(16) uint8_t lds[];
  uint64_t *words = reinterpret_cast<uint64_t *>(lds);  // sign bits, one word per block
  // book: [0] current tracked energy, [1] best, [2] this workgroup's dq, [3] its accepted flips,
  // [4] accepted flips of the chain so far
  long long *book = reinterpret_cast<long long *>(lds + static_cast<size_t>(a.num_blocks) * 8u);
  uint32_t *improved = reinterpret_cast<uint32_t *>(book + 5);
  // ctl[0]: 1 while the team tracks which blocks are untouched ("tracking": few flips per
  // sweep), ctl[1]: 1 in the sweep tracking was switched on.  Then per block a dirty byte (a
  // neighbour flipped since the block's last evaluation) and an inert byte (its last evaluation
  // was all certain rejections) — the bookkeeping of k_sa_sweep's cached mode without the cached
  // fields: a clean inert block is skipped, everything else is evaluated in full.
  uint32_t *ctl = improved + 1;
  uint8_t *dirty = reinterpret_cast<uint8_t *>(ctl + 3);
  uint8_t *inert = dirty + ((a.num_blocks + 15u) & ~15u);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = blockDim.x >> 6;
  const uint32_t G = ta.team_size;
  // members of a team are num_teams apart: the same XCD when num_teams is a multiple of 8
  const uint32_t team = blockIdx.x % ta.num_teams, member = blockIdx.x / ta.num_teams;
  const uint32_t r = a.replica_first + team;
  const uint32_t key0 = static_cast<uint32_t>(a.seed), key1 = static_cast<uint32_t>(a.seed >> 32);
  uint64_t *flipbuf = ta.flips + static_cast<uint64_t>(team) * a.num_blocks;
  unsigned long long *counter = ta.arrivals + team;
  unsigned long long target = 0;

  // every member builds the same initial configuration
  for (uint32_t b0 = wave; b0 < a.num_blocks; b0 += waves) {
    const uint32_t p = b0 * 64u + lane;
    const uint32_t spin = a.spin_of_pos[p];
    uint32_t negative = 0;
    if (spin != kDummySpin) {
      if (a.x0_perm != nullptr) {
        negative = static_cast<uint32_t>((a.x0_perm[p >> 6] >> (p & 63u)) & 1ull);
      } else {
        const Philox4 rnd = philox4x32_10(spin, 0xFFFFFFFFu, r >> 2, 0u, key0, key1);
        negative = (pick_word(rnd, r & 3u) & 1u) ^ 1u;
      }
    }
    const uint64_t word = __ballot(negative);
    if (lane == 0) words[b0] = word;
  }
  if (tid < 5) book[tid] = 0;
  if (tid == 0) {
    *improved = 0;
    ctl[0] = 0;
    ctl[1] = 0;
  }
  __syncthreads();
  if (member == 0) {
    for (uint32_t w = tid; w < a.num_blocks; w += blockDim.x) {
      a.best_perm[static_cast<uint64_t>(team) * a.num_blocks + w] = words[w];
    }
  }

  double mult[4] = {1.0, 1.0, 1.0, 1.0};  // (accumulate's kWide multipliers: unused by kBits)
  for (uint32_t t = 0; t < a.num_sweeps; ++t) {
    const double beta = a.betas[t];
    const bool tracking = __builtin_amdgcn_readfirstlane(ctl[0]) != 0;
    if (tracking && t > 0 && beta < a.betas[t - 1]) {
      // certain rejections are only certain for non-decreasing beta (team-uniform branch)
      for (uint32_t b = tid; b < a.num_blocks; b += blockDim.x) inert[b] = 0;
      __syncthreads();
    }
    long long q_acc = 0;
    uint32_t n_acc = 0;
    for (uint32_t c = 0; c < a.num_colors; ++c) {
      const uint32_t b_begin = a.color_block_start[c];
      const uint32_t b_end = a.color_block_start[c + 1];
      for (uint32_t b = b_begin + member * waves + wave; b < b_end; b += G * waves) {
        if (tracking && __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(dirty[b])) == 0u &&
            __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(inert[b])) != 0u) {
          // nothing around this block moved and every proposal was a certain rejection
          if (lane == 0) {
            __hip_atomic_store(flipbuf + b, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          continue;
        }
        const uint32_t p = b * 64u + lane;
        const uint32_t quads = a.block_width[b] >> 2;
        const uint64_t first_quad = a.ell_off[b] >> 2;
        const uint4 *cptr = reinterpret_cast<const uint4 *>(a.ell_col) + first_quad * 64u + lane;
        const double2 *vptr =
            reinterpret_cast<const double2 *>(a.ell_val) + first_quad * 128u + lane;
        const uint32_t spin = a.spin_of_pos[p];
        const double h = a.field_pos[p];
        double acc[1] = {0.0};
        Quad qa, qb;
        load_quad(qa, cptr, vptr, 0);
        uint32_t i = 0;
        for (; i + 2 <= quads; i += 2) {
          load_quad(qb, cptr, vptr, i + 1);
          __builtin_amdgcn_sched_barrier(0);
          accumulate<1, kBits>(qa, lds, acc, mult);
          __builtin_amdgcn_sched_barrier(0);
          load_quad(qa, cptr, vptr, i + 2);
          __builtin_amdgcn_sched_barrier(0);
          accumulate<1, kBits>(qb, lds, acc, mult);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (i < quads) accumulate<1, kBits>(qa, lds, acc, mult);
        const bool valid = spin != kDummySpin;
        const bool negative = (words[b] >> lane) & 1ull;
        const double g = __dadd_rn(acc[0], h);
        const double de = __dmul_rn(negative ? 2.0 : -2.0, g);
        bool accept;
        // this lane's proposal is not a certain rejection
        const bool open = DESCENT ? (valid && de < 0.0)
                                  : (valid && !(__dmul_rn(beta, de) >= 23.0));
        if constexpr (DESCENT) {
          accept = valid && de < 0.0;
        } else {
          const Philox4 rnd = philox4x32_10(spin, t, r >> 2, 0u, key0, key1);
          const uint32_t word = pick_word(rnd, r & 3u);
          accept = valid && (de <= 0.0 || metropolis_accept_word(word, __dmul_rn(beta, de)));
        }
        if (accept) {
          q_acc += __double_as_longlong(__dadd_rn(__dmul_rn(de, a.scale), 0x1.8p52)) -
                   0x4338000000000000ll;
          n_acc += 1;
        }
        const uint64_t flips = __ballot(accept);
        if (lane == 0) {
          if (flips != 0) words[b] ^= flips;
          __hip_atomic_store(flipbuf + b, flips, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tracking) {
          const bool none_open = __ballot(open) == 0ull;
          if (lane == 0) {
            dirty[b] = 0;  // nobody marks a block during its own colour step
            inert[b] = none_open ? 1 : 0;
          }
          if (flips != 0) {
            // the neighbours of a flipped spin sit in blocks of other colours: stale now
            for (uint32_t q = 0; q < quads; ++q) {
              const uint4 c4 = cptr[q * 64u];
              if (accept) {  // (padding entries point at the lane's own position)
                if (c4.x != p) dirty[c4.x >> 6] = 1;
                if (c4.y != p) dirty[c4.y >> 6] = 1;
                if (c4.z != p) dirty[c4.z >> 6] = 1;
                if (c4.w != p) dirty[c4.w >> 6] = 1;
              }
            }
          }
        }
      }
      if (c + 1u == a.num_colors) {
        // the sweep's energy change rides on the last colour's barrier (integers: order-free)
        const long long v = wave_sum_i64(q_acc);
        const long long n = wave_sum_i64(static_cast<long long>(n_acc));
        if (lane == 0 && n != 0) {
          atomicAdd(reinterpret_cast<unsigned long long *>(&book[2]), static_cast<unsigned long long>(v));
          atomicAdd(reinterpret_cast<unsigned long long *>(&book[3]), static_cast<unsigned long long>(n));
        }
        __syncthreads();
        if (tid == 0) {
          long long *mine = ta.sums + (static_cast<uint64_t>(team) * 3u + t % 3u) * 2u;
          if (book[3] != 0) {
            __hip_atomic_fetch_add(&mine[0], book[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&mine[1], book[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          book[2] = 0;
          book[3] = 0;
        }
      }
      team_barrier(ta, counter, target);
      // the other members' flips of this colour step: XOR them in and, when tracking, mark the
      // blocks of the flipped spins' neighbours (a wavefront per flipped block, lane = row)
      if (tracking) {
        for (uint32_t i = wave; i < b_end - b_begin; i += waves) {
          if ((i / waves) % G == member) continue;
          const uint32_t b = b_begin + i;
          const uint64_t flips =
              __hip_atomic_load(flipbuf + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (flips == 0) continue;  // wave-uniform
          if (lane == 0) words[b] ^= flips;
          const uint32_t quads = a.block_width[b] >> 2;
          const uint4 *cptr =
              reinterpret_cast<const uint4 *>(a.ell_col) + (a.ell_off[b] >> 2) * 64u + lane;
          const bool flipped = (flips >> lane) & 1ull;
          for (uint32_t q = 0; q < quads; ++q) {
            const uint4 c4 = cptr[q * 64u];
            if (flipped) {
              const uint32_t p = b * 64u + lane;
              if (c4.x != p) dirty[c4.x >> 6] = 1;
              if (c4.y != p) dirty[c4.y >> 6] = 1;
              if (c4.z != p) dirty[c4.z >> 6] = 1;
              if (c4.w != p) dirty[c4.w >> 6] = 1;
            }
          }
        }
      } else {
        for (uint32_t i = tid; i < b_end - b_begin; i += blockDim.x) {
          if ((i / waves) % G != member) {
            const uint64_t flips = __hip_atomic_load(flipbuf + b_begin + i, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
            if (flips != 0) words[b_begin + i] ^= flips;
          }
        }
      }
      __syncthreads();
    }

    // ---- bookkeeping of the sweep: the team sums were exchanged with the last colour ----
    long long *mine = ta.sums + (static_cast<uint64_t>(team) * 3u + t % 3u) * 2u;
    long long *other = ta.sums + (static_cast<uint64_t>(team) * 3u + (t + 2u) % 3u) * 2u;
    if (tid == 0) {
      const long long dq = __hip_atomic_load(&mine[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long dn = __hip_atomic_load(&mine[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long e = book[0] + dq;
      book[0] = e;
      book[4] += dn;
      const bool better = e < book[1];
      if (better) book[1] = e;
      *improved = (better || DESCENT) ? 1u : 0u;
      // tracking pays while the flips of a sweep touch a fraction of the blocks (the same
      // hysteresis as the field cache; dn is the team-wide count, so all members agree)
      const bool was = ctl[0] != 0;
      const bool now = was ? dn < 2ll * a.cache_enter_flips : dn < static_cast<long long>(a.cache_enter_flips);
      ctl[0] = now ? 1u : 0u;
      ctl[1] = (now && !was) ? 1u : 0u;
      // three rotating slots: the one cleared here was read a sweep ago and is next added to
      // two sweeps from now, with team barriers on either side; one member clears it
      if (member == 0) {
        __hip_atomic_store(&other[0], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&other[1], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    if (*improved != 0u && member == 0) {
      for (uint32_t w = tid; w < a.num_blocks; w += blockDim.x) {
        a.best_perm[static_cast<uint64_t>(team) * a.num_blocks + w] = words[w];
      }
    }
    if (ctl[1] != 0u) {  // tracking starts with the next sweep: every block is stale
      for (uint32_t b = tid; b < a.num_blocks; b += blockDim.x) {
        dirty[b] = 1;
        inert[b] = 0;
      }
    }
    __syncthreads();
  }
  if (member == 0 && tid == 0) {
    a.tracked[team] = book[1];
    a.accepted[team] = static_cast<unsigned long long>(book[4]);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Which kernel runs in which shape
// ---------------------------------------------------------------------------

namespace {

// A FORM of the sweep kernel: M chains per group (one workgroup) in layout LAYOUT.
template <int M, int LAYOUT>
struct Form {
  static constexpr int kM = M, kLayout = LAYOUT;
  static constexpr bool is(int m, int layout) { return m == M && layout == LAYOUT; }
};
template <typename... Forms>
struct FormList {};
// Every form there is.  A kernel family below has these or a subset of them and nothing else, so that a
// resumed, ladder or batched run takes a form the closed call has.
using ColourForms = FormList<Form<1, kBytes>, Form<2, kBytes>, Form<4, kBytes>, Form<8, kBytes>,  // eight chains: bytes only
                             Form<4, kWide>, Form<4, kNibbles>,    // a word, four bits per position: four chains
                             Form<1, kBits>, Form<1, kGlobal>>;    // a bit per position: one chain per workgroup

template <typename... Forms>
constexpr bool form_listed(FormList<Forms...>, int m, int layout) {
  return (Forms::is(m, layout) || ...);
}
constexpr bool colour_form_exists(int m, int layout) { return form_listed(ColourForms{}, m, layout); }
static_assert(colour_form_exists(1, kBytes) && colour_form_exists(2, kBytes) && colour_form_exists(4, kBytes) &&
                  colour_form_exists(8, kBytes) && !colour_form_exists(0, kBytes) && !colour_form_exists(3, kBytes) &&
                  !colour_form_exists(16, kBytes),
              "1, 2, 4 or 8 chains per group in the byte layout");
static_assert(colour_form_exists(4, kWide) && colour_form_exists(4, kNibbles) && !colour_form_exists(1, kWide) &&
                  !colour_form_exists(2, kWide) && !colour_form_exists(8, kWide) && !colour_form_exists(1, kNibbles) &&
                  !colour_form_exists(2, kNibbles) && !colour_form_exists(8, kNibbles),
              "a word and four bits per position: four chains per group");
static_assert(colour_form_exists(1, kBits) && colour_form_exists(1, kGlobal) && !colour_form_exists(2, kBits) &&
                  !colour_form_exists(4, kBits) && !colour_form_exists(2, kGlobal) && !colour_form_exists(4, kGlobal),
              "a bit per position, in LDS or in HBM: one chain per workgroup");

// A group of four replicas that starts on a multiple of four is one whole Philox call (the ALIGNED
// form of sa_sweep_body): any sharding of the chains by multiples of four.  Eight replicas stay
// generic: an aligned visit of two calls back to back needed 36 B of scratch against 28 B.
bool aligned_replicas(int m, uint32_t replica_first) { return m == 4 && replica_first % 4u == 0; }

// A kernel FAMILY gives the kernel of a form, Family::of<Form>(), for the forms it has<Form>().
// The closed call: every form; strict descent (DESCENT) in the forms of one chain, the ALIGNED variant
// (aligned_replicas() holds for the launch) in those of four; every other kernel is the generic one,
// which is right for any first replica.
template <bool DESCENT, bool ALIGNED>
struct ClosedFamily {
  using Kernel = void (*)(SweepArgs);
  template <typename F>
  static constexpr bool has() {
    return DESCENT ? (F::kM == 1 && !ALIGNED) : (!ALIGNED || F::kM == 4);
  }
  template <typename F>
  static Kernel of() {
    return k_sa_sweep<F::kM, DESCENT, F::kLayout, ALIGNED>;
  }
};
// A handle's segment (Res = Resume) or ladder segment (ResumeLadder): every form of the closed call, no teams.
template <typename Res>
struct SegmentFamily {
  using Kernel = void (*)(SweepArgs, Res);
  template <typename F>
  static constexpr bool has() {
    return true;
  }
  template <typename F>
  static Kernel of() {
    return k_sa_sweep_resume<F::kM, F::kLayout, Res>;
  }
};
// The shared launches of many problems, by descriptor: closed anneals (SweepArgs) in every form with the
// spins in LDS; segments and ladder segments in bytes up to four chains and words (a cluster beyond
// a byte per position runs alone); descents as one chain in bytes.
template <typename Problem>
struct BatchFamily {
  using Kernel = void (*)(BatchArgs<Problem>);
  template <typename F>
  static constexpr bool has() {
    if (std::is_same_v<Problem, SweepArgs>) return F::kLayout != kGlobal;
    if (std::is_same_v<Problem, DescentProblem>) return F::kM == 1 && F::kLayout == kBytes;
    return (F::kLayout == kBytes && F::kM <= 4) || F::kLayout == kWide;
  }
  template <typename F>
  static Kernel of() {
    return k_sa_sweep_batch<F::kM, F::kLayout, Problem>;
  }
};

// The family's kernel for m chains per group in `layout`, or nullptr: no such form (in this family).
template <typename Family, typename... Forms>
typename Family::Kernel colour_kernel_in(FormList<Forms...>, int m, int layout) {
  typename Family::Kernel kernel = nullptr;
  auto take = [&](auto form) {
    using F = decltype(form);
    if constexpr (Family::template has<F>()) {
      if (F::is(m, layout)) kernel = Family::template of<F>();
    }
  };
  (take(Forms{}), ...);
  return kernel;
}
template <typename Family>
typename Family::Kernel colour_kernel_of(int m, int layout) {
  return colour_kernel_in<Family>(ColourForms{}, m, layout);
}

}  // namespace

namespace asp {
namespace colour {

bool colour_form_listed(int m, int layout) { return colour_form_exists(m, layout); }

ClosedKernel closed_kernel_of(int m, bool descent, int layout, uint32_t replica_first) {
  if (descent) return colour_kernel_of<ClosedFamily<true, false>>(m, layout);
  if (aligned_replicas(m, replica_first)) return colour_kernel_of<ClosedFamily<false, true>>(m, layout);
  return colour_kernel_of<ClosedFamily<false, false>>(m, layout);
}
template <typename Res>
SegmentKernel<Res> segment_kernel_of(int m, int layout) {
  return colour_kernel_of<SegmentFamily<Res>>(m, layout);
}
template SegmentKernel<Resume> segment_kernel_of<Resume>(int, int);
template SegmentKernel<ResumeLadder> segment_kernel_of<ResumeLadder>(int, int);
template <typename Problem>
BatchKernel<Problem> batch_kernel_of(int m, int layout) {
  return colour_kernel_of<BatchFamily<Problem>>(m, layout);
}
template BatchKernel<SweepArgs> batch_kernel_of<SweepArgs>(int, int);
template BatchKernel<DescentProblem> batch_kernel_of<DescentProblem>(int, int);
template BatchKernel<ResumeProblem> batch_kernel_of<ResumeProblem>(int, int);
template BatchKernel<LadderProblem> batch_kernel_of<LadderProblem>(int, int);
TeamKernel team_kernel_of(bool descent) { return descent ? k_sa_sweep_team<true> : k_sa_sweep_team<false>; }

// The dynamic LDS of a launch (SweepLds::total): a kernel without tail sweeps, or (tail) k_sa_sweep_tail
// with `threads` threads.  (32-bit offsets: 2^20 blocks are far beyond any LDS in every layout that keeps
// something per block.)
size_t sweep_lds_bytes(const asp::SaHostLayout &L, int layout, bool tail, int threads) {
  if (layout != kGlobal && L.num_blocks > (1u << 20)) return SIZE_MAX;
  return SweepLds(L.num_blocks, layout, tail, static_cast<uint32_t>(threads / 64)).total;
}

// Tail sweeps after a sweep with fewer flips of the workgroup than this (asp_sa_set_tail's automatic
// value): a flip lists ~degree rows, so c * num_spins / degree flips list the fraction c of all rows at
// the most.  A listed row costs several times what a row of a block visit costs — its loads touch a cache
// line per lane where a block visit touches eight per instruction —, so c is small: 0.05 was the fastest
// of 0.00625 .. 0.4 at K = 3e4 and 1e5 (profiles/tail_timing.txt).  With about one block
// per wavefront and colour (K = 1e4 on 16 wavefronts) a tail visit replaces one block visit at best: there
// 0.0125 would be 1 % faster and 0.05 is 0 - 2 % behind the kernel without tail sweeps.
constexpr double kTailEnterShare = 0.05;
uint32_t tail_enter_flips_of(const asp::SaHostLayout &L) {
  const double degree = std::max(1.0, static_cast<double>(L.a_col.size()) / static_cast<double>(L.num_spins));
  return static_cast<uint32_t>(std::max(1.0, kTailEnterShare * static_cast<double>(L.num_spins) / degree));
}

// The TAIL kernel of a closed call in `form`, or nullptr: the launch keeps the kernel without tail sweeps
// of the same form — tail sweeps or the field cache off, another form than four chains in bytes or words,
// no room in the LDS for the bitmap and the rings, or arrays beyond the 32-bit buffer offsets of a row.
TailKernel tail_kernel_of(const asp_sa_plan *p, int m, int threads, int layout, bool descent, uint32_t replica_first) {
  const asp::SaHostLayout &L = p->host;
  if (p->tail_mode == 0 || !p->use_field_cache || descent || m != 4 || (layout != kBytes && layout != kWide)) {
    return nullptr;
  }
  if (sweep_lds_bytes(L, layout, true, threads) > p->max_lds) return nullptr;
  if (L.ell_val.size() * sizeof(double) >= (1ull << 32)) return nullptr;
  const bool aligned = replica_first % 4u == 0;
  if (layout == kWide) return aligned ? k_sa_sweep_tail<kWide, true> : k_sa_sweep_tail<kWide, false>;
  return aligned ? k_sa_sweep_tail<kBytes, true> : k_sa_sweep_tail<kBytes, false>;
}

// k_sa_sweep_team: sign words | book, flags (64 B) | dirty[num_blocks] | inert[num_blocks]
size_t team_lds_bytes(const asp::SaHostLayout &L) {
  return static_cast<size_t>(L.num_blocks) * 8 + 64 +
         2 * (((static_cast<size_t>(L.num_blocks) + 15) / 16) * 16);
}

// blocks of the largest colour class
uint32_t widest_color(const asp::SaHostLayout &L) {
  uint32_t widest = 1;
  for (uint32_t c = 0; c < L.num_colors; ++c) {
    widest = std::max(widest, L.color_block_start[c + 1] - L.color_block_start[c]);
  }
  return widest;
}

// Launch geometry: as many replicas per group as still leaves one group per CU,
// as many wavefronts as a colour class has blocks.
static void choose_launch(const asp_sa_plan *p, uint32_t repetitions, int *m_out, int *threads_out) {
  const uint32_t widest = widest_color(p->host);
  int m = 1;
  bool two_per_cu = false;
  if (p->force_m) {
    m = p->force_m;
  } else {
    for (int cand : {8, 4, 2}) {
      if ((repetitions + cand - 1) / cand >= static_cast<uint32_t>(p->num_cus)) {
        m = cand;
        break;
      }
    }
    // Small clusters with chains to spare: two workgroups of four replicas per CU, eight
    // wavefronts each, fill the thin rounds of one another (K = 1e4, 2048 chains: 209 -> 228
    // G flips/s against eight replicas in one workgroup; the reverse from ~50 blocks per colour)
    if (m == 8 && widest <= 32 && !p->force_threads) {
      m = 4;
      two_per_cu = true;
    }
  }
  int threads = p->force_threads;
  if (two_per_cu) threads = 512;
  if (!threads) {
    // one wavefront per block of the LARGEST colour class (DSATUR classes are skewed, the
    // first is the biggest), at most 16
    // (round 1 preferred 12 wavefronts below ~80 blocks per colour; with this round's accept
    // phase 16 are faster at every size: K = 1e4 180 -> 198 G flips/s, 3e4 238 -> 253, two boxes)
    const uint32_t most = 16u;
    threads = static_cast<int>(std::min<uint32_t>(widest, most)) * 64;
  }
  *m_out = m;
  *threads_out = threads;
}

// a bit per position, in LDS or in HBM (forced by asp_sa_set_packed or chosen: the launch is the same)
bool bit_packed(int layout) { return layout == kBits || layout == kGlobal; }
ColourLaunch choose_colour_launch(const asp_sa_plan *p, uint32_t repetitions, bool descent, bool traced) {
  const asp::SaHostLayout &L = p->host;
  ColourLaunch c;
  choose_launch(p, repetitions, &c.m, &c.threads);
  if (descent) c.m = 1;
  // One byte per position when that fits the LDS; otherwise one BIT per position, one replica
  // per workgroup (flips applied by wavefront ballot) — 8x the capacity.
  bool packed = p->force_packed != 0, nibbles = false;
  if (!packed && sweep_lds_bytes(L, kBytes) > p->spin_lds()) {
    // ... or, with chains enough for four per workgroup, four bits per position: twice the
    // capacity of bytes and still four replicas sharing every coupling load
    if (!descent && !traced && c.m >= 4 && sweep_lds_bytes(L, kNibbles) <= p->spin_lds()) {
      nibbles = true;
      c.m = 4;
    } else {
      packed = true;
    }
  }
  // not even a bit per position fits the LDS: keep the words in HBM (no size limit, slow)
  const bool global = p->force_packed == 2 || (packed && sweep_lds_bytes(L, kBits) > p->spin_lds());
  if (packed) c.m = 1;
  // A word per position (SDWA sign trick) when four replicas share the
  // workgroup and the words fit; results do not depend on the layout.
  // (measured: +2..12 % with four replicas per workgroup, nothing with two)
  const bool wide = !packed && !nibbles && !descent && p->allow_wide && c.m == 4 && p->ell_col4.ptr != nullptr &&
                    sweep_lds_bytes(L, kWide) <= p->spin_lds();
  c.layout = global ? kGlobal : (packed ? kBits : (nibbles ? kNibbles : (wide ? kWide : kBytes)));
  return c;
}

// Few chains on a large cluster: spread each chain over a team of workgroups (k_sa_sweep_team).
uint32_t choose_team(const asp_sa_plan *p, const ColourLaunch &form, uint32_t repetitions, bool traced) {
  const asp::SaHostLayout &L = p->host;
  uint32_t team = 0;
  const uint32_t widest = widest_color(L);
  // (one colour class only — a diagonal or field-only J —: the single barrier per sweep would
  // not separate a fast member's next publication from a slow member's read of this one)
  const bool possible = !traced && form.layout != kGlobal && form.layout != kNibbles && p->force_packed == 0 &&
                        L.num_colors >= 2 && p->force_m == 0 && team_lds_bytes(L) <= p->max_lds &&
                        static_cast<uint64_t>(repetitions) * 2 <= static_cast<uint64_t>(p->num_cus);
  if (possible && p->team_mode >= 2) {
    team = static_cast<uint32_t>(p->team_mode);  // forced (tests, measurements)
  } else if (possible && p->team_mode < 0 && widest >= 64) {
    // auto: as many workgroups per chain as the chip has to spare, up to 8
    const uint32_t spare = static_cast<uint32_t>(p->num_cus) / repetitions;
    team = spare >= 8 ? 8u : (spare >= 4 ? 4u : 2u);
    while (team > 2 && widest < 16u * team) team >>= 1;  // every member needs a full round
  }
  if (team * repetitions > static_cast<uint32_t>(p->num_cus)) team = 0;  // must be co-resident
  return team;
}

// The plan's part of the sweep arguments (the same for every launch of the plan in `layout`) ...
static SweepArgs plan_sweep_args(const asp_sa_plan *p, int layout) {
  const asp::SaHostLayout &L = p->host;
  SweepArgs plan_args{};
  plan_args.color_block_start = p->color_block_start.ptr;
  plan_args.block_width = p->block_width.ptr;
  plan_args.ell_off = p->ell_off.ptr;
  plan_args.ell_col = layout == kWide ? p->ell_col4.ptr : p->ell_col.ptr;
  plan_args.ell_val = p->ell_val.ptr;
  plan_args.spin_of_pos = p->spin_of_pos.ptr;
  plan_args.field_pos = p->field_pos.ptr;
  plan_args.scale = std::ldexp(1.0, L.energy_scale_exp);
  plan_args.num_colors = L.num_colors;
  plan_args.num_blocks = L.num_blocks;
  plan_args.spin_words = layout == kGlobal ? p->w_spins.ptr : nullptr;
  return plan_args;
}
// ... and with the call's: the schedule, the start (nullptr: all spins up, or a segment's own), the outputs,
// the seed and the sweep / replica counts.  The trace and the field cache stay off: the caller's.
SweepArgs sweep_args(const asp_sa_plan *p, int layout, const double *betas, const uint64_t *x0_perm,
                     uint64_t *best_perm, long long *tracked, unsigned long long *accepted, uint64_t seed,
                     uint32_t num_sweeps, uint32_t replica_first) {
  SweepArgs args = plan_sweep_args(p, layout);
  args.betas = betas;
  args.x0_perm = x0_perm;
  args.best_perm = best_perm;
  args.tracked = tracked;
  args.accepted = accepted;
  args.seed = seed;
  args.num_sweeps = num_sweeps;
  args.replica_first = replica_first;
  return args;
}

// Switch the field cache on after a sweep with fewer flips than this: a flip stales ~degree blocks,
// and cached mode pays while that is a fraction of all blocks.
uint32_t cache_enter_flips_of(const asp::SaHostLayout &L) {
  const double degree = std::max(1.0, static_cast<double>(L.a_col.size()) / static_cast<double>(L.num_spins));
  return static_cast<uint32_t>(std::max(1.0, 0.7 * static_cast<double>(L.num_blocks) / degree));
}

// What asp_sa_anneal_batch and the batched segments (sa_chains_advance_colour_batch) decide alike, in
// one place: the wavefront counts of the launch classes, and the layout and wavefronts of a problem
// that fits a byte per position (the thresholds are measured; see asp_sa_anneal_batch).
constexpr uint64_t kBatchWideMax = 10000, kBatchSmallMax = 10000;

int batch_waves_index(uint32_t waves) {
  for (int c = 0; c < kNumBatchWaves; ++c) {
    if (waves <= kBatchWaves[c]) return c;
  }
  return kNumBatchWaves - 1;
}
int batch_layout_in_lds(const asp_sa_plan *p) {  // kWide or kBytes
  const asp::SaHostLayout &L = p->host;
  return p->allow_wide && p->ell_col4.ptr && L.num_spins <= kBatchWideMax && sweep_lds_bytes(L, kWide) <= p->spin_lds()
             ? kWide
             : kBytes;
}
uint32_t batch_waves(const asp::SaHostLayout &L) {
  return std::min<uint32_t>(widest_color(L), L.num_spins <= kBatchSmallMax ? 4u : 16u);
}

// Chains per workgroup of a batch.  Measured on the production mix (K log-uniform in [1e2, 1e4], 64
// chains x 5120 sweeps): four replicas per workgroup — the word layout with its one-instruction signs —
// is fastest from 64 problems (86 G flips/s against 73 with two) over 128 (127 against 101
// with eight, 95 with two, 62 with one) to 512 (161, the same as eight); fewer replicas per
// workgroup only when four would leave SIMDs without a wavefront.  Nibble and bit entries count at their
// fixed group sizes.
int batch_chains_per_group(const std::vector<BatchEntry> &entries, int num_cus) {
  for (int cand : {4, 2}) {
    uint64_t waves = 0;
    for (const BatchEntry &e : entries) {
      const uint32_t per_group = e.layout == kBits ? 1 : (e.layout == kNibbles ? 4 : cand);
      waves += static_cast<uint64_t>((e.chains + per_group - 1) / per_group) *
               kBatchWaves[batch_waves_index(e.waves)];
    }
    if (waves >= static_cast<uint64_t>(num_cus) * 4u) return cand;
  }
  return 1;
}

}  // namespace colour
}  // namespace asp
