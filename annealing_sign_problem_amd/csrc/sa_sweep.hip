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
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <numeric>
#include <type_traits>
#include <vector>

#include "asp_common.hpp"
#include "greedy.hpp"
#include "sa_device.hpp"
#include "sa_internal.hpp"
#include "sa_plan.hpp"

namespace {

using asp::DeviceBuffer;
using asp::kDummySpin;
using asp::upload_vector;
using namespace asp::dev;  // Philox, the accept filter, the spin layouts (sa_device.hpp)

constexpr int kMaxThreads = 1024;  // launch bound of the sweep kernel (VGPR budget = 512 / waves per SIMD)
constexpr int kTeamSleep = 4;  // s_sleep argument between two polls of the team barrier (0/1/4/16/64 scanned)

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

// v with its sign flipped when bit 0 of `neg` is set (energy kernel, not hot).
__device__ __forceinline__ double signed_coupling(double v, uint32_t neg, int m) {
  const unsigned long long flip = static_cast<unsigned long long>((neg >> m) & 1u) << 63;
  return __longlong_as_double(__double_as_longlong(v) ^ static_cast<long long>(flip));
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

// Butterfly sum over the 64 lanes; every lane ends with the balanced-tree total
// ((v0+v1)+(v2+v3))+... (f64 addition commutes, so all lanes agree bitwise).
__device__ __forceinline__ double wave_tree_sum_f64(double v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v = __dadd_rn(v, __shfl_xor(v, step, 64));
  return v;
}

// Collect bit m of each of the four bytes of d into a nibble (byte 0 -> bit 0).
__device__ __forceinline__ uint32_t gather_bit4(uint32_t d, int m) {
  const uint32_t t = (d >> m) & 0x01010101u;
  return ((t * 0x00204081u) >> 21) & 0xFu;
}

// kBytes with M <= 4 keeps replica m at bit 2m of the spin byte (the odd bits stay 0); M = 8
// fills the byte and keeps bit m.  With the even bits the high word of the term's +-1.0 is
//   (byte << (31 - 2m)) | 0x3FF00000   (one v_lshl_or_b32)
// for every m: bit 2m lands on bit 31, the higher replica bits leave the word, the lower ones
// land on bits 29, 27 or 25 (already 1 in 0x3FF00000) and bit 30 receives an odd bit, always 0.
// With bit m = replica m that shift drags replica m - 1 into bit 30.  Replica MASKS (flip, the
// dirty and inert bytes, snapshot's `mask`) stay indexed by replica; encode_replicas() turns
// one into spin-byte bits where it meets the byte.
template <int M, int LAYOUT>
constexpr bool kEvenBits = LAYOUT == kBytes && M <= 4;

template <int M, int LAYOUT>
__device__ __forceinline__ constexpr int replica_bit(int m) {
  return kEvenBits<M, LAYOUT> ? 2 * m : m;
}

template <int M, int LAYOUT>
__device__ __forceinline__ uint32_t encode_replicas(uint32_t mask) {
  if constexpr (kEvenBits<M, LAYOUT>) {
    return (mask & 1u) | ((mask & 2u) << 1) | ((mask & 4u) << 2) | ((mask & 8u) << 3);
  } else {
    return mask;
  }
}

// +-1.0 with the sign taken from replica m's bit of a neighbour's spin byte (1 -> -1.0).
// acc = fma(v, +-1.0, acc) is bit-identical to acc + (+-v): the product is exact, so the only
// rounding is the add's; the low dword of the multiplier is a constant zero.
//   even-bit bytes: one v_lshl_or_b32 (above) that the compiler schedules (plain C++: no inline
//     asm, so no hazard padding);
//   bit m (bytes at M = 8, nibbles, bits): replica m's bit to bit 0 with a RIGHT shift — a plain
//     VOP2, 2.5 SIMD cycles per wave64 on this chip, where every left shift and every VOP3 costs
//     4.3-4.4 (profiles/r02_issue_rate_probe.txt) — then the m = 0 instruction.
template <int M, int LAYOUT>
__device__ __forceinline__ double spin_factor(uint32_t spin_byte, int m) {
  uint32_t hi;
  if constexpr (kEvenBits<M, LAYOUT>) {
    hi = (spin_byte << (31 - 2 * m)) | 0x3FF00000u;
  } else if (m == 0) {
    hi = (spin_byte << 31) | 0x3FF00000u;  // v_lshl_or_b32: nothing but bit 0 survives the shift
  } else {
    const uint32_t down = spin_byte >> m;
    asm("v_lshl_or_b32 %0, %1, 31, %2" : "=v"(hi) : "v"(down), "s"(0x3FF00000u));
  }
  return __hiloint2double(static_cast<int>(hi), 0);
}

// kWide: byte m of `word` (0x00 / 0x80) OR 0x3F becomes byte 3 of `hi`, whose lower three bytes
// keep 0xF00000 — i.e. hi = high word of +1.0 or -1.0 — in one v_or_b32_sdwa (byte select on
// the source, byte-3 write with the rest preserved).  Two VALU ops per (term, replica)
// instead of three.
__device__ __forceinline__ double wide_factor(uint32_t word, int m, uint32_t &hi) {
  const uint32_t top = 0x3Fu;
  switch (m) {
    case 0:
      asm("v_or_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
          "src1_sel:BYTE_0" : "+v"(hi) : "v"(top), "v"(word));
      break;
    case 1:
      asm("v_or_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
          "src1_sel:BYTE_1" : "+v"(hi) : "v"(top), "v"(word));
      break;
    case 2:
      asm("v_or_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
          "src1_sel:BYTE_2" : "+v"(hi) : "v"(top), "v"(word));
      break;
    default:
      asm("v_or_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
          "src1_sel:BYTE_3" : "+v"(hi) : "v"(top), "v"(word));
      break;
  }
  return __hiloint2double(static_cast<int>(hi), 0);
}

// The SDWA of wide_factor rewrites the top byte of a multiplier held as a whole f64 whose low
// word stays 0 for the whole anneal (rebuilt from `hi` and a literal 0, as wide_factor returns
// it, the pair was re-assembled and low words re-zeroed inside the k-loop).
__device__ __forceinline__ double wide_factor_held(uint32_t word, int m, double &mult) {
  uint32_t hi = static_cast<uint32_t>(__double2hiint(mult));
  wide_factor(word, m, hi);
  mult = __hiloint2double(static_cast<int>(hi), __double2loint(mult));
  return mult;
}

// Four consecutive ELL entries of one lane (one row), k = 4q .. 4q+3.
struct Quad {
  uint4 c;
  double2 v01, v23;
};

// Three 16-byte loads per lane through pointers (the team kernel); quad index `quad` is relative
// to the block's first quad.
__device__ __forceinline__ void load_quad(Quad &q, const uint4 *__restrict__ cptr,
                                          const double2 *__restrict__ vptr, uint32_t quad) {
  q.c = cptr[quad * 64u];
  q.v01 = vptr[quad * 128u];
  q.v23 = vptr[quad * 128u + 64u];
}

// The ELL stream of one block through BUFFER loads: the resource's base is the block's first
// quad (scalar, set up once per visit), the quad is a scalar offset (quad * 1024 B of columns,
// quad * 2048 B of values) and the lane part a vector offset fixed for the whole kernel, so a
// quad costs no vector address arithmetic.  Offsets are relative to the block, so any plan size
// fits the 32-bit offsets.  `cptr`: the lane's columns through a plain pointer, for the dirty
// marking that re-reads them after a flip.
using BufferRsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ BufferRsrc block_rsrc(const void *base) {
  // raw buffer, 4 GiB range, gfx9 DATA_FORMAT word
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0xFFFFFFFF, 0x00020000);
}
struct BlockStream {
  const uint4 *cptr;
  BufferRsrc col, val;
  uint32_t lane16;  // lane * 16
};

__device__ __forceinline__ void load_quad(Quad &q, const BlockStream &s, uint32_t quad) {
  q.c = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(s.col, s.lane16, quad * 1024u, 0));
  q.v01 = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(s.val, s.lane16, quad * 2048u, 0));
  q.v23 = __builtin_bit_cast(double2,
                             __builtin_amdgcn_raw_buffer_load_b128(s.val, s.lane16 + 1024u, quad * 2048u, 0));
}

// The row sums of one quad: the four neighbours' spins are gathered, then neighbour-major FMAs
// (consecutive FMAs go to different accumulators; each acc[m] still receives its terms in
// ascending k).  `mult`: kWide's held multipliers (wide_factor_held), untouched by the others.
template <int M, int LAYOUT>
__device__ __forceinline__ void accumulate(const Quad &q, const uint8_t *spins, double (&acc)[M],
                                           double (&mult)[4]) {
  const uint32_t cs[4] = {q.c.x, q.c.y, q.c.z, q.c.w};
  const double vs[4] = {q.v01.x, q.v01.y, q.v23.x, q.v23.y};
  uint32_t s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (LAYOUT == kBytes) {
      // even-bit bytes and bytes at M = 8: the spin bytes start at LDS address 0 (checked in the
      // kernel prologue), so a position IS its LDS address — no base add in front of every
      // ds_read_u8
      s[j] = *reinterpret_cast<LdsByte *>(static_cast<uintptr_t>(cs[j]));
    } else if constexpr (LAYOUT == kWide) {
      // columns of the wide plan are LDS byte addresses (position * 4)
      s[j] = *reinterpret_cast<LdsWord *>(static_cast<uintptr_t>(cs[j]));
    } else if constexpr (LAYOUT == kNibbles) {
      // position c: byte c / 2, nibble c % 2; the bits above replica m's are ignored by spin_factor
      const uint32_t byte = *reinterpret_cast<LdsByte *>(static_cast<uintptr_t>(cs[j] >> 1));
      s[j] = byte >> ((cs[j] & 1u) << 2);
    } else if constexpr (LAYOUT == kBits) {
      const uint32_t *words = reinterpret_cast<const uint32_t *>(spins);
      s[j] = (words[cs[j] >> 5] >> (cs[j] & 31u)) & 1u;
    } else {
      static_assert(LAYOUT == kGlobal, "spins are LDS bytes, words, nibbles or bits, or bits in HBM");
      // words written by other wavefronts of the workgroup during earlier colour steps: read at
      // device scope (past the CU's vector L1)
      const uint32_t *words = reinterpret_cast<const uint32_t *>(spins);
      const uint32_t w = __hip_atomic_load(words + (cs[j] >> 5), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      s[j] = (w >> (cs[j] & 31u)) & 1u;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if constexpr (LAYOUT == kWide) {
        acc[m] = __builtin_fma(vs[j], wide_factor_held(s[j], m, mult[m & 3]), acc[m]);
      } else {
        acc[m] = __builtin_fma(vs[j], spin_factor<M, LAYOUT>(s[j], m), acc[m]);
      }
    }
  }
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
// meta[b] = {first ELL slab, width} of block b.  ctl: the CtlSlot words below.
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
// ahead of the accumulate it overlaps.  For an even quad count the last load reads one quad past the
// block — the next block's first slabs or the tail padding the plan appends — and is never consumed.
template <int M, int LAYOUT>
__device__ __forceinline__ void block_row_sums(const BlockStream &stream, uint32_t quads, const uint8_t *spins,
                                               double (&acc)[M], double (&mult)[4]) {
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
  Quad qa, qb;
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
    }
    if constexpr (!PACKED) {
      for (uint32_t b = tid; b < a.num_blocks; b += blockDim.x) {
        meta[b] = make_uint2(static_cast<uint32_t>(a.ell_off[b]), a.block_width[b]);
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
      row_quads = info.y >> 2;
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
    // {first slab, width}: one broadcast LDS read (two scalar loads when bit-packed)
    const uint2 info = PACKED ? make_uint2(static_cast<uint32_t>(a.ell_off[b]), a.block_width[b]) : meta[b];
    // wave-uniform by construction; readfirstlane makes the loop control scalar
    const uint32_t quads = __builtin_amdgcn_readfirstlane(info.y) >> 2;
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
      block_row_sums<M, LAYOUT>(stream, quads, spins, acc, mult);
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
// the call is repeated without teams.  Chains are bit-identical to k_sa_sweep's.

// team launches of the process that the barrier's watchdog cut short (asp_sa_team_watchdog_trips)
std::atomic<uint64_t> g_team_watchdog_trips{0};

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

// Barrier polls before the watchdog gives up and the call is repeated without teams: ~ 5 s (a
// barrier normally completes in ~ 5 us; members can only be kept waiting by other kernels
// holding compute units — team launches themselves take turns).
constexpr uint32_t kTeamSpinLimit = 1u << 22;

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

// ---------------------------------------------------------------------------
// Energy of packed configurations: E = D + T, T = radix-64
// pairwise tree over the blocks of t_p = s_p (A_p . s / 2 + h_p).
// ---------------------------------------------------------------------------

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
struct PostArgs {
  EnergyArgs e;
  const uint32_t *pos_of_spin;
  uint64_t *x;  // nullptr, or [count][words] configurations in original order (bit = +1)
  uint64_t num_spins;
  uint32_t words;
};

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
struct PostProblem {
  EnergyArgs e;  // perm_words / partial: this problem's rows
  const uint32_t *pos_of_spin;
  uint64_t num_spins;
  uint32_t words;
  double diag_sum;
  double *out_e;    // [repetitions]
  uint64_t *out_x;  // [repetitions][words]
};

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

// ---------------------------------------------------------------------------
// Plan object and C ABI
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
ClosedFamily<false, false>::Kernel closed_kernel_of(int m, bool descent, int layout, uint32_t replica_first) {
  if (descent) return colour_kernel_of<ClosedFamily<true, false>>(m, layout);
  if (aligned_replicas(m, replica_first)) return colour_kernel_of<ClosedFamily<false, true>>(m, layout);
  return colour_kernel_of<ClosedFamily<false, false>>(m, layout);
}

// The dynamic LDS of a launch (SweepLds::total): a kernel without tail sweeps, or (tail) k_sa_sweep_tail
// with `threads` threads.  (32-bit offsets: 2^20 blocks are far beyond any LDS in every layout that keeps
// something per block.)
size_t sweep_lds_bytes(const asp::SaHostLayout &L, int layout, bool tail = false, int threads = 0) {
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
using TailKernel = void (*)(SweepArgs, TailArgs);
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
void choose_launch(const asp_sa_plan *p, uint32_t repetitions, int *m_out, int *threads_out) {
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

// Chains per group, threads and spin layout of a launch with one workgroup per group of chains —
// shared by the closed calls (run_chains, which may then spread a chain over a team instead) and by
// the segments of a handle (sa_chains_advance_colour), so that both take the same form.
struct ColourLaunch {
  int m = 1, threads = 64, layout = kBytes;
};
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

// The plan's part of the sweep arguments (the same for every launch of the plan in `layout`) ...
SweepArgs plan_sweep_args(const asp_sa_plan *p, int layout) {
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

// The field cache of `padded` chains (512 B per block and replica), when it fits comfortably in HBM.
void attach_field_cache(asp_sa_plan *p, uint64_t padded, SweepArgs *args) {
  const asp::SaHostLayout &L = p->host;
  const uint64_t cache_elems = padded * L.num_blocks * 64ull;
  if (cache_elems * sizeof(double) <= (32ull << 30) && p->w_field_cache.ensure(cache_elems) == ASP_OK) {
    args->field_cache = p->w_field_cache.ptr;
    args->cache_enter_flips = cache_enter_flips_of(L);
  } else {
    asp_clear_error();  // the cache is an optimisation: run without it
  }
}

// out_x: nullptr, or [count][ceil(K/64)] — the configurations in original order (bit = +1) as well:
// written by k_sa_post where it runs, by k_unpermute_bits behind the older energy kernels.
int energies_of_perm(asp_sa_plan *p, const uint64_t *perm_words, uint32_t count, double *partial,
                     double *out_e, uint64_t *out_x = nullptr) {
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
  if (out_x != nullptr) {
    hipLaunchKernelGGL(k_unpermute_bits,
                       dim3((words + 3) / 4, (count + kUnpermuteChains - 1) / kUnpermuteChains), dim3(256),
                       0, p->stream, perm_words, L.num_blocks, p->pos_of_spin.ptr, L.num_spins, words,
                       count, out_x);
  }
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

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
  return energies_of_perm(p, perm, count, partial, out_e);
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
  if (replicas_per_group != 0 && !colour_form_exists(replicas_per_group, kBytes)) {
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

namespace {

int greedy_relax(asp_sa_plan *p, uint32_t max_sweeps, std::vector<uint64_t> &x, uint64_t *out_x,
                 double *out_e, uint32_t *out_sweeps, bool exact_sweeps);

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
  void (*team_kernel)(TeamArgs) = descent ? k_sa_sweep_team<true> : k_sa_sweep_team<false>;
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

// All chains of one call; descent = strict-descent sweeps (greedy relaxation).
int run_chains(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
               uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0, bool descent,
               uint64_t *out_x, double *out_e, int64_t *out_trace = nullptr) {
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  ASP_TRY(asp::bind_device());
  if (repetitions == 0) return ASP_OK;
  if (!out_x || !out_e || (num_sweeps && !betas)) {
    return asp::set_error(ASP_ERR_INVALID, "null argument");
  }
  if (num_sweeps == 0xFFFFFFFFu) {
    return asp::set_error(ASP_ERR_INVALID, "num_sweeps 2^32-1 is reserved");
  }
  if (static_cast<uint64_t>(replica_offset) + repetitions + 8 > 0xFFFFFFFFull) {
    return asp::set_error(ASP_ERR_INVALID, "replica ids exceed 32 bits");
  }
  for (uint32_t t = 0; t < num_sweeps; ++t) {
    if (!(betas[t] >= 0.0)) return asp::set_error(ASP_ERR_INVALID, "betas[%u] is not >= 0", t);
  }
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  const uint32_t words = static_cast<uint32_t>((K + 63) / 64);
  p->last_sweep_ms = p->last_total_ms = 0.0f;
  if (K == 0) {
    for (uint32_t r = 0; r < repetitions; ++r) out_e[r] = 0.0;
    return ASP_OK;
  }
  ColourLaunch form = choose_colour_launch(p, repetitions, descent, out_trace != nullptr);
  // Few chains on a large cluster: spread each chain over a team of workgroups (k_sa_sweep_team).
  uint32_t team = 0;
  {
    const uint32_t widest = widest_color(L);
    // (one colour class only — a diagonal or field-only J —: the single barrier per sweep would
    // not separate a fast member's next publication from a slow member's read of this one)
    const bool possible = !out_trace && form.layout != kGlobal && form.layout != kNibbles && p->force_packed == 0 &&
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
  }
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
  const uint64_t K = L.num_spins;
  const uint32_t words = c->words, repetitions = c->repetitions;
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
    ASP_TRY(run.launch(colour_kernel_of<SegmentFamily<ResumeLadder>>(run.m, run.layout),
                       ResumeLadder{p->w_cur_perm.ptr, p->w_e_cur.ptr, c->sweeps_done, p->w_betas.ptr}));
  } else {
    ASP_TRY(run.launch(colour_kernel_of<SegmentFamily<Resume>>(run.m, run.layout),
                       Resume{p->w_cur_perm.ptr, p->w_e_cur.ptr, c->sweeps_done}));
  }
  const dim3 grid((words + 3) / 4, (repetitions + kUnpermuteChains - 1) / kUnpermuteChains);
  hipLaunchKernelGGL(k_unpermute_bits, grid, dim3(256), 0, s, p->w_cur_perm.ptr, L.num_blocks,
                     p->pos_of_spin.ptr, K, words, repetitions, c->x_cur.ptr);
  hipLaunchKernelGGL(k_unpermute_bits, grid, dim3(256), 0, s, p->w_best.ptr, L.num_blocks,
                     p->pos_of_spin.ptr, K, words, repetitions, c->x_best.ptr);
  ASP_HIP_TRY(hipGetLastError());
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

namespace {

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

}  // namespace

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
  ASP_TRY(energies_of_perm(p, d_perm.ptr, count, d_partial.ptr, d_e.ptr));
  ASP_TRY(d_e.download(out_e, count, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  return ASP_OK;
}

}  // extern "C"

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

thread_local float g_batch_sweep_ms = 0.0f;

// What asp_sa_anneal_batch and the batched segments (sa_chains_advance_colour_batch) decide alike, in
// one place: the wavefront counts of the launch classes, and the layout and wavefronts of a problem
// that fits a byte per position (the thresholds are measured; see asp_sa_anneal_batch).
constexpr uint32_t kBatchWaves[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int kNumBatchWaves = sizeof kBatchWaves / sizeof kBatchWaves[0];
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
  void (*kernel)(BatchArgs<Problem>);
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

struct BatchEntry {
  uint32_t item;     // index into the caller's array
  uint32_t waves;    // wavefronts per workgroup this problem wants
  int layout;        // kWide or kBytes; the closed batch: kNibbles or kBits as well
  double work;       // ~ time of one group: sweeps * ELL slabs
  uint64_t beta_at;  // offset of its schedule (a ladder segment: its chains' betas) in the concatenated betas
};

// Chains per workgroup of a batch.  Measured on the production mix (K log-uniform in [1e2, 1e4], 64
// chains x 5120 sweeps): four replicas per workgroup — the word layout with its one-instruction signs —
// is fastest from 64 problems (86 G flips/s against 73 with two) over 128 (127 against 101
// with eight, 95 with two, 62 with one) to 512 (161, the same as eight); fewer replicas per
// workgroup only when four would leave SIMDs without a wavefront.  Nibble and bit entries count at their
// fixed group sizes.  chains_of(e.item): the chains of an entry.
template <typename ChainsOf>
int batch_chains_per_group(const std::vector<BatchEntry> &entries, int num_cus, ChainsOf chains_of) {
  for (int cand : {4, 2}) {
    uint64_t waves = 0;
    for (const BatchEntry &e : entries) {
      const uint32_t per_group = e.layout == kBits ? 1 : (e.layout == kNibbles ? 4 : cand);
      waves += static_cast<uint64_t>((chains_of(e.item) + per_group - 1) / per_group) *
               kBatchWaves[batch_waves_index(e.waves)];
    }
    if (waves >= static_cast<uint64_t>(num_cus) * 4u) return cand;
  }
  return 1;
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
    if (!it.out_x || !it.out_e || (it.num_sweeps && !it.betas)) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: null argument", i);
    }
    if (it.num_sweeps == 0xFFFFFFFFu) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: num_sweeps 2^32-1 is reserved", i);
    }
    if (it.flags & ~static_cast<uint32_t>(ASP_SA_BATCH_SHUFFLED)) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: unknown flags 0x%x", i, it.flags);
    }
    if (static_cast<uint64_t>(it.replica_offset) + it.repetitions + 8 > 0xFFFFFFFFull) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: replica ids exceed 32 bits", i);
    }
    for (uint32_t t = 0; t < it.num_sweeps; ++t) {
      if (!(it.betas[t] >= 0.0)) {
        return asp::set_error(ASP_ERR_INVALID, "item %u: betas[%u] is not >= 0", i, t);
      }
    }
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
    const int m = batch_chains_per_group(entries, num_cus, [&](uint32_t i) { return items[i].repetitions; });
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
  if (n_cache * sizeof(double) > (32ull << 30)) use_cache = false;

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
  if (use_cache && d_cache.alloc(n_cache) != ASP_OK) {
    asp_clear_error();  // the cache is an optimisation: run without it
    use_cache = false;
  }
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
    return ClassKernel<SweepArgs>{colour_kernel_of<BatchFamily<SweepArgs>>(m_of_class[c], layout_of_class(c)),
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
    p->last_m = m_of_class[c];
    p->last_layout = p->last_spin_layout = layout_of_class(c);
    p->last_threads = static_cast<int>(64u * waves_of_class(c));
    p->last_groups = static_cast<int>(off[k].groups);
    p->last_sweep_ms = p->last_total_ms = 0.0f;  // shared launches: see asp_sa_batch_last_ms
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
  const int m = batch_chains_per_group(entries, segs[entries[0].item].chains->plan->num_cus,
                                       [&](uint32_t i) { return segs[i].chains->repetitions; });
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
  if (n_cache * sizeof(double) > (32ull << 30)) use_cache = false;

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
  if (use_cache && d_cache.alloc(n_cache) != ASP_OK) {
    asp_clear_error();  // the cache is an optimisation: run without it
    use_cache = false;
  }
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
  hipLaunchKernelGGL(k_chains_permute_problems, dim3(static_cast<unsigned>(h_chains_in.size())), dim3(256), 0, s,
                     d_io.ptr, d_chains_in.ptr);
  ASP_HIP_TRY(hipGetLastError());
  // ---- one sweep launch per class ----
  ASP_TRY(launcher.run(s, d_problems.ptr, d_slots.ptr, [&](int cl) {
    return ClassKernel<Problem>{colour_kernel_of<BatchFamily<Problem>>(cl % 2 == 0 ? 4 : m, cl % 2 == 0 ? kWide : kBytes),
                                64u * kWaves[cl / 2]};
  }));
  // ---- the state back into the handles (after the attempt: the colour order has no retry) ----
  hipLaunchKernelGGL(k_chains_unpermute_problems, dim3(static_cast<unsigned>(h_chains_out.size())), dim3(256), 0, s,
                     d_io.ptr, d_chains_out.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.0f;
  ASP_HIP_TRY(hipEventElapsedTime(&ms, launcher.begin, launcher.end));
  if (sweep_ms) *sweep_ms += ms;
  for (size_t k = 0; k < entries.size(); ++k) {
    asp_sa_plan *p = segs[entries[k].item].chains->plan;
    const int cl = class_of(entries[k]);
    p->last_m = m;
    p->last_layout = p->last_spin_layout = cl % 2 == 0 ? kWide : kBytes;
    p->last_threads = static_cast<int>(64u * kWaves[cl / 2]);
    p->last_groups = static_cast<int>(off[k].groups);
    p->last_sweep_ms = p->last_total_ms = 0.0f;  // shared launches: see asp_sa_chains_batch_last_ms
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
  if (n_cache * sizeof(double) > (32ull << 30)) use_cache = false;
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
  if (use_cache && d_cache.alloc(n_cache) != ASP_OK) {
    asp_clear_error();  // the cache is an optimisation: run without it
    use_cache = false;
  }
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
  hipLaunchKernelGGL(k_permute_bits_problems, dim3(static_cast<unsigned>(n)), dim3(256), 0, s,
                     d_problems.ptr);
  ASP_HIP_TRY(hipGetLastError());
  // ---- one descent launch per class ----
  ASP_TRY(launcher.run(s, d_problems.ptr, d_slots.ptr, [&](int c) {
    return ClassKernel<DescentProblem>{colour_kernel_of<BatchFamily<DescentProblem>>(1, kBytes), 64u * kBatchWaves[c]};
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
    p->last_m = 1;
    p->last_layout = p->last_spin_layout = kBytes;
    p->last_threads = static_cast<int>(64u * kBatchWaves[members[k].cls]);
    p->last_groups = 1;
    p->last_sweep_ms = p->last_total_ms = 0.0f;  // shared launches: see asp_sa_greedy_batch_last_ms
  }
  return ASP_OK;
}

}  // extern "C"
