// The row sums of a quad of couplings, as the colour sweep's k-loop and k_sa_post run them: the +-1.0
// multiplier of a term from a neighbour's spin byte or word, the quad-interleaved ELL stream through
// buffer loads, and accumulate().  Device code that csrc/sa_sweep.hip and csrc/sa_energy.hip share;
// what only one of them uses lives in that file.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sa_device.hpp"

namespace asp {
namespace colour {

using namespace dev;  // the spin layouts, LdsByte, LdsWord

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
// TERMS < 4: the partial form, the quad's first TERMS terms only — gathers and FMAs alike (accumulate_last).
template <int M, int LAYOUT, int TERMS = 4>
__device__ __forceinline__ void accumulate(const Quad &q, const uint8_t *spins, double (&acc)[M],
                                           double (&mult)[4]) {
  static_assert(TERMS >= 1 && TERMS <= 4, "a quad holds four terms");
  const uint32_t cs[4] = {q.c.x, q.c.y, q.c.z, q.c.w};
  const double vs[4] = {q.v01.x, q.v01.y, q.v23.x, q.v23.y};
  uint32_t s[4];
#pragma unroll
  for (int j = 0; j < TERMS; ++j) {
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
  for (int j = 0; j < TERMS; ++j) {
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

// The LAST quad of a block whose longest row ends inside it: `last_terms` = exact width & 3 (1, 2 or 3
// real terms; 0: all four).  Wave-uniform — a scalar branch, no lane mask — so the terms past the longest
// row, which are padding in all 64 lanes, cost neither a gather nor an FMA.  The sums keep their bits: a
// dropped term is fma(+0.0, +-1.0, acc) = acc + (+-0.0) (the plan pads values with +0.0), which is acc for
// every acc but -0.0, and acc is never -0.0: it starts as +0.0 and a sum rounds to -0.0 only when both of
// its addends are -0.0 (x + (-x) is +0.0 in round-to-nearest).  The real terms are added in ascending k,
// as before.
template <int M, int LAYOUT>
__device__ __forceinline__ void accumulate_last(const Quad &q, uint32_t last_terms, const uint8_t *spins,
                                                double (&acc)[M], double (&mult)[4]) {
  if constexpr (LAYOUT == kWide) {
    // Words: every term rewrites the held multipliers in place.  As four bodies of their own hipcc copied
    // the eight registers into each body and out of it again (12 v_mov per visit: what the dropped terms
    // save); one body with early exits keeps them where they are.  The gathers go first, as in accumulate.
    const uint32_t cs[4] = {q.c.x, q.c.y, q.c.z, q.c.w};
    const double vs[4] = {q.v01.x, q.v01.y, q.v23.x, q.v23.y};
    uint32_t s[4] = {0u, 0u, 0u, 0u};
    s[0] = *reinterpret_cast<LdsWord *>(static_cast<uintptr_t>(cs[0]));
    if (last_terms != 1u) {
      s[1] = *reinterpret_cast<LdsWord *>(static_cast<uintptr_t>(cs[1]));
      if (last_terms != 2u) {
        s[2] = *reinterpret_cast<LdsWord *>(static_cast<uintptr_t>(cs[2]));
        if (last_terms != 3u) s[3] = *reinterpret_cast<LdsWord *>(static_cast<uintptr_t>(cs[3]));
      }
    }
    auto term = [&](int j) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m] = __builtin_fma(vs[j], wide_factor_held(s[j], m, mult[m & 3]), acc[m]);
    };
    term(0);
    if (last_terms == 1u) return;
    term(1);
    if (last_terms == 2u) return;
    term(2);
    if (last_terms == 3u) return;
    term(3);
  } else {
    switch (last_terms) {
      case 1: accumulate<M, LAYOUT, 1>(q, spins, acc, mult); break;
      case 2: accumulate<M, LAYOUT, 2>(q, spins, acc, mult); break;
      case 3: accumulate<M, LAYOUT, 3>(q, spins, acc, mult); break;
      default: accumulate<M, LAYOUT, 4>(q, spins, acc, mult); break;
    }
  }
}

}  // namespace colour
}  // namespace asp
