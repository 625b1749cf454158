// Device helpers that BOTH annealing sweeps use (csrc/sa_sweep.hip: colour order;
// csrc/sa_shuffled.hip: a fresh order every sweep): the Philox stream, the acceptance rule, the
// wide spin word and the spin layouts.  What only one sweep uses lives in that sweep's files (the
// colour order: csrc/sa_sweep.hip with sa_colour.hpp and sa_colour_kloop.hpp), so a change to one kernel
// leaves the other's source-set fingerprint alone (build.KERNEL_SOURCE_SETS) — and so does a change to
// the colour order's host drivers (csrc/sa_anneal.hip, csrc/sa_batch.hip) or its energy pass
// (csrc/sa_energy.hip), which are in neither set.
// Specification: DESIGN.md §4.3-4.5.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace asp {
namespace dev {

struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                 uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = static_cast<uint32_t>(p1);
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = static_cast<uint32_t>(p0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ uint32_t pick_word(const Philox4 &p, uint32_t which) {
  const uint32_t lo = (which & 1u) ? p.w[1] : p.w[0];
  const uint32_t hi = (which & 1u) ? p.w[3] : p.w[2];
  return (which & 2u) ? hi : lo;
}

// exp(-x), x >= 0: a fixed sequence of IEEE operations (v_rndne_f64, v_fma_f64,
// v_mul_f64) so that the result is bit-identical to the CPU restatement.
__device__ __forceinline__ double expneg(double x) {
  if (!(x < 23.0)) return 0.0;
  const double y = -x;
  const double kf = __builtin_rint(__dmul_rn(y, 0x1.71547652b82fep+0));
  double r = __builtin_fma(kf, -0x1.62e42fee00000p-1, y);
  r = __builtin_fma(kf, -0x1.a39ef35793c76p-33, r);
  double p = 0x1.6124613a86d09p-33;
  p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29);
  p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26);
  p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);
  p = __builtin_fma(p, r, 0x1.71de3a556c734p-19);
  p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16);
  p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);
  p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10);
  p = __builtin_fma(p, r, 0x1.1111111111111p-7);
  p = __builtin_fma(p, r, 0x1.5555555555555p-5);
  p = __builtin_fma(p, r, 0x1.5555555555555p-3);
  p = __builtin_fma(p, r, 0x1.0000000000000p-1);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  const long long k = static_cast<long long>(kf);
  const double scale = __longlong_as_double((1023ll + k) << 52);
  return __dmul_rn(p, scale);
}

// u < expneg(x) for u = (word + 0.5) * 2^-32, decided through a hardware-exp filter on the random
// WORD: u < p  <=>  word + 0.5 < p * 2^32.  v_exp_f32 of the f32-rounded argument estimates
// p = expneg(x) within |est / p - 1| <= 2.63e-6 (measured) for 0 < x < 23.  With the two f32
// products lo = est * 2^32 (1 - 2e-5), hi = est * 2^32 (1 + 2e-5) (constant and product rounding
// <= 1.3e-7 together): word < trunc(lo) implies word + 0.5 < lo < p * 2^32 (accept), word >
// trunc(hi) implies word + 0.5 > hi > p * 2^32 (reject); in between (~4e-5 of the proposals) the
// exact sequence of §4.4 decides.  The result therefore ALWAYS equals `u < expneg(x)` — same bits
// as the oracle — at a fraction of the sixteen dependent f64 FMAs.
__device__ __forceinline__ bool metropolis_accept_word(uint32_t word, double x) {
  if (!(x < 23.0)) return false;  // expneg(x) = 0 < u; also NaN
  const float estimate = __builtin_amdgcn_exp2f(static_cast<float>(x) * -1.44269504f);
  const float lo = estimate * (4294967296.0f * (1.0f - 2e-5f));  // < 2^32: conversion in range
  if (word < static_cast<uint32_t>(lo)) return true;
  const float hi = estimate * (4294967296.0f * (1.0f + 2e-5f));
  if (hi < 4294967040.0f && word > static_cast<uint32_t>(hi)) return false;
  const double u = __dmul_rn(__dadd_rn(static_cast<double>(word), 0.5), 0x1p-32);
  return u < expneg(x);
}

// Replica mask (bit m) -> wide spin word (byte m = 0x80): bits 0..3 to bits 7, 15, 23, 31.
__device__ __forceinline__ uint32_t spread_mask(uint32_t mask) {
  return ((mask & 0xFu) * 0x00204081u & 0x01010101u) << 7;
}

// The wide word of the COLOUR sweep carries one more bit per replica.  Byte m is 0x80 * s_m + d_m:
//   bit 8m + 7 = s_m, replica m's sign bit (all the shuffled sweep keeps, and all any reader of the
//                current configuration looks at);
//   bit 8m     = d_m, "replica m's spin here differs from replica m's best configuration".
// The sign instruction of the k-loop ORs the selected byte with 0x3F into the top byte of the +-1.0
// multiplier, so bits 0..5 of a byte never reach it (checked below for both values of d_m).  A flip
// toggles both bits, an improvement of replica m clears d_m at every position, and the best
// configuration is s_m ^ d_m, materialised once per launch: no copy per improving sweep.
constexpr uint32_t kWideDiffers = 0x01010101u;  // the d bits
constexpr uint32_t kWideSigns = 0x80808080u;    // the s bits
static_assert((0x3Fu | 0x00u) == 0x3Fu && (0x3Fu | 0x01u) == 0x3Fu && (0x3Fu | 0x80u) == 0xBFu &&
                  (0x3Fu | 0x81u) == 0xBFu,
              "the top byte of the multiplier is that of +1.0 or -1.0 whatever d_m is");
// Replica mask (bit m) -> the d bits of those replicas: bits 0..3 to bits 0, 8, 16, 24.
__device__ __forceinline__ uint32_t differs_mask(uint32_t mask) {
  return (mask & 0xFu) * 0x00204081u & kWideDiffers;
}
// Replica mask -> what a flip of those replicas XORs into the word: s_m and d_m (one v_lshl_or_b32
// where spread_mask has a shift).
__device__ __forceinline__ uint32_t flip_mask(uint32_t mask) {
  const uint32_t t = differs_mask(mask);
  return (t << 7) | t;
}
// Bit 8m + 7 of the result = replica m's sign bit in its BEST configuration, s_m ^ d_m.
__device__ __forceinline__ uint32_t best_signs(uint32_t word) { return word ^ (word << 7); }

// Spins addressed absolutely in LDS: the kernels check in their prologue that the dynamic LDS
// block starts at address 0, so a byte or word address of the spin area needs no base add.
using LdsByte = __attribute__((address_space(3))) const uint8_t;
using LdsWord = __attribute__((address_space(3))) const uint32_t;

// How a workgroup keeps its spins in LDS.
//   kBytes: one byte per position, bit m = sign bit of replica m (M <= 8; the colour sweep keeps
//           replica m at bit 2m for M <= 4);
//   kBits:  one bit per position, one replica (8x the capacity);
//   kWide:  one 32-bit word per position, byte m = 0x80 * sign bit of replica m (M <= 4; fits
//           up to ~4e4 spins): the +-1.0 multiplier of a term is then ONE SDWA instruction (the colour
//           sweep: plus bit 0 of the byte, above);
//   kGlobal: the bit words of kBits kept in HBM (one replica): no LDS limit on the size, every
//           neighbour gather is an L2 access — the slow path for clusters beyond ~1.3e6 spins.
//   kNibbles: four bits per position — two positions share a byte — for M <= 4 replicas: twice the
//           capacity of kBytes (~2.4e5 spins) at four replicas per workgroup instead of kBits'
//           one; a flip is an LDS atomic XOR on the word that holds the nibble.
constexpr int kBytes = 0, kBits = 1, kWide = 2, kGlobal = 3, kNibbles = 6;  // (4, 5: team / shuffled launches, as reported by asp_sa_last_layout)

}  // namespace dev
}  // namespace asp
