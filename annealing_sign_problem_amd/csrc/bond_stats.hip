// Bond statistics of an Ising model on gfx950 (specification ASP-BONDS-1): the
// reference's
//   analyze_probability_of_frustration            common.py:963-1002  (numpy, scipy)
//   analyze_coupling_distribution                 common.py:940-960   (numpy, scipy)
//   cluster_statistics                            common.py:439-478   (Python loops)
// from a CSR matrix that stays resident in a handle, and the device-resident CSR of a whole symmetry
// sector's Ising model from its ELL matrix and ground state (asp_sector_bonds_create).
//
// HBM layout: indptr i64[K+1], indices i32[nnz], data f64[nnz] (columns of a row unique, any order),
// signs u64[ceil(K/64)] (bit i set: s_i = +1); per row strongest f64, strongest_col i32,
// strongest_frustrated u8, row_bonds u32; seven u64 global values and one partial of them per workgroup.
// Kernels: k_bond_rows + k_bond_finish (pass 1, rerun by set_signs) -> k_bond_hist (per histogram call) ->
// k_bond_compact after a scan of row_bonds, then rocprim's descending radix sort of the bit patterns.
// All three map one wavefront to a row, lanes striding over its entries, wavefronts striding over the
// rows; every output is an integer count, an extremum or a sorted copy, so nothing depends on the
// launch geometry or on the order of the atomics.  12 B per stored entry in, read once per pass, plus
// the sign words (K/8 bytes, L2-resident); no MFMA.
// The sector build is count -> scan -> emit with ONE LANE per row: the ELL arrays are slot-major
// ([k * n + i]), so a wavefront reads 64 consecutive rows of a slot in one coalesced access.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "asp_common.hpp"

namespace {

using asp::DeviceBuffer;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned long long kAbsMask = 0x7FFFFFFFFFFFFFFFull;
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;
constexpr uint32_t kMaxBins = 4096;
// a row has at most K entries and a workgroup counts kWaves rows between two looks at its 32-bit LDS
// counters
constexpr uint64_t kMaxSpins = 1ull << 30;

enum Global { G_BONDS, G_FRUSTRATED, G_NONFINITE, G_MAX, G_MIN, G_ROWS, G_STRONGEST_FRUSTRATED, G_COUNT };

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) {
    const unsigned long long other = __shfl_xor(v, step, 64);
    v = other > v ? other : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) {
    const unsigned long long other = __shfl_xor(v, step, 64);
    v = other < v ? other : v;
  }
  return v;
}

// How two partial values of global `which` combine: maximum, minimum or sum.
__device__ __forceinline__ unsigned long long fold(int which, unsigned long long a, unsigned long long b) {
  if (which == G_MAX) return a > b ? a : b;
  if (which == G_MIN) return a < b ? a : b;
  return a + b;
}

__device__ __forceinline__ bool sign_up(const uint64_t *__restrict__ signs, uint32_t i) {
  return (signs[i >> 6] >> (i & 63u)) & 1ull;
}

struct CsrArgs {
  const int64_t *indptr;
  const int32_t *indices;
  const double *data;
  const uint64_t *signs;
  uint64_t num_spins;
};

struct RowOut {
  unsigned long long *partials;  // [workgroups][G_COUNT]
  double *strongest;
  int32_t *strongest_col;
  uint8_t *strongest_frustrated;
  uint32_t *row_bonds;
};

// Pass 1.  The strongest bond of a row is the maximum of the key (bits of |x|, ~column, frustrated):
// columns are unique within a row, so the last part never decides and ties go to the smallest column.
__global__ __launch_bounds__(kThreads) void k_bond_rows(CsrArgs a, RowOut o) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  unsigned long long bonds = 0, frustrated = 0, nonfinite = 0, top = 0, bottom = ~0ull;
  unsigned long long rows = 0, strongest_frustrated = 0;  // lane 0's count
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); row < a.num_spins;
       row += waves) {
    const uint32_t i = static_cast<uint32_t>(row);
    const bool up = sign_up(a.signs, i);
    const int64_t begin = a.indptr[row], end = a.indptr[row + 1];
    unsigned long long here = 0, key_bits = 0, key_rest = 0;
    for (int64_t k = begin + lane; k < end; k += 64) {
      const uint32_t j = static_cast<uint32_t>(a.indices[k]);
      const double x = a.data[k];
      const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x)) & kAbsMask;
      if (b >= kInfBits) {
        ++nonfinite;
        continue;
      }
      if (j == i || b == 0) continue;
      const unsigned long long f = ((up == sign_up(a.signs, j)) == (x > 0.0)) ? 1ull : 0ull;
      ++here;
      frustrated += f;
      top = b > top ? b : top;
      bottom = b < bottom ? b : bottom;
      const unsigned long long rest = (static_cast<unsigned long long>(~j) << 1) | f;
      if (b > key_bits || (b == key_bits && rest > key_rest)) {
        key_bits = b;
        key_rest = rest;
      }
    }
    bonds += here;
    here = wave_sum(here);
    const unsigned long long best = wave_max(key_bits);
    key_rest = wave_max(key_bits == best ? key_rest : 0ull);
    if (lane == 0) {
      o.row_bonds[row] = static_cast<uint32_t>(here);
      o.strongest[row] = __longlong_as_double(static_cast<long long>(best));
      o.strongest_col[row] = best ? static_cast<int32_t>(~static_cast<uint32_t>(key_rest >> 1)) : -1;
      o.strongest_frustrated[row] = best ? static_cast<uint8_t>(key_rest & 1ull) : 0;
      rows += best ? 1ull : 0ull;
      strongest_frustrated += best ? (key_rest & 1ull) : 0ull;
    }
  }
  // one partial per workgroup: no two workgroups write the same address, k_bond_finish folds them
  __shared__ unsigned long long part[kWaves][G_COUNT];
  const uint32_t w = threadIdx.x >> 6;
  bonds = wave_sum(bonds);
  frustrated = wave_sum(frustrated);
  nonfinite = wave_sum(nonfinite);
  top = wave_max(top);
  bottom = wave_min(bottom);
  if (lane == 0) {
    part[w][G_BONDS] = bonds;
    part[w][G_FRUSTRATED] = frustrated;
    part[w][G_NONFINITE] = nonfinite;
    part[w][G_MAX] = top;
    part[w][G_MIN] = bottom;
    part[w][G_ROWS] = rows;
    part[w][G_STRONGEST_FRUSTRATED] = strongest_frustrated;
  }
  __syncthreads();
  if (threadIdx.x < G_COUNT) {
    unsigned long long v = part[0][threadIdx.x];
    for (int k = 1; k < kWaves; ++k) v = fold(threadIdx.x, v, part[k][threadIdx.x]);
    o.partials[static_cast<uint64_t>(blockIdx.x) * G_COUNT + threadIdx.x] = v;
  }
}

// One workgroup: partials[blocks][G_COUNT] -> globals[G_COUNT].
__global__ __launch_bounds__(kThreads) void k_bond_finish(const unsigned long long *__restrict__ partials,
                                                         uint32_t blocks, unsigned long long *__restrict__ globals) {
  __shared__ unsigned long long part[kWaves][G_COUNT];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long v[G_COUNT] = {0, 0, 0, 0, ~0ull, 0, 0};
  for (uint32_t b = threadIdx.x; b < blocks; b += kThreads) {
#pragma unroll
    for (int g = 0; g < G_COUNT; ++g) v[g] = fold(g, v[g], partials[static_cast<uint64_t>(b) * G_COUNT + g]);
  }
#pragma unroll
  for (int g = 0; g < G_COUNT; ++g) {
    v[g] = g == G_MAX ? wave_max(v[g]) : g == G_MIN ? wave_min(v[g]) : wave_sum(v[g]);
    if (lane == 0) part[w][g] = v[g];
  }
  __syncthreads();
  if (threadIdx.x < G_COUNT) {
    unsigned long long r = part[0][threadIdx.x];
    for (int k = 1; k < kWaves; ++k) r = fold(threadIdx.x, r, part[k][threadIdx.x]);
    globals[threadIdx.x] = r;
  }
}

// Histogram of |J| over the bonds.  LDS: edges f64[nb + 1], then counts u32[2 nb] (normal, frustrated).
// counts_out u64[2 nb + 2]: normal, frustrated, below, above.
__global__ __launch_bounds__(kThreads) void k_bond_hist(CsrArgs a, uint32_t nb, const double *__restrict__ edges_in,
                                                       unsigned long long *__restrict__ counts_out) {
  extern __shared__ unsigned char lds_raw[];
  double *edges = reinterpret_cast<double *>(lds_raw);
  uint32_t *counts = reinterpret_cast<uint32_t *>(edges + nb + 1);
  for (uint32_t t = threadIdx.x; t <= nb; t += kThreads) edges[t] = edges_in[t];
  for (uint32_t t = threadIdx.x; t < 2 * nb; t += kThreads) counts[t] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const double first = edges[0], last = edges[nb];
  unsigned long long below = 0, above = 0;
  uint64_t pending = 0;  // entries this workgroup has looked at since its last flush (uniform)
  for (uint64_t row0 = static_cast<uint64_t>(blockIdx.x) * kWaves; row0 < a.num_spins;
       row0 += static_cast<uint64_t>(gridDim.x) * kWaves) {
    const uint64_t row1 = row0 + kWaves < a.num_spins ? row0 + kWaves : a.num_spins;
    const uint64_t entries = static_cast<uint64_t>(a.indptr[row1] - a.indptr[row0]);
    if (pending + entries > 0xFFFFFFFFull) {  // the 32-bit counters could wrap: flush first
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < 2 * nb; t += kThreads) {
        const uint32_t c = counts[t];
        if (c) atomicAdd(&counts_out[t], static_cast<unsigned long long>(c));
        counts[t] = 0;
      }
      __syncthreads();
      pending = 0;
    }
    pending += entries;
    const uint64_t row = row0 + (threadIdx.x >> 6);
    if (row >= a.num_spins) continue;
    const uint32_t i = static_cast<uint32_t>(row);
    const bool up = sign_up(a.signs, i);
    const int64_t begin = a.indptr[row], end = a.indptr[row + 1];
    for (int64_t k = begin + lane; k < end; k += 64) {
      const uint32_t j = static_cast<uint32_t>(a.indices[k]);
      const double x = a.data[k];
      const double m = fabs(x);
      if (j == i || m == 0.0) continue;
      if (m < first) {
        ++below;
        continue;
      }
      if (m > last) {
        ++above;
        continue;
      }
      // number of edges <= m, in [1, nb + 1]
      uint32_t lo = 1, hi = nb + 1;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (edges[mid] <= m) {
          lo = mid + 1;
        } else {
          hi = mid;
        }
      }
      const uint32_t bin = lo > nb ? nb - 1 : lo - 1;  // the last bin is closed on the right
      const bool f = (up == sign_up(a.signs, j)) == (x > 0.0);
      atomicAdd(&counts[(f ? nb : 0u) + bin], 1u);
    }
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < 2 * nb; t += kThreads) {
    const uint32_t c = counts[t];
    if (c) atomicAdd(&counts_out[t], static_cast<unsigned long long>(c));
  }
  below = wave_sum(below);
  above = wave_sum(above);
  if (lane == 0) {
    if (below) atomicAdd(&counts_out[2 * nb], below);
    if (above) atomicAdd(&counts_out[2 * nb + 1], above);
  }
}

// Bit patterns of |J| of the bonds, row after row, at the offsets the scan of row_bonds gave.
__global__ __launch_bounds__(kThreads) void k_bond_compact(CsrArgs a, const int64_t *__restrict__ offsets,
                                                          unsigned long long *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); row < a.num_spins;
       row += waves) {
    const uint32_t i = static_cast<uint32_t>(row);
    const int64_t begin = a.indptr[row], end = a.indptr[row + 1];
    int64_t at = offsets[row];
    for (int64_t base = begin; base < end; base += 64) {
      const int64_t k = base + lane;
      unsigned long long b = 0;
      if (k < end && static_cast<uint32_t>(a.indices[k]) != i) {
        b = static_cast<unsigned long long>(__double_as_longlong(a.data[k])) & kAbsMask;
      }
      const uint64_t votes = __ballot(b != 0);
      if (b != 0) out[at + __popcll(votes & ((1ull << lane) - 1ull))] = b;
      at += __popcll(votes);
    }
  }
}

// s_i = +1 iff psi_i >= 0: one wavefront writes one word (the tail's missing lanes vote 0).
__global__ __launch_bounds__(kThreads) void k_sector_signs(const double *__restrict__ psi, uint64_t n,
                                                          uint64_t *__restrict__ signs) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t votes = __ballot(i < n && psi[i] >= 0.0);
  if ((threadIdx.x & 63u) == 0 && (i >> 6) < (n + 63) / 64) signs[i >> 6] = votes;
}

// The sector's Ising model, row i by one lane.  Candidates are the distinct targets j != i of row i
// in the order of their first slot; H_ij and H_ji are summed in slot order from +0.0.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_sector_csr(uint64_t n, uint32_t width,
                                                        const uint32_t *__restrict__ idx,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ psi,
                                                        uint32_t *__restrict__ row_count,
                                                        const int64_t *__restrict__ indptr,
                                                        int32_t *__restrict__ out_indices,
                                                        double *__restrict__ out_data) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const double mine = fabs(psi[i]);
  const int64_t out = EMIT ? indptr[i] : 0;
  uint32_t count = 0;
  if (mine != 0.0) {  // (an amplitude of 0 makes every product of the row +-0: no entry is kept)
    for (uint32_t k = 0; k < width; ++k) {
      const uint32_t j = idx[static_cast<uint64_t>(k) * n + i];
      if (j == i || j >= n) continue;
      bool seen = false;
      for (uint32_t e = 0; e < k && !seen; ++e) seen = idx[static_cast<uint64_t>(e) * n + i] == j;
      if (seen) continue;
      const double theirs = fabs(psi[j]);
      if (theirs == 0.0) continue;
      double h_ij = 0.0, h_ji = 0.0;
      for (uint32_t e = k; e < width; ++e) {
        if (idx[static_cast<uint64_t>(e) * n + i] == j) h_ij = __dadd_rn(h_ij, val[static_cast<uint64_t>(e) * n + i]);
      }
      for (uint32_t e = 0; e < width; ++e) {
        if (idx[static_cast<uint64_t>(e) * n + j] == i) h_ji = __dadd_rn(h_ji, val[static_cast<uint64_t>(e) * n + j]);
      }
      const double m_ij = __dmul_rn(__dmul_rn(h_ij, theirs), mine);
      const double m_ji = __dmul_rn(__dmul_rn(h_ji, mine), theirs);
      const double coupling = __dmul_rn(0.5, __dadd_rn(m_ij, m_ji));
      if (coupling != 0.0) {
        if (EMIT) {
          out_indices[out + count] = static_cast<int32_t>(j);
          out_data[out + count] = coupling;
        }
        ++count;
      }
    }
  }
  if (!EMIT) row_count[i] = count;
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  return static_cast<unsigned>((items + per_block - 1) / per_block);
}

// Wavefronts stride over the rows: enough workgroups to fill the device, and a number of partials and
// of histogram flushes that does not grow with the matrix (one atomic per wavefront and value, all to
// the same addresses, cost 0.8 ms on 12 870 rows: same-address atomics serialise in L2).
int row_grid(uint64_t num_spins, unsigned *blocks) {
  int cus = 0;
  size_t lds = 0;
  ASP_TRY(asp::device_limits(&cus, &lds));
  const uint64_t want = std::max<uint64_t>(1, (num_spins + kWaves - 1) / kWaves);
  *blocks = static_cast<unsigned>(std::min<uint64_t>(want, static_cast<uint64_t>(std::max(cus, 1)) * 16));
  return ASP_OK;
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

}  // namespace

struct asp_bonds {
  int device = 0;
  uint64_t num_spins = 0, stored = 0;
  DeviceBuffer<int64_t> indptr;
  DeviceBuffer<int32_t> indices;
  DeviceBuffer<double> data;
  DeviceBuffer<uint64_t> signs;
  DeviceBuffer<unsigned long long> globals, partials;
  DeviceBuffer<double> strongest;
  DeviceBuffer<int32_t> strongest_col;
  DeviceBuffer<uint8_t> strongest_frustrated;
  DeviceBuffer<uint32_t> row_bonds;
  asp_bonds_summary summary{};

  CsrArgs csr() const { return CsrArgs{indptr.ptr, indices.ptr, data.ptr, signs.ptr, num_spins}; }
  uint64_t sign_words() const { return (num_spins + 63) / 64; }
};

namespace {

int alloc_row_outputs(asp_bonds *b) {
  const uint64_t K = b->num_spins;
  ASP_TRY(b->signs.alloc(b->sign_words()));
  ASP_TRY(b->globals.alloc(G_COUNT));
  ASP_TRY(b->strongest.alloc(K));
  ASP_TRY(b->strongest_col.alloc(K));
  ASP_TRY(b->strongest_frustrated.alloc(K));
  ASP_TRY(b->row_bonds.alloc(K));
  return ASP_OK;
}

// Pass 1 on the resident matrix and signs; fills b->summary.  The stream is synchronised on return.
int run_rows(asp_bonds *b, hipStream_t stream, Timer &timer) {
  unsigned blocks = 0;
  if (b->num_spins > 0) ASP_TRY(row_grid(b->num_spins, &blocks));
  ASP_TRY(b->partials.ensure(static_cast<size_t>(blocks) * G_COUNT));
  if (b->num_spins > 0) {
    RowOut out{b->partials.ptr, b->strongest.ptr, b->strongest_col.ptr, b->strongest_frustrated.ptr,
               b->row_bonds.ptr};
    hipLaunchKernelGGL(k_bond_rows, dim3(blocks), dim3(kThreads), 0, stream, b->csr(), out);
  }
  // (no workgroups: the identities, with the minimum at all ones)
  hipLaunchKernelGGL(k_bond_finish, dim3(1), dim3(kThreads), 0, stream, b->partials.ptr, blocks, b->globals.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(timer.mark());
  unsigned long long g[G_COUNT];
  ASP_HIP_TRY(hipMemcpyAsync(g, b->globals.ptr, sizeof g, hipMemcpyDeviceToHost, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  timer.read();
  if (g[G_NONFINITE] != 0) {
    return asp::set_error(ASP_ERR_INVALID, "%llu stored couplings are not finite", g[G_NONFINITE]);
  }
  asp_bonds_summary &s = b->summary;
  s.num_spins = b->num_spins;
  s.stored = b->stored;
  s.bonds = g[G_BONDS];
  s.frustrated = g[G_FRUSTRATED];
  s.rows_with_bonds = g[G_ROWS];
  s.strongest_frustrated = g[G_STRONGEST_FRUSTRATED];
  const unsigned long long low = s.bonds ? g[G_MIN] : 0ull;
  std::memcpy(&s.max_abs, &g[G_MAX], sizeof(double));
  std::memcpy(&s.min_abs, &low, sizeof(double));
  return ASP_OK;
}

}  // namespace

extern "C" float asp_bonds_last_ms(void) { return g_last_ms; }

extern "C" void asp_bonds_destroy(asp_bonds *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

extern "C" int asp_bonds_create(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                                double const *data, uint64_t const *sign_words, asp_bonds **out) {
  asp_clear_error();
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output handle");
  *out = nullptr;
  ASP_TRY(asp::require_device());
  const uint64_t K = num_spins;
  if (K >= kMaxSpins) return asp::set_error(ASP_ERR_TOO_LARGE, "2^30 spins or more");
  if (K > 0 && (!indptr || !sign_words)) return asp::set_error(ASP_ERR_INVALID, "null input array");
  uint64_t nnz = 0;
  if (K > 0) {
    if (indptr[0] != 0) return asp::set_error(ASP_ERR_INVALID, "indptr[0] must be 0");
    for (uint64_t i = 0; i < K; ++i) {
      if (indptr[i + 1] < indptr[i]) return asp::set_error(ASP_ERR_INVALID, "indptr is not monotone");
    }
    nnz = static_cast<uint64_t>(indptr[K]);
    if (nnz && (!indices || !data)) return asp::set_error(ASP_ERR_INVALID, "null indices/data");
    for (uint64_t k = 0; k < nnz; ++k) {
      if (indices[k] < 0 || static_cast<uint64_t>(indices[k]) >= K) {
        return asp::set_error(ASP_ERR_INVALID, "column index %d out of range at entry %llu", indices[k],
                              (unsigned long long)k);
      }
    }
  }
  asp_bonds *b = new (std::nothrow) asp_bonds();
  if (!b) return asp::set_error(ASP_ERR_ALLOC, "out of host memory");
  struct Guard {
    asp_bonds *b;
    ~Guard() { delete b; }
  } guard{b};
  ASP_HIP_TRY(hipGetDevice(&b->device));
  b->num_spins = K;
  b->stored = nnz;
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  asp::StreamFence fence(stream);
  ASP_TRY(b->indptr.alloc(K + 1));
  ASP_TRY(b->indices.alloc(nnz));
  ASP_TRY(b->data.alloc(nnz));
  ASP_TRY(alloc_row_outputs(b));
  if (K > 0) {
    ASP_TRY(b->indptr.upload(indptr, K + 1, stream));
    ASP_TRY(b->indices.upload(indices, nnz, stream));
    ASP_TRY(b->data.upload(data, nnz, stream));
    ASP_TRY(b->signs.upload(sign_words, b->sign_words(), stream));
  }
  Timer timer;
  ASP_TRY(timer.start(stream));
  ASP_TRY(run_rows(b, stream, timer));
  guard.b = nullptr;
  *out = b;
  return ASP_OK;
}

extern "C" int asp_bonds_set_signs(asp_bonds *b, uint64_t const *sign_words) {
  asp_clear_error();
  if (!b) return asp::set_error(ASP_ERR_INVALID, "null bonds handle");
  if (b->num_spins > 0 && !sign_words) return asp::set_error(ASP_ERR_INVALID, "null sign words");
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  ASP_TRY(b->signs.upload(sign_words, b->sign_words(), stream));
  Timer timer;
  ASP_TRY(timer.start(stream));
  return run_rows(b, stream, timer);
}

extern "C" int asp_bonds_get_summary(asp_bonds const *b, asp_bonds_summary *out) {
  asp_clear_error();
  if (!b || !out) return asp::set_error(ASP_ERR_INVALID, "null bonds handle or summary");
  *out = b->summary;
  return ASP_OK;
}

extern "C" int asp_bonds_rows(asp_bonds const *b, double *strongest, int32_t *strongest_col,
                              uint8_t *strongest_frustrated) {
  asp_clear_error();
  if (!b) return asp::set_error(ASP_ERR_INVALID, "null bonds handle");
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  const uint64_t K = b->num_spins;
  if (strongest) ASP_TRY(b->strongest.download(strongest, K, stream));
  if (strongest_col) ASP_TRY(b->strongest_col.download(strongest_col, K, stream));
  if (strongest_frustrated) ASP_TRY(b->strongest_frustrated.download(strongest_frustrated, K, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  return ASP_OK;
}

extern "C" int asp_bonds_histogram(asp_bonds const *b, uint32_t num_bins, double const *edges,
                                   uint64_t *normal, uint64_t *frustrated, uint64_t *below,
                                   uint64_t *above) {
  asp_clear_error();
  if (!b) return asp::set_error(ASP_ERR_INVALID, "null bonds handle");
  if (num_bins < 1 || num_bins > kMaxBins) {
    return asp::set_error(ASP_ERR_INVALID, "%u bins: 1 to %u are supported", num_bins, kMaxBins);
  }
  if (!edges || !normal || !frustrated) return asp::set_error(ASP_ERR_INVALID, "null edges or counts");
  const uint32_t nb = num_bins;
  for (uint32_t k = 0; k <= nb; ++k) {
    if (!std::isfinite(edges[k]) || (k > 0 && !(edges[k - 1] < edges[k]))) {
      return asp::set_error(ASP_ERR_INVALID, "edges must be finite and strictly ascending (edge %u)", k);
    }
  }
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  DeviceBuffer<double> d_edges;
  DeviceBuffer<unsigned long long> d_counts;
  asp::StreamFence fence(stream);
  const size_t values = 2 * static_cast<size_t>(nb) + 2;
  ASP_TRY(d_edges.alloc(nb + 1));
  ASP_TRY(d_counts.alloc(values));
  ASP_TRY(d_edges.upload(edges, nb + 1, stream));
  Timer timer;
  ASP_TRY(timer.start(stream));
  ASP_HIP_TRY(hipMemsetAsync(d_counts.ptr, 0, values * sizeof(unsigned long long), stream));
  if (b->num_spins > 0) {
    const size_t lds = (nb + 1) * sizeof(double) + 2 * static_cast<size_t>(nb) * sizeof(uint32_t);
    ASP_TRY(asp::allow_dynamic_lds(reinterpret_cast<const void *>(k_bond_hist), lds));
    unsigned blocks = 1;
    ASP_TRY(row_grid(b->num_spins, &blocks));
    hipLaunchKernelGGL(k_bond_hist, dim3(blocks), dim3(kThreads), lds, stream, b->csr(), nb, d_edges.ptr,
                       d_counts.ptr);
    ASP_HIP_TRY(hipGetLastError());
  }
  ASP_TRY(timer.mark());
  std::vector<unsigned long long> host(values);
  ASP_TRY(d_counts.download(host.data(), values, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  timer.read();
  for (uint32_t k = 0; k < nb; ++k) {
    normal[k] = host[k];
    frustrated[k] = host[nb + k];
  }
  if (below) *below = host[2 * nb];
  if (above) *above = host[2 * nb + 1];
  return ASP_OK;
}

extern "C" int asp_bonds_magnitudes(asp_bonds const *b, uint64_t capacity, double *out) {
  asp_clear_error();
  if (!b) return asp::set_error(ASP_ERR_INVALID, "null bonds handle");
  const uint64_t bonds = b->summary.bonds;
  if (capacity < bonds || (bonds && !out)) {
    return asp::set_error(ASP_ERR_INVALID, "%llu bonds do not fit capacity %llu", (unsigned long long)bonds,
                          (unsigned long long)capacity);
  }
  if (bonds == 0) return ASP_OK;
  ASP_TRY(asp::bind_device());
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  DeviceBuffer<int64_t> d_offsets, d_scratch;
  DeviceBuffer<unsigned long long> d_keys, d_sorted;
  DeviceBuffer<unsigned char> d_temp;
  asp::StreamFence fence(stream);
  const uint64_t K = b->num_spins;
  ASP_TRY(d_offsets.alloc(K + 1));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(K)));
  ASP_TRY(d_keys.alloc(bonds));
  ASP_TRY(d_sorted.alloc(bonds));
  size_t temp_bytes = 0;
  // the sign bit is clear in every key: 63 significant bits
  ASP_HIP_TRY(rocprim::radix_sort_keys_desc(nullptr, temp_bytes, d_keys.ptr, d_sorted.ptr, bonds, 0, 63, stream));
  ASP_TRY(d_temp.alloc(temp_bytes));
  Timer timer;
  ASP_TRY(timer.start(stream));
  ASP_TRY(asp::exclusive_scan_u32(b->row_bonds.ptr, K, d_offsets.ptr, d_scratch.ptr, stream));
  unsigned blocks = 1;
  ASP_TRY(row_grid(K, &blocks));
  hipLaunchKernelGGL(k_bond_compact, dim3(blocks), dim3(kThreads), 0, stream, b->csr(), d_offsets.ptr, d_keys.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(rocprim::radix_sort_keys_desc(d_temp.ptr, temp_bytes, d_keys.ptr, d_sorted.ptr, bonds, 0, 63, stream));
  ASP_TRY(timer.mark());
  ASP_HIP_TRY(hipMemcpyAsync(out, d_sorted.ptr, bonds * sizeof(double), hipMemcpyDeviceToHost, stream));
  ASP_HIP_TRY(hipStreamSynchronize(stream));
  timer.read();
  return ASP_OK;
}

extern "C" int asp_sector_bonds_create(uint64_t n, uint32_t width, uint32_t const *idx_dev,
                                       double const *val_dev, double const *psi_dev, asp_bonds **out) {
  asp_clear_error();
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output handle");
  *out = nullptr;
  ASP_TRY(asp::require_device());
  if (n >= kMaxSpins) return asp::set_error(ASP_ERR_TOO_LARGE, "2^30 states or more");
  if (n > 0 && (!psi_dev || (width > 0 && (!idx_dev || !val_dev)))) {
    return asp::set_error(ASP_ERR_INVALID, "null device array");
  }
  asp_bonds *b = new (std::nothrow) asp_bonds();
  if (!b) return asp::set_error(ASP_ERR_ALLOC, "out of host memory");
  struct Guard {
    asp_bonds *b;
    ~Guard() { delete b; }
  } guard{b};
  ASP_HIP_TRY(hipGetDevice(&b->device));
  b->num_spins = n;
  asp::ScopedStream scoped;
  ASP_TRY(scoped.acquire());
  hipStream_t stream = scoped.stream;
  DeviceBuffer<int64_t> d_scratch;
  asp::StreamFence fence(stream);
  ASP_TRY(b->indptr.alloc(n + 1));
  ASP_TRY(alloc_row_outputs(b));
  ASP_TRY(d_scratch.alloc(asp::scan_scratch_elems(n)));
  Timer timer;
  ASP_TRY(timer.start(stream));
  int64_t nnz = 0;
  if (n > 0) {
    const unsigned blocks = grid_for(n, kThreads);
    hipLaunchKernelGGL(k_sector_signs, dim3(blocks), dim3(kThreads), 0, stream, psi_dev, n, b->signs.ptr);
    // (row_bonds is free until pass 1 runs: it holds the rows' entry counts meanwhile)
    hipLaunchKernelGGL(k_sector_csr<false>, dim3(blocks), dim3(kThreads), 0, stream, n, width, idx_dev, val_dev,
                       psi_dev, b->row_bonds.ptr, nullptr, nullptr, nullptr);
    ASP_HIP_TRY(hipGetLastError());
    ASP_TRY(asp::exclusive_scan_u32(b->row_bonds.ptr, n, b->indptr.ptr, d_scratch.ptr, stream));
    ASP_HIP_TRY(hipMemcpyAsync(&nnz, b->indptr.ptr + n, sizeof nnz, hipMemcpyDeviceToHost, stream));
    ASP_HIP_TRY(hipStreamSynchronize(stream));
    b->stored = static_cast<uint64_t>(nnz);
    ASP_TRY(b->indices.alloc(b->stored));
    ASP_TRY(b->data.alloc(b->stored));
    hipLaunchKernelGGL(k_sector_csr<true>, dim3(blocks), dim3(kThreads), 0, stream, n, width, idx_dev, val_dev,
                       psi_dev, nullptr, b->indptr.ptr, b->indices.ptr, b->data.ptr);
    ASP_HIP_TRY(hipGetLastError());
  } else {
    ASP_TRY(b->indices.alloc(0));
    ASP_TRY(b->data.alloc(0));
  }
  ASP_TRY(run_rows(b, stream, timer));  // (one timer: build and pass 1)
  guard.b = nullptr;
  *out = b;
  return ASP_OK;
}
