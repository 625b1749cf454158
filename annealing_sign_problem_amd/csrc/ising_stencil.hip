// Coupling stencil (ASP-STENCIL-1; include/asp.h): the couplings of a fixed set of
// states from new amplitudes alone.  All matrix elements H_ij among the keys are found once
// (asp_ising_stencil_create: the action, the key search and the grouping by target, on the host from the
// downloaded connection list) and stay on the device; a draw is then K doubles up, one fold per
// (row, target) group in connection order and one 0.5 * (a + b) per stored entry — the arithmetic of both
// paths of csrc/operator_apply.hip (pair_coupling / k_ising_rows and k_merge_rows / k_sym_rows) without
// the operator pass, the hash lookups and the per-row sort.  asp_sa_plan_reweight_stencil_batch hands the
// values of a round of draws to the steps of csrc/sa_reweight.hip without a visit to the host.  gfx950 only.
//
// The kernels are gather-and-fold over a few MB: one thread per group (k_st_fold) and per stored or silent
// pair (k_st_pairs), grid-stride, the draw in blockIdx.y; no workgroup depends on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "asp_common.hpp"
#include "operator_internal.hpp"
#include "sa_internal.hpp"
#include "sa_reweight.hpp"

struct asp_ising_stencil {
  uint64_t K = 0, nnz = 0, connections = 0, groups = 0, silent = 0, longest = 0, diagonals = 0;
  std::vector<int64_t> indptr;   // the pattern, to compare a plan's with
  std::vector<int32_t> indices;
  // plans' patterns that were compared with this one and are equal (kept alive: the address is the key)
  std::vector<std::shared_ptr<asp::SaPattern>> verified;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  // resident: groups g (row, target, connections [g_ptr[g], g_ptr[g + 1]) in connection order) and the
  // pairs t — t < nnz: stored entry t, then the silent pairs — with their forward and mirror group
  asp::DeviceBuffer<uint32_t> g_ptr, pair_fwd, pair_mir, diag_rank;
  asp::DeviceBuffer<int32_t> g_row, g_col;
  asp::DeviceBuffer<double> coeff;
  // per call, grown on demand and kept
  asp::DeviceBuffer<double> b_psi, b_gsum, b_data, b_diag, b_field, b_staged, b_row_sum, b_row_min;
  asp::DeviceBuffer<uint32_t> b_changed, b_zeros;
  // the host side of a batched reweight, kept as well (a round's arrays are tens of MB: allocating them
  // anew for every call costs more than the kernels); spare[d] receives draw d's merged values and is
  // swapped with the plan's on commit, so the two buffers alternate
  std::vector<double> h_psi, h_field, h_row_sum, h_row_min, h_diag, h_data;
  std::vector<uint32_t> h_changed, h_zeros;
  std::vector<std::vector<double>> spare;
  ~asp_ising_stencil() {
    for (hipEvent_t e : ev) {
      if (e) (void)hipEventDestroy(e);
    }
    if (stream) {
      (void)hipStreamSynchronize(stream);
      asp::stream_release(stream);
    }
  }
};

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kThreads = 256;

thread_local float g_batch_ms = 0.0f;

// gsum[d][g] = ((+0.0 + e_1) + e_2) + ...,  e = (c * |psi_col|) * |psi_row|, every operation rounded.
__global__ __launch_bounds__(kThreads) void k_st_fold(const double *__restrict__ psi, uint64_t K, uint32_t count,
                                                      const uint32_t *__restrict__ g_ptr,
                                                      const int32_t *__restrict__ g_row,
                                                      const int32_t *__restrict__ g_col,
                                                      const double *__restrict__ coeff, uint64_t groups,
                                                      double *__restrict__ gsum) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint32_t d = blockIdx.y; d < count; d += gridDim.y) {
    const double *p = psi + static_cast<uint64_t>(d) * K;
    double *out = gsum + static_cast<uint64_t>(d) * groups;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < groups; g += stride) {
      const double psi_i = fabs(p[g_row[g]]), psi_j = fabs(p[g_col[g]]);
      double sum = 0.0;
      for (uint32_t c = g_ptr[g]; c < g_ptr[g + 1]; ++c) {
        sum = __dadd_rn(sum, __dmul_rn(__dmul_rn(coeff[c], psi_j), psi_i));
      }
      out[g] = sum;
    }
  }
}

// Pair t of draw d: Mhat_ij + Mhat_ji (an absent side +0.0).  A stored pair writes 0.5 * sum in pattern
// order (and the diagonal entries once more, compacted in row order) and counts a sum of exactly 0 in
// changed[d][0]; a silent pair counts a non-zero sum in changed[d][1].
__global__ __launch_bounds__(kThreads) void k_st_pairs(const double *__restrict__ gsum, uint64_t groups,
                                                       uint32_t count, const uint32_t *__restrict__ pair_fwd,
                                                       const uint32_t *__restrict__ pair_mir,
                                                       const uint32_t *__restrict__ diag_rank, uint64_t nnz,
                                                       uint64_t pairs, uint64_t diagonals,
                                                       double *__restrict__ data, double *__restrict__ diag,
                                                       uint32_t *changed) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint32_t d = blockIdx.y; d < count; d += gridDim.y) {
    const double *gs = gsum + static_cast<uint64_t>(d) * groups;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; t < pairs; t += stride) {
      const uint32_t f = pair_fwd[t], m = pair_mir[t];
      const double a = f != kNone ? gs[f] : 0.0;
      const double b = m != kNone ? gs[m] : 0.0;
      const double sum = __dadd_rn(a, b);
      if (t < nnz) {
        const double v = __dmul_rn(0.5, sum);
        data[static_cast<uint64_t>(d) * nnz + t] = v;
        const uint32_t r = diag_rank[t];
        if (r != kNone) diag[static_cast<uint64_t>(d) * diagonals + r] = v;
        if (sum == 0.0) atomicAdd(&changed[2u * d], 1u);
      } else if (sum != 0.0) {
        atomicAdd(&changed[2u * d + 1u], 1u);
      }
    }
  }
}

// (the kernels stride over their items and draws by the grid: the caps lose none)
dim3 grid_for(uint64_t items, uint32_t count) {
  const unsigned x = static_cast<unsigned>(std::min<uint64_t>((items + kThreads - 1) / kThreads, 1u << 16));
  return dim3(std::max(x, 1u), std::min(count, 1024u));
}

int check_amplitudes(uint64_t K, uint32_t d, const double *psi) {
  for (uint64_t i = 0; i < K; ++i) {
    if (!std::isfinite(psi[i])) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: non-finite amplitude at %llu", d, (unsigned long long)i);
    }
  }
  return ASP_OK;
}

// Everything of `count` draws whose amplitudes are in st->b_psi: data, diagonal entries, counts.
int queue_values(asp_ising_stencil *st, uint32_t count) {
  hipStream_t s = st->stream;
  ASP_TRY(st->b_gsum.ensure(static_cast<size_t>(count) * st->groups));
  ASP_TRY(st->b_data.ensure(static_cast<size_t>(count) * st->nnz));
  ASP_TRY(st->b_diag.ensure(static_cast<size_t>(count) * st->diagonals));
  ASP_TRY(st->b_changed.ensure(2 * static_cast<size_t>(count)));
  ASP_HIP_TRY(hipMemsetAsync(st->b_changed.ptr, 0, 2 * static_cast<size_t>(count) * sizeof(uint32_t), s));
  if (st->groups > 0) {
    hipLaunchKernelGGL(k_st_fold, grid_for(st->groups, count), dim3(kThreads), 0, s, st->b_psi.ptr, st->K, count,
                       st->g_ptr.ptr, st->g_row.ptr, st->g_col.ptr, st->coeff.ptr, st->groups, st->b_gsum.ptr);
  }
  const uint64_t pairs = st->nnz + st->silent;
  if (pairs > 0) {
    hipLaunchKernelGGL(k_st_pairs, grid_for(pairs, count), dim3(kThreads), 0, s, st->b_gsum.ptr, st->groups, count,
                       st->pair_fwd.ptr, st->pair_mir.ptr, st->diag_rank.ptr, st->nnz, pairs, st->diagonals,
                       st->b_data.ptr, st->b_diag.ptr, st->b_changed.ptr);
  }
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

bool same_pattern(const asp_ising_stencil *st, const asp::SaPattern &P) {
  return P.nnz == st->nnz && P.indptr == st->indptr && P.indices == st->indices;
}

}  // namespace

extern "C" {

int asp_ising_stencil_create(asp_operator const *op, uint64_t num_spins, uint64_t const *keys,
                             int64_t const *indptr, int32_t const *indices, asp_ising_stencil **out) {
  asp_clear_error();
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output pointer");
  *out = nullptr;
  if (!op) return asp::set_error(ASP_ERR_INVALID, "null operator");
  const uint64_t K = num_spins;
  if (K && !keys) return asp::set_error(ASP_ERR_INVALID, "null keys");
  if (!indptr) return asp::set_error(ASP_ERR_INVALID, "null indptr");
  if (K >= 0x7FFFFFFFull) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^31-1 spins");
  for (uint64_t i = 1; i < K; ++i) {
    if (keys[i - 1] >= keys[i]) return asp::set_error(ASP_ERR_INVALID, "keys are not sorted and unique");
  }
  if (indptr[0] != 0) return asp::set_error(ASP_ERR_INVALID, "pattern is not canonical: indptr[0] != 0");
  for (uint64_t i = 0; i < K; ++i) {
    if (indptr[i + 1] < indptr[i] || indptr[i + 1] - indptr[i] > static_cast<int64_t>(K)) {
      return asp::set_error(ASP_ERR_INVALID, "pattern is not canonical: indptr[%llu]", (unsigned long long)(i + 1));
    }
  }
  const uint64_t nnz = static_cast<uint64_t>(indptr[K]);
  if (nnz && !indices) return asp::set_error(ASP_ERR_INVALID, "null indices");
  for (uint64_t i = 0; i < K; ++i) {
    for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) {
      if (indices[k] < 0 || static_cast<uint64_t>(indices[k]) >= K || (k > indptr[i] && indices[k - 1] >= indices[k])) {
        return asp::set_error(ASP_ERR_INVALID, "pattern is not canonical: columns of row %llu",
                              (unsigned long long)i);
      }
    }
  }
  std::unique_ptr<asp_ising_stencil> st(new (std::nothrow) asp_ising_stencil());
  if (!st) return asp::set_error(ASP_ERR_ALLOC, "out of host memory");
  st->K = K;
  st->nnz = nnz;
  st->indptr.assign(indptr, indptr + K + 1);
  st->indices.assign(indices, indices + nnz);
  if (K == 0) {  // no states: no device
    *out = st.release();
    return ASP_OK;
  }
  ASP_TRY(asp::bind_device());
  ASP_TRY(asp::stream_acquire(&st->stream));
  hipStream_t s = st->stream;
  for (hipEvent_t &e : st->ev) ASP_HIP_TRY(hipEventCreate(&e));
  // ---- the action, once; the connection list comes to the host ----
  std::vector<int64_t> offsets(K + 1);
  std::vector<uint64_t> other;
  std::vector<double> coeffs;
  {
    asp::ConnectionList list;
    asp::StreamFence fence(s);
    ASP_TRY(asp::connection_list(op, K, keys, &list, s));  // (ASP_ERR_INVALID: a key outside the sector)
    other.resize(list.batch.total);
    coeffs.resize(list.batch.total);
    ASP_TRY(list.batch.d_offsets.download(offsets.data(), K + 1, s));
    ASP_TRY(list.d_other.download(other.data(), other.size(), s));
    ASP_TRY(list.d_coeffs.download(coeffs.data(), coeffs.size(), s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
  }
  // ---- groups: per row the in-cluster connections by target, connection order kept ----
  std::vector<uint32_t> g_ptr{0}, row_groups(K + 1, 0);
  std::vector<int32_t> g_row, g_col;
  std::vector<double> coeff;
  std::vector<std::pair<int32_t, int64_t>> hits;  // (target, connection)
  for (uint64_t i = 0; i < K; ++i) {
    hits.clear();
    for (int64_t c = offsets[i]; c < offsets[i + 1]; ++c) {
      const uint64_t *at = std::lower_bound(keys, keys + K, other[c]);
      if (at != keys + K && *at == other[c]) hits.emplace_back(static_cast<int32_t>(at - keys), c);
    }
    std::sort(hits.begin(), hits.end());  // (connections ascend inside a target)
    for (size_t h = 0; h < hits.size(); ++h) {
      if (h == 0 || hits[h].first != hits[h - 1].first) {
        if (h != 0) g_ptr.push_back(static_cast<uint32_t>(coeff.size()));
        g_row.push_back(static_cast<int32_t>(i));
        g_col.push_back(hits[h].first);
      }
      coeff.push_back(coeffs[hits[h].second]);
    }
    if (!hits.empty()) g_ptr.push_back(static_cast<uint32_t>(coeff.size()));
    if (coeff.size() >= kNone) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 2 connections");
    row_groups[i + 1] = static_cast<uint32_t>(g_row.size());
  }
  const uint64_t groups = g_row.size();
  st->groups = groups;
  st->connections = coeff.size();
  for (uint64_t g = 0; g < groups; ++g) st->longest = std::max<uint64_t>(st->longest, g_ptr[g + 1] - g_ptr[g]);
  auto group_of = [&](uint64_t i, int32_t j) -> uint32_t {
    const int32_t *begin = g_col.data() + row_groups[i], *end = g_col.data() + row_groups[i + 1];
    const int32_t *at = std::lower_bound(begin, end, j);
    return at != end && *at == j ? static_cast<uint32_t>(at - g_col.data()) : kNone;
  };
  auto stored = [&](uint64_t i, int32_t j) -> bool {
    return std::binary_search(indices + indptr[i], indices + indptr[i + 1], j);
  };
  const bool duplicates = asp_operator_unique_targets(op) == 0;
  if (duplicates) {  // k_sym_rows: every element of Mhat needs its mirror element
    uint64_t missing = 0;
    for (uint64_t g = 0; g < groups; ++g) {
      if (group_of(static_cast<uint64_t>(g_col[g]), g_row[g]) == kNone) ++missing;
    }
    if (missing != 0) {
      return asp::set_error(ASP_ERR_INVALID,
                            "%llu couplings have no mirror element (one-directional matrix elements): "
                            "use the host route", (unsigned long long)missing);
    }
  }
  // ---- pairs: the stored entries, then the silent pairs ----
  std::vector<uint32_t> pair_fwd(nnz), pair_mir(nnz), diag_rank(nnz, kNone);
  for (uint64_t i = 0; i < K; ++i) {
    for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) {
      const int32_t j = indices[k];
      pair_fwd[k] = group_of(i, j);
      pair_mir[k] = group_of(static_cast<uint64_t>(j), static_cast<int32_t>(i));
      if (pair_fwd[k] == kNone && pair_mir[k] == kNone) {
        return asp::set_error(ASP_ERR_INVALID, "pattern entry (%llu, %d) is produced by no connection",
                              (unsigned long long)i, j);
      }
      if (!stored(static_cast<uint64_t>(j), static_cast<int32_t>(i))) {
        return asp::set_error(ASP_ERR_INVALID, "pattern holds (%llu, %d) without its mirror entry",
                              (unsigned long long)i, j);
      }
      if (static_cast<uint64_t>(j) == i) diag_rank[k] = static_cast<uint32_t>(st->diagonals++);
    }
  }
  for (uint64_t g = 0; g < groups; ++g) {
    const uint64_t i = static_cast<uint64_t>(g_row[g]);
    const int32_t j = g_col[g];
    if (stored(i, j)) continue;
    const uint32_t mirror = group_of(static_cast<uint64_t>(j), static_cast<int32_t>(i));
    if (static_cast<uint64_t>(j) < i && mirror != kNone) continue;  // listed from the other side
    pair_fwd.push_back(static_cast<uint32_t>(g));
    pair_mir.push_back(mirror);
  }
  st->silent = pair_fwd.size() - nnz;
  if (pair_fwd.size() >= kNone) return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 2 pairs");
  {
    asp::StreamFence fence(s);
    ASP_TRY(asp::upload_vector(st->g_ptr, g_ptr, s));
    ASP_TRY(asp::upload_vector(st->g_row, g_row, s));
    ASP_TRY(asp::upload_vector(st->g_col, g_col, s));
    ASP_TRY(asp::upload_vector(st->coeff, coeff, s));
    ASP_TRY(asp::upload_vector(st->pair_fwd, pair_fwd, s));
    ASP_TRY(asp::upload_vector(st->pair_mir, pair_mir, s));
    ASP_TRY(asp::upload_vector(st->diag_rank, diag_rank, s));
    ASP_HIP_TRY(hipStreamSynchronize(s));
  }
  *out = st.release();
  return ASP_OK;
}

void asp_ising_stencil_destroy(asp_ising_stencil *st) {
  if (!st) return;
  if (st->stream) (void)asp::bind_device();
  delete st;
}

int asp_ising_stencil_info(asp_ising_stencil const *st, asp_ising_stencil_counts *out) {
  asp_clear_error();
  if (!st) return asp::set_error(ASP_ERR_INVALID, "null stencil");
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output pointer");
  out->num_spins = st->K;
  out->stored = st->nnz;
  out->connections = st->connections;
  out->groups = st->groups;
  out->silent_pairs = st->silent;
  out->longest_group = st->longest;
  return ASP_OK;
}

int asp_ising_stencil_values(asp_ising_stencil *st, uint32_t count, double const *psi, double *data,
                             int32_t *status) {
  asp_clear_error();
  if (!st) return asp::set_error(ASP_ERR_INVALID, "null stencil");
  if (count == 0) return ASP_OK;
  if (!status) return asp::set_error(ASP_ERR_INVALID, "null status");
  const uint64_t K = st->K, nnz = st->nnz;
  if (K == 0) {
    std::fill(status, status + count, 0);
    return ASP_OK;
  }
  if (!psi || (nnz && !data)) return asp::set_error(ASP_ERR_INVALID, "null psi or data");
  for (uint32_t d = 0; d < count; ++d) ASP_TRY(check_amplitudes(K, d, psi + static_cast<uint64_t>(d) * K));
  ASP_TRY(asp::bind_device());
  hipStream_t s = st->stream;
  std::vector<uint32_t> changed(2 * static_cast<size_t>(count));
  asp::StreamFence fence(s);
  ASP_TRY(st->b_psi.ensure(static_cast<size_t>(count) * K));
  ASP_TRY(st->b_psi.upload(psi, static_cast<size_t>(count) * K, s));
  ASP_TRY(queue_values(st, count));
  // the values of all draws in one copy, the 2 * count counters in a second; one synchronisation
  ASP_TRY(st->b_data.download(data, static_cast<size_t>(count) * nnz, s));
  ASP_TRY(st->b_changed.download(changed.data(), changed.size(), s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t d = 0; d < count; ++d) status[d] = (changed[2 * d] | changed[2 * d + 1]) != 0 ? 1 : 0;
  return ASP_OK;
}

int asp_sa_plan_reweight_stencil_batch(asp_ising_stencil *st, asp_sa_stencil_item *items, uint32_t count) {
  asp_clear_error();
  if (!st) return asp::set_error(ASP_ERR_INVALID, "null stencil");
  if (count == 0) return ASP_OK;
  if (!items) return asp::set_error(ASP_ERR_INVALID, "null items");
  const uint64_t K = st->K, nnz = st->nnz;
  // ---- everything that can be refused, before anything of a plan is touched ----
  for (uint32_t d = 0; d < count; ++d) {
    const asp_sa_stencil_item &it = items[d];
    if (!it.plan) return asp::set_error(ASP_ERR_INVALID, "item %u: null plan", d);
    if (K && !it.psi) return asp::set_error(ASP_ERR_INVALID, "item %u: null psi", d);
    for (uint32_t o = 0; o < d; ++o) {
      if (items[o].plan == it.plan) {
        return asp::set_error(ASP_ERR_INVALID, "item %u: the plan of item %u again", d, o);
      }
    }
  }
  for (uint32_t d = 0; d < count; ++d) {
    const asp_sa_stencil_item &it = items[d];
    const std::shared_ptr<asp::SaPattern> &P = it.plan->pattern;
    bool known = false;
    for (const auto &v : st->verified) known = known || v.get() == P.get();
    if (!known) {
      if (it.plan->host.num_spins != K || !same_pattern(st, *P)) {
        return asp::set_error(ASP_ERR_INVALID,
                              "item %u: pattern mismatch: the plan was not created from the stencil's pattern", d);
      }
      st->verified.push_back(P);
    }
    const int live = it.plan->live_chains->load(std::memory_order_relaxed);
    if (live > 0) {
      return asp::set_error(ASP_ERR_INVALID,
                            "item %u: the plan has %d live chains handle(s): their tracked energies belong to "
                            "the old couplings", d, live);
    }
    ASP_TRY(check_amplitudes(K, d, it.psi));
    for (uint64_t i = 0; it.field && i < K; ++i) {
      if (!std::isfinite(it.field[i])) {
        return asp::set_error(ASP_ERR_INVALID, "item %u: non-finite field at %llu", d, (unsigned long long)i);
      }
    }
  }
  for (uint32_t d = 0; d < count; ++d) items[d].status = 0;
  if (K == 0) return ASP_OK;
  ASP_TRY(asp::bind_device());
  bool any_dropped = false;
  for (uint32_t d = 0; d < count; ++d) {
    ASP_TRY(asp::rw_ensure_maps(items[d].plan));
    any_dropped = any_dropped || !items[d].plan->pattern->dropped.empty();
  }
  const uint64_t entries = items[0].plan->host.a_col.size();  // (the pattern decides the layout: equal for all)
  for (uint32_t d = 0; d < count; ++d) {
    if (items[d].plan->host.a_col.size() != entries) {
      return asp::set_error(ASP_ERR_INVALID, "item %u: pattern mismatch: %llu couplings in the plan, item 0 has %llu",
                            d, (unsigned long long)items[d].plan->host.a_col.size(), (unsigned long long)entries);
    }
  }
  const size_t n = count;
  std::vector<double> &psi = st->h_psi, &field_now = st->h_field, &row_sum = st->h_row_sum, &row_min = st->h_row_min,
                      &diag = st->h_diag, &data_host = st->h_data;
  std::vector<uint32_t> &changed = st->h_changed, &zeros = st->h_zeros;
  for (std::vector<double> *v : {&psi, &field_now, &row_sum, &row_min}) v->resize(n * K);
  diag.resize(n * st->diagonals);
  changed.resize(2 * n);
  zeros.resize(n);
  if (st->spare.size() < n) st->spare.resize(n);
  for (uint32_t d = 0; d < count; ++d) st->spare[d].resize(entries);
  for (uint32_t d = 0; d < count; ++d) {
    const asp_sa_stencil_item &it = items[d];
    std::copy(it.psi, it.psi + K, psi.begin() + static_cast<size_t>(d) * K);
    double *f = field_now.data() + static_cast<size_t>(d) * K;
    if (it.field) {
      std::copy(it.field, it.field + K, f);
    } else {
      const asp::SaHostLayout &L = it.plan->host;
      for (uint64_t i = 0; i < K; ++i) f[i] = L.field_pos[L.pos_of_spin[i]];
    }
  }
  hipStream_t s = st->stream;
  asp::StreamFence fence(s);  // (no exit leaves a copy from or into the vectors above in flight)
  ASP_TRY(st->b_psi.ensure(n * K));
  ASP_TRY(st->b_field.ensure(n * K));
  ASP_TRY(st->b_staged.ensure(n * entries));
  ASP_TRY(st->b_row_sum.ensure(n * K));
  ASP_TRY(st->b_row_min.ensure(n * K));
  ASP_TRY(st->b_zeros.ensure(n));
  ASP_HIP_TRY(hipEventRecord(st->ev[0], s));
  ASP_TRY(st->b_psi.upload(psi.data(), n * K, s));
  ASP_TRY(st->b_field.upload(field_now.data(), n * K, s));
  ASP_TRY(queue_values(st, count));
  for (uint32_t d = 0; d < count; ++d) {
    double *d_staged = st->b_staged.ptr + static_cast<size_t>(d) * entries;
    ASP_TRY(asp::rw_queue_merge(items[d].plan, st->b_data.ptr + static_cast<size_t>(d) * nnz, d_staged,
                                st->b_zeros.ptr + d, s));
    ASP_TRY(asp::rw_queue_row_stats(items[d].plan, d_staged, st->b_row_sum.ptr + static_cast<size_t>(d) * K,
                                    st->b_row_min.ptr + static_cast<size_t>(d) * K, s));
  }
  ASP_TRY(st->b_changed.download(changed.data(), 2 * n, s));
  ASP_TRY(st->b_zeros.download(zeros.data(), n, s));
  for (uint32_t d = 0; d < count; ++d) {
    if (entries > 0) {
      ASP_HIP_TRY(hipMemcpyAsync(st->spare[d].data(), st->b_staged.ptr + static_cast<size_t>(d) * entries,
                                 entries * sizeof(double), hipMemcpyDeviceToHost, s));
    }
  }
  ASP_TRY(st->b_row_sum.download(row_sum.data(), n * K, s));
  ASP_TRY(st->b_row_min.download(row_min.data(), n * K, s));
  ASP_TRY(st->b_diag.download(diag.data(), n * st->diagonals, s));
  if (any_dropped) {  // (pairs of J that A does not hold: asp_sa_plan_reweight checks them on the host)
    data_host.resize(n * nnz);
    ASP_TRY(st->b_data.download(data_host.data(), n * nnz, s));
  }
  ASP_HIP_TRY(hipStreamSynchronize(s));
  // ---- per draw: applied or pattern changed; an overflow refuses the whole call ----
  std::vector<asp::RwScales> scales(n);
  std::vector<double> diag_sum(n, 0.0);
  for (uint32_t d = 0; d < count; ++d) {
    asp_sa_stencil_item &it = items[d];
    bool moved = changed[2 * d] != 0 || changed[2 * d + 1] != 0 || zeros[d] != 0;
    if (!moved && any_dropped) {
      const double *data = data_host.data() + static_cast<size_t>(d) * nnz;
      for (const auto &pair : it.plan->pattern->dropped) {
        moved = moved || data[pair.first] + (pair.second >= 0 ? data[pair.second] : 0.0) != 0.0;
      }
    }
    if (moved) {
      it.status = 1;
      continue;
    }
    bool finite = asp::rw_fold_scales(K, row_sum.data() + static_cast<size_t>(d) * K,
                                      row_min.data() + static_cast<size_t>(d) * K,
                                      field_now.data() + static_cast<size_t>(d) * K, &scales[d]);
    const double *dv = diag.data() + static_cast<size_t>(d) * st->diagonals;
    double sum = 0.0;  // D in row order (diag_rank ascends with the row)
    for (uint64_t r = 0; r < st->diagonals; ++r) {
      finite = finite && std::isfinite(dv[r]);
      sum = sum + dv[r];
    }
    diag_sum[d] = sum;
    if (!finite) {
      for (uint32_t o = 0; o < count; ++o) items[o].status = 0;
      return asp::set_error(ASP_ERR_INVALID, "item %u: couplings overflow double range", d);
    }
  }
  // ---- valid: the applied plans take the new numbers ----
  for (uint32_t d = 0; d < count; ++d) {
    asp_sa_stencil_item &it = items[d];
    if (it.status != 0) continue;
    ASP_TRY(asp::rw_commit_data(it.plan, st->b_staged.ptr + static_cast<size_t>(d) * entries, &st->spare[d],
                                diag_sum[d], s));
    if (it.field) {
      ASP_TRY(asp::rw_commit_field(it.plan, st->b_field.ptr + static_cast<size_t>(d) * K,
                                   field_now.data() + static_cast<size_t>(d) * K, s));
    }
    asp::sa_finish_scales(scales[d].bound, scales[d].max_delta, scales[d].min_delta, &it.plan->host);
    if (it.data_out) {
      ASP_HIP_TRY(hipMemcpyAsync(it.data_out, st->b_data.ptr + static_cast<size_t>(d) * nnz, nnz * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
    }
  }
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(st->ev[1], s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  ASP_HIP_TRY(hipEventElapsedTime(&g_batch_ms, st->ev[0], st->ev[1]));
  return ASP_OK;
}

float asp_sa_plan_reweight_stencil_last_ms(void) { return g_batch_ms; }

}  // extern "C"
