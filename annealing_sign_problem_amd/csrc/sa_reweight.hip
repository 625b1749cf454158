// New couplings and fields on the structure of an existing plan (asp_sa_plan_reweight) and a second
// plan of the same structure (asp_sa_plan_clone), both without build_sa_layout: the colouring, the
// permutation and the sliced-ELL structure depend on the PATTERN of J alone (DSATUR breaks ties by
// degree and index, never by value).  Specification: DESIGN.md §4.14.  gfx950 only.
//
// A reweight uploads `data` and `field` once.  k_rw_merge forms v = J_ij + J_ji of every entry of A
// from recorded positions (an absent side is +0.0: the sum build_sa_layout forms), k_rw_row_stats the
// per-row sum |A_ij| in a_ptr order and the smallest non-zero 2 |A_ij|; the host folds the rows in
// index order into the bound and the scales (sa_finish_scales), so every number equals a fresh plan's
// bit for bit.  Only when everything is valid do k_rw_scatter / k_rw_field write the value arrays the
// plan holds on the device; the lazily uploaded ones are built from the updated host layout as ever.
//
// The steps — maps, merge, row statistics, scales, commit — are functions of their own (sa_reweight.hpp):
// asp_sa_plan_reweight_stencil_batch (csrc/ising_stencil.hip) runs them for a round of plans on couplings
// that are on the device already.
//
// Nothing else of a plan caches a function of the couplings across calls: the field cache
// (w_field_cache) is switched on inside a launch, from cache_ctl in LDS that every launch zeroes, and
// filled before it is read; the other w_* buffers are per-call scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "asp_common.hpp"
#include "sa_internal.hpp"
#include "sa_reweight.hpp"

namespace {

using asp::SaPattern;

constexpr uint32_t kNone = SaPattern::kNone;
constexpr int kThreads = 256;

// staged[e] = J_ij + J_ji of entry e of A; *zeros counts the entries that cancel exactly (a fresh
// plan would have dropped them: the pattern of A has changed).
__global__ __launch_bounds__(kThreads) void k_rw_merge(const double *__restrict__ data,
                                                       const uint32_t *__restrict__ src_ij,
                                                       const uint32_t *__restrict__ src_ji, uint64_t entries,
                                                       double *__restrict__ staged, uint32_t *zeros) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; e < entries; e += stride) {
    const uint32_t a = src_ij[e], b = src_ji[e];
    const double x = a != kNone ? data[a] : 0.0;  // J_ij or +0
    const double y = b != kNone ? data[b] : 0.0;  // J_ji or +0
    const double v = x + y;
    staged[e] = v;
    if (v == 0.0) atomicAdd(zeros, 1u);
  }
}

// One thread per row: the row's entries in a_ptr order, as build_sa_layout's scale loop adds them.
__global__ __launch_bounds__(kThreads) void k_rw_row_stats(const double *__restrict__ staged,
                                                           const int64_t *__restrict__ a_ptr, uint32_t rows,
                                                           double *__restrict__ row_sum,
                                                           double *__restrict__ row_min) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < rows; i += stride) {
    double row = 0.0;
    double least = __longlong_as_double(0x7FF0000000000000ll);  // +inf
    for (int64_t k = a_ptr[i]; k < a_ptr[i + 1]; ++k) {
      const double a = fabs(staged[k]);
      row += a;
      const double twice = 2.0 * a;
      if (a > 0.0 && twice < least) least = twice;
    }
    row_sum[i] = row;
    row_min[i] = least;
  }
}

// The merged values into the arrays the plan holds: the sliced ELL, the rows padded to quads (the
// shuffled sweep; nullptr: not uploaded yet) and the plain rows (cluster moves, device tree; same).
__global__ __launch_bounds__(kThreads) void k_rw_scatter(const double *__restrict__ staged,
                                                         const uint64_t *__restrict__ ell_slot,
                                                         const uint32_t *__restrict__ rq_slot, uint64_t entries,
                                                         double *__restrict__ ell_val, double *__restrict__ rq_val,
                                                         double *__restrict__ rows_val) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; e < entries; e += stride) {
    const double v = staged[e];
    ell_val[ell_slot[e]] = v;
    if (rq_val != nullptr) rq_val[rq_slot[e]] = v;
    if (rows_val != nullptr) rows_val[e] = v;
  }
}

// The field in block order and, where they exist, its two copies in original order.
__global__ __launch_bounds__(kThreads) void k_rw_field(const double *__restrict__ field,
                                                       const uint32_t *__restrict__ pos_of_spin, uint32_t rows,
                                                       double *__restrict__ field_pos,
                                                       double *__restrict__ field_dev,
                                                       double *__restrict__ rows_field) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < rows; i += stride) {
    const double h = field[i];
    field_pos[pos_of_spin[i]] = h;
    if (field_dev != nullptr) field_dev[i] = h;
    if (rows_field != nullptr) rows_field[i] = h;
  }
}

// (every kernel above strides over its items by the grid: the cap loses none)
unsigned grid_for(uint64_t items) {
  return static_cast<unsigned>(std::min<uint64_t>((items + kThreads - 1) / kThreads, 1u << 16));
}

// Position of column `col` in row `row` of the pattern, or -1.
int64_t find_in_row(const SaPattern &P, uint64_t row, int32_t col) {
  const int32_t *begin = P.indices.data() + P.indptr[row], *end = P.indices.data() + P.indptr[row + 1];
  const int32_t *at = std::lower_bound(begin, end, col);
  return at != end && *at == col ? P.indptr[row] + (at - begin) : -1;
}

}  // namespace

namespace asp {

// The maps of SaPattern, from the pattern and the layout of the plan; uploaded on the plan's stream.
int rw_ensure_maps(asp_sa_plan *p) {
  SaPattern &P = *p->pattern;
  std::lock_guard<std::mutex> guard(P.build);
  if (P.built) return ASP_OK;
  const asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  const uint64_t entries = L.a_col.size();
  if (P.nnz >= kNone || entries >= kNone) {
    return asp::set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 2 couplings: the plan cannot be reweighted");
  }
  P.src_ij.assign(entries, kNone);
  P.src_ji.assign(entries, kNone);
  P.ell_slot.assign(entries, 0);
  P.rq_slot.assign(entries, 0);
  P.diag_pos.assign(K, -1);
  P.dropped.clear();
  std::vector<uint8_t> used(P.nnz, 0);
  const uint64_t ell_elems = L.ell_off.back() * 64;
  uint64_t quad = 0;  // build_row_quads' quad_ptr
  for (uint64_t i = 0; i < K; ++i) {
    const uint32_t pos = L.pos_of_spin[i];
    const uint32_t b = pos / 64u, lane = pos % 64u;
    const int64_t degree = L.a_ptr[i + 1] - L.a_ptr[i];
    if (static_cast<uint64_t>(degree) > L.block_width[b]) {
      return asp::set_error(ASP_ERR_INVALID, "row %llu is wider than its block", (unsigned long long)i);
    }
    for (int64_t k = 0; k < degree; ++k) {
      const uint64_t e = static_cast<uint64_t>(L.a_ptr[i] + k);
      const int32_t j = L.a_col[e];
      const int64_t ij = find_in_row(P, i, j), ji = find_in_row(P, static_cast<uint64_t>(j), static_cast<int32_t>(i));
      if (ij >= 0) {
        P.src_ij[e] = static_cast<uint32_t>(ij);
        used[ij] = 1;
      }
      if (ji >= 0) {
        P.src_ji[e] = static_cast<uint32_t>(ji);
        used[ji] = 1;
      }
      // the element of the quad-interleaved ELL (sa_plan.cpp, "sliced ELL")
      const uint64_t q = (L.ell_off[b] + static_cast<uint64_t>(k)) / 4;
      const uint32_t jj = static_cast<uint32_t>(k % 4);
      P.ell_slot[e] = ((q * 2 + jj / 2) * 64 + lane) * 2 + (jj % 2);
      if (P.ell_slot[e] >= ell_elems) {
        return asp::set_error(ASP_ERR_INVALID, "ELL element of row %llu out of range", (unsigned long long)i);
      }
      P.rq_slot[e] = static_cast<uint32_t>(quad * 4 + static_cast<uint64_t>(k));
    }
    quad += static_cast<uint64_t>(degree + 3) / 4;
    if (quad >= (1ull << 30)) quad = 0;  // (build_row_quads refuses such a plan: rq_val never exists)
  }
  for (uint64_t i = 0; i < K; ++i) {
    for (int64_t k = P.indptr[i]; k < P.indptr[i + 1]; ++k) {
      const uint64_t j = static_cast<uint64_t>(P.indices[k]);
      if (j == i) {
        P.diag_pos[i] = k;
      } else if (!used[k]) {
        const int64_t mirror = find_in_row(P, j, static_cast<int32_t>(i));
        if (mirror < 0 || i < j) P.dropped.emplace_back(k, mirror);
      }
    }
  }
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);
  ASP_TRY(asp::upload_vector(P.d_src_ij, P.src_ij, s));
  ASP_TRY(asp::upload_vector(P.d_src_ji, P.src_ji, s));
  ASP_TRY(asp::upload_vector(P.d_ell_slot, P.ell_slot, s));
  ASP_TRY(asp::upload_vector(P.d_rq_slot, P.rq_slot, s));
  ASP_TRY(asp::upload_vector(P.d_a_ptr, L.a_ptr, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  P.built = true;
  return ASP_OK;
}

int rw_queue_merge(const asp_sa_plan *p, const double *d_data, double *d_staged, uint32_t *d_zeros,
                   hipStream_t s) {
  const SaPattern &P = *p->pattern;
  const uint64_t entries = p->host.a_col.size();
  ASP_HIP_TRY(hipMemsetAsync(d_zeros, 0, sizeof(uint32_t), s));
  if (entries > 0) {
    hipLaunchKernelGGL(k_rw_merge, dim3(grid_for(entries)), dim3(kThreads), 0, s, d_data, P.d_src_ij.ptr,
                       P.d_src_ji.ptr, entries, d_staged, d_zeros);
  }
  return ASP_OK;
}

int rw_queue_row_stats(const asp_sa_plan *p, const double *d_staged, double *d_row_sum, double *d_row_min,
                       hipStream_t s) {
  const uint64_t K = p->host.num_spins;
  hipLaunchKernelGGL(k_rw_row_stats, dim3(grid_for(K)), dim3(kThreads), 0, s, d_staged, p->pattern->d_a_ptr.ptr,
                     static_cast<uint32_t>(K), d_row_sum, d_row_min);
  ASP_HIP_TRY(hipGetLastError());
  return ASP_OK;
}

bool rw_fold_scales(uint64_t K, const double *row_sum, const double *row_min, const double *field_now,
                    RwScales *out) {
  double bound = 0.0, max_delta = 0.0;
  double min_delta = std::numeric_limits<double>::infinity();
  for (uint64_t i = 0; i < K; ++i) {
    const double row = row_sum[i];
    min_delta = std::min(min_delta, row_min[i]);
    const double h = std::fabs(field_now[i]);
    if (h > 0.0) min_delta = std::min(min_delta, 2.0 * h);
    bound += 0.5 * row + h;
    max_delta = std::max(max_delta, 2.0 * (row + h));
  }
  out->bound = bound;
  out->max_delta = max_delta;
  out->min_delta = min_delta;
  return std::isfinite(bound);
}

int rw_commit_data(asp_sa_plan *p, const double *d_staged, std::vector<double> *a_val, double diag_sum,
                   hipStream_t s) {
  const SaPattern &P = *p->pattern;
  asp::SaHostLayout &L = p->host;
  const uint64_t entries = L.a_col.size();
  if (entries > 0) {
    hipLaunchKernelGGL(k_rw_scatter, dim3(grid_for(entries)), dim3(kThreads), 0, s, d_staged, P.d_ell_slot.ptr,
                       P.d_rq_slot.ptr, entries, p->ell_val.ptr, p->rq_ptr.ptr ? p->rq_val.ptr : nullptr,
                       p->cluster_row_ptr.ptr ? p->cluster_val.ptr : nullptr);
  }
  L.diag_sum = diag_sum;
  for (uint64_t e = 0; e < entries; ++e) L.ell_val[P.ell_slot[e]] = (*a_val)[e];
  L.a_val.swap(*a_val);
  return ASP_OK;
}

int rw_commit_field(asp_sa_plan *p, const double *d_field, const double *field_now, hipStream_t s) {
  asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  hipLaunchKernelGGL(k_rw_field, dim3(grid_for(K)), dim3(kThreads), 0, s, d_field, p->pos_of_spin.ptr,
                     static_cast<uint32_t>(K), p->field_pos.ptr, p->rq_ptr.ptr ? p->field_dev.ptr : nullptr,
                     p->cluster_row_ptr.ptr ? p->cluster_field.ptr : nullptr);
  for (uint64_t i = 0; i < K; ++i) L.field_pos[L.pos_of_spin[i]] = field_now[i];
  return ASP_OK;
}

}  // namespace asp

extern "C" {

int asp_sa_plan_reweight(asp_sa_plan *p, uint64_t nnz, int64_t const *indptr, int32_t const *indices,
                         double const *data, double const *field) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  asp::SaHostLayout &L = p->host;
  const uint64_t K = L.num_spins;
  SaPattern &P = *p->pattern;
  // ---- everything that can be refused, before anything of the plan is touched ----
  if (nnz != P.nnz) {
    return asp::set_error(ASP_ERR_INVALID, "pattern mismatch: %llu stored entries, the plan was created from %llu",
                          (unsigned long long)nnz, (unsigned long long)P.nnz);
  }
  if (K > 0) {
    if (!indptr || (nnz > 0 && !indices)) return asp::set_error(ASP_ERR_INVALID, "null indptr/indices");
    for (uint64_t i = 0; i <= K; ++i) {
      if (indptr[i] != P.indptr[i]) {
        return asp::set_error(ASP_ERR_INVALID, "pattern mismatch: indptr[%llu] differs from the plan's",
                              (unsigned long long)i);
      }
    }
    if (nnz > 0 && std::memcmp(indices, P.indices.data(), nnz * sizeof(int32_t)) != 0) {
      uint64_t k = 0;
      while (indices[k] == P.indices[k]) ++k;
      return asp::set_error(ASP_ERR_INVALID, "pattern mismatch: indices[%llu] differs from the plan's",
                            (unsigned long long)k);
    }
  }
  if (K == 0) return ASP_OK;  // no spins: nothing to reweight
  if (!data && !field) return asp::set_error(ASP_ERR_INVALID, "neither data nor field given");
  if (p->live_chains->load(std::memory_order_relaxed) > 0) {
    return asp::set_error(ASP_ERR_INVALID,
                          "the plan has %d live chains handle(s): their tracked energies belong to the old couplings",
                          p->live_chains->load(std::memory_order_relaxed));
  }
  for (uint64_t i = 0; i < K; ++i) {  // (asp_sa_plan_create's messages)
    if (data) {
      for (int64_t k = P.indptr[i]; k < P.indptr[i + 1]; ++k) {
        if (!std::isfinite(data[k])) {
          return asp::set_error(ASP_ERR_INVALID, "non-finite coupling in row %llu", (unsigned long long)i);
        }
      }
    }
    if (field && !std::isfinite(field[i])) {
      return asp::set_error(ASP_ERR_INVALID, "non-finite field at %llu", (unsigned long long)i);
    }
  }
  ASP_TRY(asp::bind_device());
  ASP_TRY(asp::rw_ensure_maps(p));
  if (data) {
    for (const auto &pair : P.dropped) {
      const double v = data[pair.first] + (pair.second >= 0 ? data[pair.second] : 0.0);
      if (v != 0.0) {
        return asp::set_error(ASP_ERR_INVALID,
                              "pattern mismatch: a coupling that cancelled when the plan was created (stored entry "
                              "%lld) no longer does",
                              (long long)pair.first);
      }
    }
  }
  const uint64_t entries = L.a_col.size();
  std::vector<double> field_now(K);
  if (field) {
    std::copy(field, field + K, field_now.begin());
  } else {
    for (uint64_t i = 0; i < K; ++i) field_now[i] = L.field_pos[L.pos_of_spin[i]];
  }
  std::vector<double> a_val(data ? entries : 0), row_sum(K), row_min(K);
  uint32_t zeros = 0;
  hipStream_t s = p->stream;
  asp::StreamFence fence(s);  // (no exit leaves a copy from or into the vectors above in flight)
  ASP_TRY(p->rw_a_val.ensure(entries));
  ASP_TRY(p->rw_row_sum.ensure(K));
  ASP_TRY(p->rw_row_min.ensure(K));
  ASP_TRY(p->rw_zeros.ensure(1));
  if (field) ASP_TRY(p->rw_field.ensure(K));
  ASP_HIP_TRY(hipEventRecord(p->ev[0], s));
  if (data) {
    ASP_TRY(p->rw_data.ensure(nnz));
    ASP_TRY(p->rw_data.upload(data, nnz, s));
    ASP_TRY(asp::rw_queue_merge(p, p->rw_data.ptr, p->rw_a_val.ptr, p->rw_zeros.ptr, s));
  } else {
    ASP_TRY(p->rw_a_val.upload(L.a_val.data(), entries, s));  // field only: the rows as they are
  }
  ASP_TRY(asp::rw_queue_row_stats(p, p->rw_a_val.ptr, p->rw_row_sum.ptr, p->rw_row_min.ptr, s));
  ASP_TRY(p->rw_row_sum.download(row_sum.data(), K, s));
  ASP_TRY(p->rw_row_min.download(row_min.data(), K, s));
  if (data) {
    ASP_TRY(p->rw_a_val.download(a_val.data(), entries, s));
    ASP_TRY(p->rw_zeros.download(&zeros, 1, s));
  }
  ASP_HIP_TRY(hipStreamSynchronize(s));
  if (zeros != 0) {
    uint64_t e = 0;
    while (e < entries && a_val[e] != 0.0) ++e;
    const uint64_t row = static_cast<uint64_t>(std::upper_bound(L.a_ptr.begin(), L.a_ptr.end(), static_cast<int64_t>(e)) -
                                               L.a_ptr.begin()) - 1;
    return asp::set_error(ASP_ERR_INVALID,
                          "pattern mismatch: J_ij + J_ji of (%llu, %d) is now exactly 0 (%u such entries); a fresh "
                          "plan would drop it",
                          (unsigned long long)row, e < entries ? L.a_col[e] : -1, zeros);
  }
  // the scales, rows in index order (sa_plan.cpp, "energy scale and automatic beta range")
  asp::RwScales scales;
  if (!asp::rw_fold_scales(K, row_sum.data(), row_min.data(), field_now.data(), &scales)) {
    return asp::set_error(ASP_ERR_INVALID, "couplings overflow double range");
  }
  // ---- valid: the plan takes the new numbers ----
  if (data) {
    double diag = 0.0;  // D in row order
    for (uint64_t i = 0; i < K; ++i) {
      if (P.diag_pos[i] >= 0) diag = diag + data[P.diag_pos[i]];
    }
    ASP_TRY(asp::rw_commit_data(p, p->rw_a_val.ptr, &a_val, diag, s));
  }
  if (field) {
    ASP_TRY(p->rw_field.upload(field_now.data(), K, s));
    ASP_TRY(asp::rw_commit_field(p, p->rw_field.ptr, field_now.data(), s));
  }
  asp::sa_finish_scales(scales.bound, scales.max_delta, scales.min_delta, &L);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(p->ev[3], s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  ASP_HIP_TRY(hipEventElapsedTime(&p->rw_last_ms, p->ev[0], p->ev[3]));
  return ASP_OK;
}

float asp_sa_plan_reweight_last_ms(asp_sa_plan const *p) { return p ? p->rw_last_ms : 0.0f; }

int asp_sa_plan_clone(asp_sa_plan const *p, asp_sa_plan **out) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (!out) return asp::set_error(ASP_ERR_INVALID, "null output pointer");
  *out = nullptr;
  ASP_TRY(asp::bind_device());
  asp_sa_plan *c = new (std::nothrow) asp_sa_plan();
  if (!c) return asp::set_error(ASP_ERR_ALLOC, "out of host memory");
  c->host = p->host;  // (copies of the structure: the clone outlives its source)
  c->pattern = p->pattern;
  c->force_m = p->force_m;
  c->force_threads = p->force_threads;
  c->force_packed = p->force_packed;
  c->spin_lds_limit = p->spin_lds_limit;
  c->allow_wide = p->allow_wide;
  c->team_mode = p->team_mode;
  c->use_field_cache = p->use_field_cache;
  c->tail_mode = p->tail_mode;
  c->use_post = p->use_post;
  c->shuffled_m = p->shuffled_m;
  c->shuffled_waves = p->shuffled_waves;
  c->shuffled_teams = p->shuffled_teams;
  c->greedy_tree = p->greedy_tree;
  const int rc = asp::sa_plan_device_setup(c);
  if (rc != ASP_OK) {
    asp_sa_plan_destroy(c);
    return rc;
  }
  *out = c;
  return ASP_OK;
}

}  // extern "C"
