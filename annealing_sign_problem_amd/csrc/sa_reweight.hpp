// The steps of a reweight (csrc/sa_reweight.hip) that asp_sa_plan_reweight and the
// batched route from a coupling stencil (csrc/ising_stencil.hip, asp_sa_plan_reweight_stencil_batch) share:
// the maps of a plan's family, the merge and row statistics from couplings that lie on the DEVICE, the
// fold of the scales in row order, and the step that makes a plan take the numbers.  A caller queues the
// device steps on a stream of its choice (the plan's buffers are idle between entry points) and
// synchronises that stream itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "sa_internal.hpp"

namespace asp {

// Builds and uploads SaPattern's maps once per family (on the plan's stream, which it waits for).
int rw_ensure_maps(asp_sa_plan *p);

// staged[e] = J_ij + J_ji of every entry e of A from `d_data` (pattern order, on the device); *d_zeros
// (cleared here) counts the entries that cancel exactly.
int rw_queue_merge(const asp_sa_plan *p, const double *d_data, double *d_staged, uint32_t *d_zeros,
                   hipStream_t s);
// Per row: sum |A_ij| in a_ptr order and the smallest non-zero 2 |A_ij| (+inf: none).
int rw_queue_row_stats(const asp_sa_plan *p, const double *d_staged, double *d_row_sum, double *d_row_min,
                       hipStream_t s);

struct RwScales {
  double bound = 0.0, max_delta = 0.0, min_delta = 0.0;
};
// The scales, rows folded in index order (sa_plan.cpp, "energy scale and automatic beta range");
// false: the bound is not finite.
bool rw_fold_scales(uint64_t K, const double *row_sum, const double *row_min, const double *field_now,
                    RwScales *out);

// The plan takes the merged values: the scatter into every value array it holds on the device (queued
// on `s`), the host mirrors (a_val is swapped in) and diag_sum.
int rw_commit_data(asp_sa_plan *p, const double *d_staged, std::vector<double> *a_val, double diag_sum,
                   hipStream_t s);
// The plan takes the field (`d_field`: its K values on the device, `field_now` the same on the host).
int rw_commit_field(asp_sa_plan *p, const double *d_field, const double *field_now, hipStream_t s);

}  // namespace asp
