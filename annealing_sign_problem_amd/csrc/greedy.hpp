// Host helpers of the batched greedy solve (csrc/greedy.cpp), kept out of sa_plan.hpp so that the
// shuffled sweep's source-set fingerprint (build.KERNEL_SOURCE_SETS) does not move with them.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sa_plan.hpp"

struct asp_sa_plan;

namespace asp {

// greedy_tree_signs for `count` problems, x[i] = configuration of layouts[i], on up to 8 threads.
void greedy_tree_signs_many(const SaHostLayout *const *layouts, uint64_t *const *x, size_t count);

// The same trees on the device (csrc/greedy_tree.hip), word for word: the problems of one call share
// the launches of the bond build, the sorts and the orientation, and every problem is one workgroup of
// k_greedy_tree.  Distinct plans; a plan without spins is skipped.  The words of target t go to d_out
// (DEVICE, written on `stream`) when it is set and to h_out (HOST) otherwise.  The stream is idle on
// return.  split_ms (may be null): device time of bonds + sort, k_greedy_tree, orientation + packing.
struct GreedyTreeTarget {
  asp_sa_plan *plan;
  uint64_t *d_out;
  uint64_t *h_out;
};
int greedy_tree_device(const GreedyTreeTarget *targets, uint32_t count, hipStream_t stream, float split_ms[3]);
// Whether the plan's forest lives in LDS (asp_sa_set_greedy_tree, the plan's LDS limit).
bool greedy_forest_in_lds(const asp_sa_plan *p);
// What asp_sa_greedy_tree_last_ms reports: set to (add: increased by) the three times of one call.
void greedy_tree_record_ms(const float split_ms[3], bool add);

}  // namespace asp
