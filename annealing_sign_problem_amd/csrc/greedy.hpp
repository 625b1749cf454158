// Host helpers of the batched greedy solve (csrc/greedy.cpp), kept out of sa_plan.hpp so that the
// shuffled sweep's source-set fingerprint (build.KERNEL_SOURCE_SETS) does not move with them.
#pragma once

#include <cstddef>
#include <cstdint>

#include "sa_plan.hpp"

namespace asp {

// greedy_tree_signs for `count` problems, x[i] = configuration of layouts[i], on up to 8 threads.
void greedy_tree_signs_many(const SaHostLayout *const *layouts, uint64_t *const *x, size_t count);

}  // namespace asp
