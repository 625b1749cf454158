// The strongest-coupling tree of the greedy solver (ASP-GREEDY-1) on the
// device: the same law as greedy_tree_signs (csrc/greedy.cpp), word for word.
//
//   Stage A (all problems of a call in shared launches): per row the number of stored entries with
//     j > i (a binary search, the columns ascend), one device-wide scan over the rows of all
//     problems, the bonds emitted in generation order with the key ~bits(|w|), one stable radix sort
//     of all bonds by that key and, for a batch, one stable sort by the problem index: every problem's
//     bonds end up contiguous and in the law's order.
//   Stage B (k_greedy_tree, one workgroup per problem): the signed forest — one word per spin, parent
//     index with the flip in the top bit, all-ones = unassigned, and the size of a root — lives in LDS
//     when it fits and in a per-problem slab of HBM otherwise.  The workgroup takes the sorted bonds in
//     windows of one bond per lane: every lane finds the roots of both ends and drops the bond when they
//     agree (clusters only merge, so such a bond is a skip forever); the survivors, compacted in sorted
//     order, are applied one at a time, each classified against the forest as it then stands.  The row
//     sum of a fresh spin is taken by wavefront 0: a find per lane and neighbour, then the terms folded
//     left to right in column order through cross-lane reads.
//   Stage C (k_greedy_orient, one workgroup per problem): with a field, one wavefront walks the spins
//     ascending in chunks of 64 and keeps the running sum of a run of one root in a register; then the
//     bits are packed with ballots into words in original order.
//
// Every loop is bounded (find by the number of spins, windows by the bond count); there is no wait on
// another lane, wavefront or workgroup besides the workgroup barrier.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "asp_common.hpp"
#include "greedy.hpp"
#include "sa_internal.hpp"

namespace {

using asp::DeviceBuffer;

constexpr uint32_t kNone = 0xFFFFFFFFu;  // forest word of a spin no bond has touched yet
constexpr uint32_t kFlip = 0x80000000u;  // sign relative to the parent: set = opposite
constexpr uint32_t kTreeThreads = 256;   // workgroup of k_greedy_tree = its filter window
constexpr uint32_t kRowThreads = 256;
constexpr size_t kTreeStaticLds = 8192;  // upper bound of k_greedy_tree's static LDS

struct TreeProblem {
  const uint32_t *row_ptr;  // rows of A over original indices (asp_sa_plan::cluster_*)
  const uint32_t *col;
  const double *val;
  const double *field;      // original order
  uint32_t *forest;         // HBM form: [2 K] words; nullptr: LDS
  uint64_t *out;            // device, ceil(K/64) words
  uint32_t num_spins;
  uint32_t row_at;          // first row of the problem among the rows of the call
  uint32_t has_field;       // some h is not +-0: the orientation pass runs
  uint32_t pad;
};

// ---- stage A -------------------------------------------------------------------------------------

// The problem of global row r: the last k with row_at[k] <= r (row_at ascends strictly, row_at[0] = 0).
__device__ inline uint32_t problem_of_row(const TreeProblem *problems, uint32_t count, uint32_t r) {
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (problems[mid].row_at <= r) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// counts[r] = stored entries of the row with column > row; first_upper[r] = the first of them.
__global__ __launch_bounds__(kRowThreads) void k_greedy_bond_count(const TreeProblem *problems, uint32_t count,
                                                                   uint32_t total_rows, uint32_t *counts,
                                                                   uint32_t *first_upper) {
  const uint32_t r = blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= total_rows) return;
  const TreeProblem &P = problems[problem_of_row(problems, count, r)];
  const uint32_t i = r - P.row_at;
  uint32_t lo = P.row_ptr[i];
  const uint32_t end = P.row_ptr[i + 1];
  uint32_t hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (P.col[mid] > i) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  counts[r] = end - lo;
  first_upper[r] = lo;
}

// Bond g (global generation order: problems in call order, rows ascending, columns ascending).
__global__ __launch_bounds__(kRowThreads) void k_greedy_bond_emit(const TreeProblem *problems, uint32_t count,
                                                                  uint32_t total_rows, const int64_t *bond_scan,
                                                                  const uint32_t *first_upper, uint64_t capacity,
                                                                  uint64_t *keys, uint32_t *values, uint32_t *bond_row,
                                                                  uint32_t *bond_entry, uint32_t *bond_problem) {
  const uint32_t r = blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= total_rows) return;
  const uint32_t k_problem = problem_of_row(problems, count, r);
  const TreeProblem &P = problems[k_problem];
  const uint32_t i = r - P.row_at;
  const uint32_t end = P.row_ptr[i + 1];
  uint64_t g = static_cast<uint64_t>(bond_scan[r]);
  for (uint32_t k = first_upper[r]; k < end && g < capacity; ++k, ++g) {
    keys[g] = ~static_cast<uint64_t>(__double_as_longlong(fabs(P.val[k])));
    values[g] = static_cast<uint32_t>(g);
    bond_row[g] = i;
    bond_entry[g] = k;
    if (bond_problem) bond_problem[g] = k_problem;
  }
}

__global__ __launch_bounds__(kRowThreads) void k_greedy_problem_keys(const uint32_t *sorted, const uint32_t *bond_problem,
                                                                     uint64_t n, uint32_t *keys) {
  const uint64_t b = static_cast<uint64_t>(blockIdx.x) * kRowThreads + threadIdx.x;
  if (b < n) keys[b] = bond_problem[sorted[b]];
}

// ---- stage B -------------------------------------------------------------------------------------

__device__ inline uint32_t forest_load(const uint32_t *node, uint32_t v) {
  return __hip_atomic_load(node + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ inline void forest_store(uint32_t *node, uint32_t v, uint32_t word) {
  __hip_atomic_store(node + v, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Root of the ASSIGNED spin v and v's sign relative to it (top bit), reading only.
__device__ inline uint32_t find_root(const uint32_t *node, uint32_t v, uint32_t num_spins) {
  uint32_t at = v, sign = 0;
  for (uint32_t step = 0; step < num_spins; ++step) {
    const uint32_t word = forest_load(node, at);
    const uint32_t up = word & ~kFlip;
    if (up == at) break;
    sign ^= word & kFlip;
    at = up;
  }
  return at | sign;
}

// The same for the one lane of the serial phase, compressing the whole path as the host's find does.
__device__ inline uint32_t find_root_compress(uint32_t *node, uint32_t v, uint32_t num_spins) {
  const uint32_t found = find_root(node, v, num_spins);
  const uint32_t root = found & ~kFlip;
  uint32_t carried = found & kFlip;
  for (uint32_t step = 0; step < num_spins && v != root; ++step) {
    const uint32_t word = forest_load(node, v);
    const uint32_t up = word & ~kFlip;
    if (up == root) break;
    forest_store(node, v, root | carried);
    carried ^= word & kFlip;
    v = up;
  }
  return found;
}

struct TreeArgs {
  const TreeProblem *problems;
  const uint32_t *which;      // the problems of this launch
  const int64_t *bond_scan;   // [rows of the call + 1]
  const uint32_t *sorted;     // global generation index of every bond, problems contiguous, the law's order
  const uint32_t *bond_row;   // by generation index: i
  const uint32_t *bond_entry; // by generation index: the entry of the problem's CSR (j, w)
  uint32_t *root_sign;        // [rows of the call] out: root | down << 31 of every spin
  uint64_t capacity;          // entries of `sorted`
};

template <bool HBM>
__global__ __launch_bounds__(kTreeThreads) void k_greedy_tree(TreeArgs a) {
  extern __shared__ uint32_t lds_forest[];
  __shared__ uint32_t s_i[kTreeThreads], s_j[kTreeThreads];
  __shared__ double s_w[kTreeThreads];
  __shared__ uint32_t s_wave_count[kTreeThreads / 64];
  __shared__ uint32_t s_fresh, s_root, s_unions;

  const TreeProblem P = a.problems[a.which[blockIdx.x]];
  const uint32_t K = P.num_spins;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t *node = HBM ? P.forest : lds_forest;
  uint32_t *size = node + K;
  for (uint32_t v = tid; v < K; v += kTreeThreads) {
    node[v] = kNone;
    size[v] = 1u;
  }
  if (tid == 0) s_unions = 0u;
  __syncthreads();

  const uint64_t first = static_cast<uint64_t>(a.bond_scan[P.row_at]);
  uint64_t num_bonds = static_cast<uint64_t>(a.bond_scan[P.row_at + K]) - first;
  if (first + num_bonds > a.capacity) num_bonds = first < a.capacity ? a.capacity - first : 0;  // (never: A is symmetric)
  uint32_t unions = 0;  // (thread 0's count)
  for (uint64_t base = 0; base < num_bonds; base += kTreeThreads) {
    // ---- filter: nobody merges here, so a find may store its own answer (a pointer to the root that
    // every other reader may follow instead of the old one) ----
    const uint64_t b = base + tid;
    uint32_t i = 0, j = 0;
    double w = 0.0;
    bool survives = false;
    if (b < num_bonds) {
      const uint32_t g = a.sorted[first + b];
      i = a.bond_row[g];
      const uint32_t entry = a.bond_entry[g];
      j = P.col[entry];
      w = P.val[entry];
      const uint32_t word_i = forest_load(node, i), word_j = forest_load(node, j);
      survives = true;
      if (word_i != kNone && word_j != kNone) {
        const uint32_t found_i = find_root(node, i, K), found_j = find_root(node, j, K);
        if ((found_i & ~kFlip) != i) forest_store(node, i, found_i);
        if ((found_j & ~kFlip) != j) forest_store(node, j, found_j);
        survives = (found_i & ~kFlip) != (found_j & ~kFlip);
      }
    }
    const uint64_t ballot = __ballot(survives);
    if (lane == 0) s_wave_count[wave] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    uint32_t before = 0, survivors = 0;
    for (uint32_t q = 0; q < kTreeThreads / 64; ++q) {
      const uint32_t c = s_wave_count[q];
      if (q < wave) before += c;
      survivors += c;
    }
    if (survives) {
      const uint32_t at = before + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
      s_i[at] = i;
      s_j[at] = j;
      s_w[at] = w;
    }
    __syncthreads();
    // ---- the survivors one at a time, in sorted order ----
    for (uint32_t s = 0; s < survivors; ++s) {
      if (tid == 0) {
        const uint32_t bi = s_i[s], bj = s_j[s];
        const double bw = s_w[s];
        const uint32_t word_i = forest_load(node, bi), word_j = forest_load(node, bj);
        uint32_t fresh = kNone, root = 0;
        if (word_i == kNone && word_j == kNone) {
          node[bi] = bi;
          node[bj] = bi | (bw > 0.0 ? kFlip : 0u);
          size[bi] = 2u;
          ++unions;
        } else if (word_i == kNone || word_j == kNone) {
          fresh = word_i == kNone ? bi : bj;
          root = find_root_compress(node, word_i == kNone ? bj : bi, K) & ~kFlip;
          ++unions;
        } else {
          const uint32_t found_i = find_root_compress(node, bi, K), found_j = find_root_compress(node, bj, K);
          const uint32_t ri = found_i & ~kFlip, rj = found_j & ~kFlip;
          if (ri != rj) {  // (an earlier survivor of this window may have merged them)
            const bool frustrated = ((found_i & kFlip) == (found_j & kFlip)) == (bw > 0.0);
            uint32_t keep = ri, gone = rj;
            if (size[rj] > size[ri]) {
              keep = rj;
              gone = ri;
            }
            node[gone] = keep | (frustrated ? kFlip : 0u);
            size[keep] += size[gone];
            ++unions;
          }
        }
        s_fresh = fresh;
        s_root = root;
      }
      __syncthreads();
      const uint32_t fresh = s_fresh;
      if (fresh != kNone && wave == 0) {
        // the fresh spin's bonds into THAT cluster as it stands, summed in ascending column order
        const uint32_t root = s_root;
        const uint32_t row_end = P.row_ptr[fresh + 1];
        double energy = 0.0;
        for (uint32_t k0 = P.row_ptr[fresh]; k0 < row_end; k0 += 64u) {
          const uint32_t k = k0 + lane;
          double term = 0.0;
          if (k < row_end) {
            const uint32_t other = P.col[k];
            if (forest_load(node, other) != kNone) {
              const uint32_t found = find_root(node, other, K);
              if ((found & ~kFlip) == root) {
                const double value = P.val[k];
                term = (found & kFlip) ? -value : value;
              }
            }
          }
          const uint32_t n = row_end - k0 < 64u ? row_end - k0 : 64u;
          for (uint32_t l = 0; l < n; ++l) energy = __dadd_rn(energy, __shfl(term, static_cast<int>(l), 64));
        }
        if (lane == 0) {
          node[fresh] = root | (energy > 0.0 ? kFlip : 0u);
          size[root] += 1u;
        }
      }
      __syncthreads();
    }
    // every spin in one cluster: all later bonds are skips
    if (tid == 0) s_unions = unions;
    __syncthreads();
    if (s_unions + 1u >= K) break;
  }
  __syncthreads();
  // ---- root and sign of every spin; a spin no bond touched is a +1 cluster of its own ----
  uint32_t *root_sign = a.root_sign + P.row_at;
  for (uint32_t v = tid; v < K; v += kTreeThreads) {
    root_sign[v] = forest_load(node, v) == kNone ? v : find_root(node, v, K);
  }
}

// ---- stage C -------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTreeThreads) void k_greedy_orient(const TreeProblem *problems, const uint32_t *root_sign_all,
                                                                double *field_energy_all) {
  const TreeProblem P = problems[blockIdx.x];
  const uint32_t K = P.num_spins;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t *root_sign = root_sign_all + P.row_at;
  double *field_energy = field_energy_all + P.row_at;
  if (P.has_field) {
    for (uint32_t v = tid; v < K; v += kTreeThreads) field_energy[v] = 0.0;
    __syncthreads();
    if (wave == 0) {
      // field_energy[root(v)] += (down_v ? -h_v : h_v) for v ascending; lane 0's sums are the ones stored
      uint32_t run_root = kNone;
      double run = 0.0;
      for (uint32_t base = 0; base < K; base += 64u) {
        const uint32_t v = base + lane;
        uint32_t root = 0;
        double term = 0.0;
        if (v < K) {
          const uint32_t word = root_sign[v];
          const double h = P.field[v];
          root = word & ~kFlip;
          term = (word & kFlip) ? -h : h;
        }
        const uint32_t n = K - base < 64u ? K - base : 64u;
        for (uint32_t l = 0; l < n; ++l) {
          const uint32_t r = __shfl(root, static_cast<int>(l), 64);
          const double t = __shfl(term, static_cast<int>(l), 64);
          if (r != run_root) {
            if (run_root != kNone && lane == 0) field_energy[run_root] = run;
            run_root = r;
            run = field_energy[r];
          }
          run = __dadd_rn(run, t);
        }
      }
      if (run_root != kNone && lane == 0) field_energy[run_root] = run;
    }
    __syncthreads();
  }
  const uint32_t words = (K + 63u) / 64u;
  for (uint32_t word_at = wave; word_at < words; word_at += kTreeThreads / 64) {
    const uint32_t v = word_at * 64u + lane;
    bool up = false;
    if (v < K) {
      const uint32_t word = root_sign[v];
      bool down = (word & kFlip) != 0u;
      if (P.has_field && field_energy[word & ~kFlip] > 0.0) down = !down;
      up = !down;
    }
    const uint64_t bits = __ballot(up);
    if (lane == 0) P.out[word_at] = bits;
  }
}

thread_local float g_tree_ms = 0.0f;
thread_local float g_tree_split_ms[3] = {0.0f, 0.0f, 0.0f};

struct Events {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t e : ev) {
      if (e) (void)hipEventDestroy(e);
    }
  }
};

uint32_t grid_of(uint64_t n, uint32_t threads) { return static_cast<uint32_t>((n + threads - 1) / threads); }

}  // namespace

namespace asp {

bool greedy_forest_in_lds(const asp_sa_plan *p) {
  return p->greedy_tree != 2 && 8ull * p->host.num_spins + kTreeStaticLds <= p->max_lds;
}

int greedy_tree_device(const GreedyTreeTarget *targets, uint32_t count, hipStream_t s, float split_ms[3]) {
  if (split_ms) split_ms[0] = split_ms[1] = split_ms[2] = 0.0f;
  // ---- host tables: offsets of every problem's rows, bond capacity, forest placement ----
  std::vector<uint32_t> live;  // K > 0, in call order
  uint64_t total_rows = 0, capacity = 0, out_words = 0, slab_words = 0;
  size_t lds_bytes = 0;
  bool any_field = false;
  for (uint32_t t = 0; t < count; ++t) {
    const asp::SaHostLayout &L = targets[t].plan->host;
    if (L.num_spins == 0) continue;
    if (L.num_spins >= 0x7FFFFFFFull) return set_error(ASP_ERR_TOO_LARGE, "item %u: 2^31 - 1 spins or more", t);
    live.push_back(t);
    total_rows += L.num_spins;
    capacity += static_cast<uint64_t>(L.a_ptr[L.num_spins]) / 2;  // A is symmetric without a diagonal
  }
  if (live.empty()) return ASP_OK;
  if (total_rows >= 0xFFFFFFFFull || capacity >= 0xFFFFFFFFull) {
    return set_error(ASP_ERR_TOO_LARGE, "more than 2^32 - 2 rows or bonds in one call (%llu, %llu)",
                     static_cast<unsigned long long>(total_rows), static_cast<unsigned long long>(capacity));
  }
  const uint32_t n = static_cast<uint32_t>(live.size());
  std::vector<TreeProblem> h_problems(n);
  std::vector<uint32_t> h_which_lds, h_which_hbm;
  std::vector<uint64_t> slab_at(n, 0), out_at(n, 0);
  for (uint32_t k = 0; k < n; ++k) ASP_TRY(ensure_rows(targets[live[k]].plan));
  {
    uint64_t row_at = 0;
    for (uint32_t k = 0; k < n; ++k) {
      const GreedyTreeTarget &target = targets[live[k]];
      asp_sa_plan *p = target.plan;
      const asp::SaHostLayout &L = p->host;
      TreeProblem P{};
      P.row_ptr = p->cluster_row_ptr.ptr;
      P.col = p->cluster_col.ptr;
      P.val = p->cluster_val.ptr;
      P.field = p->cluster_field.ptr;
      P.num_spins = static_cast<uint32_t>(L.num_spins);
      P.row_at = static_cast<uint32_t>(row_at);
      bool field = false;
      for (const double h : L.field_pos) field = field || h != 0.0;
      P.has_field = field ? 1u : 0u;
      any_field = any_field || field;
      row_at += L.num_spins;
      if (greedy_forest_in_lds(p)) {
        h_which_lds.push_back(k);
        lds_bytes = std::max<size_t>(lds_bytes, 8ull * L.num_spins);
      } else {
        h_which_hbm.push_back(k);
        slab_at[k] = slab_words;
        slab_words += 2ull * L.num_spins;
      }
      if (!target.d_out) {
        out_at[k] = out_words;
        out_words += (L.num_spins + 63) / 64;
      }
      h_problems[k] = P;
    }
  }
  const bool batch = n > 1;
  DeviceBuffer<TreeProblem> d_problems;
  DeviceBuffer<uint32_t> d_which, d_counts, d_first_upper, d_values, d_sorted, d_bond_row, d_bond_entry;
  DeviceBuffer<uint32_t> d_bond_problem, d_problem_keys, d_problem_keys_out, d_root_sign, d_slabs;
  DeviceBuffer<int64_t> d_scan, d_scan_scratch;
  DeviceBuffer<uint64_t> d_keys, d_keys_out, d_out;
  DeviceBuffer<double> d_field_energy;
  DeviceBuffer<char> d_temp;
  std::vector<uint64_t> h_out(out_words);
  std::vector<uint32_t> h_which(h_which_lds);
  h_which.insert(h_which.end(), h_which_hbm.begin(), h_which_hbm.end());
  Events events;
  StreamFence fence(s);
  ASP_TRY(d_problems.alloc(n));
  ASP_TRY(d_which.alloc(n));
  ASP_TRY(d_counts.alloc(total_rows));
  ASP_TRY(d_first_upper.alloc(total_rows));
  ASP_TRY(d_scan.alloc(total_rows + 1));
  ASP_TRY(d_scan_scratch.alloc(scan_scratch_elems(total_rows)));
  ASP_TRY(d_root_sign.alloc(total_rows));
  ASP_TRY(d_keys.alloc(capacity));
  ASP_TRY(d_keys_out.alloc(capacity));
  ASP_TRY(d_values.alloc(capacity));
  ASP_TRY(d_sorted.alloc(capacity));
  ASP_TRY(d_bond_row.alloc(capacity));
  ASP_TRY(d_bond_entry.alloc(capacity));
  if (batch) {
    ASP_TRY(d_bond_problem.alloc(capacity));
    ASP_TRY(d_problem_keys.alloc(capacity));
    ASP_TRY(d_problem_keys_out.alloc(capacity));
  }
  if (slab_words) ASP_TRY(d_slabs.alloc(slab_words));
  if (out_words) ASP_TRY(d_out.alloc(out_words));
  if (any_field) ASP_TRY(d_field_energy.alloc(total_rows));
  for (uint32_t k = 0; k < n; ++k) {
    const GreedyTreeTarget &target = targets[live[k]];
    h_problems[k].out = target.d_out ? target.d_out : d_out.ptr + out_at[k];
    h_problems[k].forest = greedy_forest_in_lds(target.plan) ? nullptr : d_slabs.ptr + slab_at[k];
  }
  for (hipEvent_t &e : events.ev) ASP_HIP_TRY(hipEventCreate(&e));
  ASP_TRY(d_problems.upload(h_problems.data(), n, s));
  ASP_TRY(d_which.upload(h_which.data(), n, s));
  ASP_HIP_TRY(hipEventRecord(events.ev[0], s));
  // ---- stage A ----
  const uint32_t rows32 = static_cast<uint32_t>(total_rows);
  hipLaunchKernelGGL(k_greedy_bond_count, dim3(grid_of(total_rows, kRowThreads)), dim3(kRowThreads), 0, s,
                     d_problems.ptr, n, rows32, d_counts.ptr, d_first_upper.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_TRY(exclusive_scan_u32(d_counts.ptr, total_rows, d_scan.ptr, d_scan_scratch.ptr, s));
  const uint32_t *sorted = d_values.ptr;
  if (capacity != 0) {
    hipLaunchKernelGGL(k_greedy_bond_emit, dim3(grid_of(total_rows, kRowThreads)), dim3(kRowThreads), 0, s,
                       d_problems.ptr, n, rows32, d_scan.ptr, d_first_upper.ptr, capacity, d_keys.ptr, d_values.ptr,
                       d_bond_row.ptr, d_bond_entry.ptr, batch ? d_bond_problem.ptr : nullptr);
    ASP_HIP_TRY(hipGetLastError());
    // strongest first, ties in generation order: a stable sort of ~bits(|w|) (bit 63 of the key is
    // always set, |w| has no sign)
    size_t temp_bytes = 0;
    ASP_HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, d_keys.ptr, d_keys_out.ptr, d_values.ptr, d_sorted.ptr,
                                          capacity, 0, 63, s));
    ASP_TRY(d_temp.alloc(temp_bytes ? temp_bytes : 1));
    ASP_HIP_TRY(rocprim::radix_sort_pairs(d_temp.ptr, temp_bytes, d_keys.ptr, d_keys_out.ptr, d_values.ptr, d_sorted.ptr,
                                          capacity, 0, 63, s));
    sorted = d_sorted.ptr;
    if (batch) {
      // ... and, stably, by problem: every problem's bonds contiguous and still in the law's order
      unsigned bits = 1;
      while ((1ull << bits) < n) ++bits;
      hipLaunchKernelGGL(k_greedy_problem_keys, dim3(grid_of(capacity, kRowThreads)), dim3(kRowThreads), 0, s,
                         d_sorted.ptr, d_bond_problem.ptr, capacity, d_problem_keys.ptr);
      ASP_HIP_TRY(hipGetLastError());
      size_t temp2_bytes = 0;
      ASP_HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp2_bytes, d_problem_keys.ptr, d_problem_keys_out.ptr, d_sorted.ptr,
                                            d_values.ptr, capacity, 0, bits, s));
      if (temp2_bytes > temp_bytes) {
        ASP_HIP_TRY(hipStreamSynchronize(s));  // (the first sort may still read the old block)
        ASP_TRY(d_temp.alloc(temp2_bytes));
      }
      ASP_HIP_TRY(rocprim::radix_sort_pairs(d_temp.ptr, temp2_bytes, d_problem_keys.ptr, d_problem_keys_out.ptr,
                                            d_sorted.ptr, d_values.ptr, capacity, 0, bits, s));
      sorted = d_values.ptr;
    }
  }
  ASP_HIP_TRY(hipEventRecord(events.ev[1], s));
  // ---- stage B ----
  TreeArgs args{d_problems.ptr, d_which.ptr, d_scan.ptr, sorted, d_bond_row.ptr, d_bond_entry.ptr, d_root_sign.ptr,
                capacity};
  if (!h_which_lds.empty()) {
    if (lds_bytes + kTreeStaticLds > 64 * 1024) {
      ASP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_greedy_tree<false>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
    }
    hipLaunchKernelGGL(k_greedy_tree<false>, dim3(static_cast<unsigned>(h_which_lds.size())), dim3(kTreeThreads),
                       lds_bytes, s, args);
    ASP_HIP_TRY(hipGetLastError());
  }
  if (!h_which_hbm.empty()) {
    args.which = d_which.ptr + h_which_lds.size();
    hipLaunchKernelGGL(k_greedy_tree<true>, dim3(static_cast<unsigned>(h_which_hbm.size())), dim3(kTreeThreads), 0, s,
                       args);
    ASP_HIP_TRY(hipGetLastError());
  }
  ASP_HIP_TRY(hipEventRecord(events.ev[2], s));
  // ---- stage C ----
  hipLaunchKernelGGL(k_greedy_orient, dim3(n), dim3(kTreeThreads), 0, s, d_problems.ptr, d_root_sign.ptr,
                     d_field_energy.ptr);
  ASP_HIP_TRY(hipGetLastError());
  ASP_HIP_TRY(hipEventRecord(events.ev[3], s));
  if (out_words) ASP_TRY(d_out.download(h_out.data(), out_words, s));
  ASP_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < n; ++k) {
    const GreedyTreeTarget &target = targets[live[k]];
    if (target.d_out) continue;
    const uint64_t words = (target.plan->host.num_spins + 63) / 64;
    std::copy(h_out.begin() + out_at[k], h_out.begin() + out_at[k] + words, target.h_out);
  }
  if (split_ms) {
    for (int q = 0; q < 3; ++q) ASP_HIP_TRY(hipEventElapsedTime(&split_ms[q], events.ev[q], events.ev[q + 1]));
  }
  return ASP_OK;
}

}  // namespace asp

extern "C" {

int asp_sa_set_greedy_tree(asp_sa_plan *p, int where) {
  asp_clear_error();
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  p->greedy_tree = where < 0 ? 0 : (where > 2 ? 2 : where);
  return ASP_OK;
}

float asp_sa_greedy_tree_last_ms(void) { return g_tree_ms; }

int asp_sa_greedy_tree_last_split_ms(float *bonds_sort_ms, float *tree_ms, float *orient_ms) {
  if (bonds_sort_ms) *bonds_sort_ms = g_tree_split_ms[0];
  if (tree_ms) *tree_ms = g_tree_split_ms[1];
  if (orient_ms) *orient_ms = g_tree_split_ms[2];
  return ASP_OK;
}

int asp_sa_greedy_tree_batch(asp_sa_plan *const *plans, uint32_t count, uint64_t *const *out_x) {
  asp_clear_error();
  g_tree_ms = 0.0f;
  g_tree_split_ms[0] = g_tree_split_ms[1] = g_tree_split_ms[2] = 0.0f;
  if (count == 0) return ASP_OK;
  if (!plans) return asp::set_error(ASP_ERR_INVALID, "null plans");
  if (!out_x) return asp::set_error(ASP_ERR_INVALID, "null output array");
  for (uint32_t i = 0; i < count; ++i) {
    if (!plans[i]) return asp::set_error(ASP_ERR_INVALID, "item %u: null plan", i);
    if (!out_x[i]) return asp::set_error(ASP_ERR_INVALID, "item %u: null output", i);
  }
  {
    std::vector<std::pair<const asp_sa_plan *, uint32_t>> seen(count);
    for (uint32_t i = 0; i < count; ++i) seen[i] = {plans[i], i};
    std::sort(seen.begin(), seen.end());
    for (uint32_t i = 1; i < count; ++i) {
      if (seen[i].first == seen[i - 1].first) {
        return asp::set_error(ASP_ERR_INVALID, "items %u and %u share a plan", seen[i - 1].second, seen[i].second);
      }
    }
  }
  std::vector<asp::GreedyTreeTarget> targets;
  for (uint32_t i = 0; i < count; ++i) {
    if (plans[i]->host.num_spins != 0) targets.push_back(asp::GreedyTreeTarget{plans[i], nullptr, out_x[i]});
  }
  if (targets.empty()) return ASP_OK;
  ASP_TRY(asp::bind_device());
  asp::ScopedStream stream;
  ASP_TRY(stream.acquire());
  ASP_TRY(asp::greedy_tree_device(targets.data(), static_cast<uint32_t>(targets.size()), stream.stream,
                                  g_tree_split_ms));
  g_tree_ms = g_tree_split_ms[0] + g_tree_split_ms[1] + g_tree_split_ms[2];
  return ASP_OK;
}

int asp_sa_greedy_tree(asp_sa_plan *p, uint64_t *out_x) {
  asp_clear_error();
  g_tree_ms = 0.0f;
  g_tree_split_ms[0] = g_tree_split_ms[1] = g_tree_split_ms[2] = 0.0f;
  if (!p) return asp::set_error(ASP_ERR_INVALID, "null plan");
  if (!out_x) return asp::set_error(ASP_ERR_INVALID, "null output");
  return asp_sa_greedy_tree_batch(&p, 1, &out_x);
}

}  // extern "C"

namespace asp {

void greedy_tree_record_ms(const float split_ms[3], bool add) {
  if (!add) g_tree_split_ms[0] = g_tree_split_ms[1] = g_tree_split_ms[2] = 0.0f;
  for (int q = 0; q < 3; ++q) g_tree_split_ms[q] += split_ms[q];
  g_tree_ms = g_tree_split_ms[0] + g_tree_split_ms[1] + g_tree_split_ms[2];
}

}  // namespace asp
