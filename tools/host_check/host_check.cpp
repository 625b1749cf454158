// Stand-alone checker of the threaded host code: the plan build (csrc/sa_plan.cpp: build_sa_layout,
// build_row_quads, shuffled_orders) and the greedy trees (csrc/greedy.cpp).  Its own main, no HIP
// runtime call, no GPU: built plain and under the thread / address / undefined-behaviour sanitizers
// by run.sh beside it, driven by tests/test_host_threads.py.
//
//   check A  every array and scalar of SaHostLayout and RowQuads is byte-identical for 1, 3, 4, 7
//            and 64 host threads (ASP_HOST_THREADS, read on every call), and with the symmetry
//            hashes forced to say "symmetric" (the threaded exact confirmation decides alone)
//   check B  A = offdiag(J + J^T) and the diagonal sum against a sequential std::map restatement;
//            the symmetric matrix and its upper triangle give identical layouts
//   check C  the structure the header comment of sa_plan.hpp and DESIGN.md §5.1 promise: proper
//            colouring, the permutation, blocks, widths, the quad-interleaved sliced ELL, row quads
//   check D  shuffled_orders for a chunk of 33 sweeps (threaded) against 33 single calls, and each
//            order against the levelisation law of DESIGN.md §4.9
//   check E  greedy_tree_signs_many against a loop of greedy_tree_signs
//
// Prints one banner line, then "check <name> ok" per check; exits 1 at the first failed check
// (--keep-going: runs them all and exits 1 at the end if any failed).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "asp.h"
#include "greedy.hpp"
#include "sa_plan.hpp"

namespace {

bool g_keep_going = false;
int g_failures = 0;

void report(const std::string &name, const std::string &failure) {
  if (failure.empty()) {
    std::printf("check %s ok\n", name.c_str());
    std::fflush(stdout);
    return;
  }
  std::printf("check %s FAILED: %s\n", name.c_str(), failure.c_str());
  std::fflush(stdout);
  ++g_failures;
  if (!g_keep_going) std::exit(1);
}

std::string text(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
std::string text(const char *fmt, ...) {
  char buffer[512];
  va_list args;
  va_start(args, fmt);
  std::vsnprintf(buffer, sizeof buffer, fmt, args);
  va_end(args);
  return buffer;
}

uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

// ---- the fixed generator ------------------------------------------------------------------------

struct Rng {
  uint64_t state;
  explicit Rng(uint64_t seed) : state(seed) {}
  uint64_t next() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
  double weight() {  // in +-[0.25, 1.25): never zero, never cancelling by accident
    const double magnitude = 0.25 + static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0);
    return (next() & 1) ? magnitude : -magnitude;
  }
};

struct Csr {
  uint64_t n = 0;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<double> data;
  std::vector<double> field;
};

using Rows = std::vector<std::map<int32_t, double>>;

Csr to_csr(const Rows &rows, const std::vector<double> &field) {
  Csr m;
  m.n = rows.size();
  m.indptr.assign(m.n + 1, 0);
  for (uint64_t i = 0; i < m.n; ++i) {
    for (const auto &entry : rows[i]) {
      m.indices.push_back(entry.first);
      m.data.push_back(entry.second);
    }
    m.indptr[i + 1] = static_cast<int64_t>(m.indices.size());
  }
  m.field = field;
  return m;
}

// The special rows (n >= 19999 throughout).
constexpr int32_t kEmptyRow = 5;     // no entry in the row or the column
constexpr int32_t kDiagOnlyRow = 6;  // only J_66
constexpr int32_t kHubRow = 7;       // kHubDegree couplings
constexpr int kHubDegree = 300;      // more than 255
constexpr int32_t kCancelA = 10, kCancelB = 11;  // one-sided matrix: J_ab = -J_ba
constexpr int32_t kZeroA = 12, kZeroB = 13;      // stored +0.0 couplings: dropped from A
constexpr int32_t kMinusA = 14, kMinusB = 15;    // stored -0.0 couplings: dropped from A

struct Inputs {
  Csr symmetric, upper, one_sided, nudged, holed;
};

Inputs make_inputs(uint64_t n) {
  Rng rng(0xA5A5000000000000ull + n);
  // the couplings above the diagonal, mean degree about 8
  std::map<std::pair<int32_t, int32_t>, double> bonds;
  auto special = [](int32_t v) { return v == kEmptyRow || v == kDiagOnlyRow; };
  while (bonds.size() < 4 * n) {
    int32_t i = static_cast<int32_t>(rng.below(n)), j = static_cast<int32_t>(rng.below(n));
    if (i == j || special(i) || special(j)) continue;
    if (i > j) std::swap(i, j);
    if ((i == kCancelA && j == kCancelB) || (i == kZeroA && j == kZeroB) || (i == kMinusA && j == kMinusB)) continue;
    bonds.emplace(std::make_pair(i, j), rng.weight());
  }
  for (int k = 0; k < kHubDegree; ++k) {
    bonds.emplace(std::make_pair(kHubRow, static_cast<int32_t>(1000 + 61 * k)), rng.weight());
  }
  bonds[{kZeroA, kZeroB}] = 0.0;
  bonds[{kMinusA, kMinusB}] = -0.0;
  std::vector<double> diagonal(n, 0.0), field(n);
  for (uint64_t i = 0; i < n; ++i) {
    diagonal[i] = rng.weight();  // stored on the even rows
    field[i] = 0.01 * rng.weight();
  }

  Rows sym(n), upper(n), one(n);
  for (uint64_t i = 0; i < n; i += 2) {
    const int32_t d = static_cast<int32_t>(i);
    if (d == kEmptyRow) continue;
    sym[i][d] = upper[i][d] = one[i][d] = diagonal[i];
  }
  for (const auto &bond : bonds) {
    const int32_t i = bond.first.first, j = bond.first.second;
    const double w = bond.second;
    sym[i][j] = w;
    sym[j][i] = w;
    upper[i][j] = 2.0 * w;
    if (rng.next() & 1) {
      one[i][j] = w;
    } else {
      one[j][i] = w;
    }
  }
  one[kCancelA][kCancelB] = 0.75;
  one[kCancelB][kCancelA] = -0.75;

  // one mirror entry (below the diagonal) moved by one ulp / missing
  Rows nudged = sym, holed = sym;
  auto first_below = [](Rows &rows, uint64_t from) {  // first non-zero entry below the diagonal in rows from..
    for (uint64_t row = from; row < rows.size(); ++row) {
      for (auto at = rows[row].begin(); at != rows[row].end(); ++at) {
        if (at->first < static_cast<int32_t>(row) && at->second != 0.0) return std::make_pair(row, at);
      }
    }
    std::fprintf(stderr, "host_check: the generator left no entry below the diagonal\n");
    std::abort();
  };
  {
    auto found = first_below(nudged, n - n / 5);
    found.second->second = std::nextafter(found.second->second, INFINITY);
    found = first_below(holed, n - n / 7);
    holed[found.first].erase(found.second);
  }
  Inputs in;
  in.symmetric = to_csr(sym, field);
  in.upper = to_csr(upper, field);
  in.one_sided = to_csr(one, field);
  in.nudged = to_csr(nudged, field);
  in.holed = to_csr(holed, field);
  return in;
}

// ---- byte comparison of two layouts (check A) ---------------------------------------------------

template <typename T>
std::string diff_vector(const char *name, const std::vector<T> &got, const std::vector<T> &want) {
  if (got.size() != want.size()) {
    return text("%s has %zu elements, expected %zu", name, got.size(), want.size());
  }
  for (size_t i = 0; i < got.size(); ++i) {
    if (std::memcmp(&got[i], &want[i], sizeof(T)) != 0) return text("%s differs first at index %zu", name, i);
  }
  return "";
}

template <typename T>
std::string diff_scalar(const char *name, const T &got, const T &want) {
  return std::memcmp(&got, &want, sizeof(T)) == 0 ? "" : text("scalar %s differs", name);
}

#define DIFF_VECTOR(field)                                              \
  do {                                                                  \
    std::string d = diff_vector(#field, got.field, want.field);         \
    if (!d.empty()) return d;                                           \
  } while (0)
#define DIFF_SCALAR(field)                                              \
  do {                                                                  \
    std::string d = diff_scalar(#field, got.field, want.field);         \
    if (!d.empty()) return d;                                           \
  } while (0)

std::string diff_layouts(const asp::SaHostLayout &got, const asp::SaHostLayout &want) {
  DIFF_SCALAR(num_spins);
  DIFF_VECTOR(a_ptr);
  DIFF_VECTOR(a_col);
  DIFF_VECTOR(a_val);
  DIFF_SCALAR(diag_sum);
  DIFF_VECTOR(color);
  DIFF_SCALAR(num_colors);
  DIFF_SCALAR(max_degree);
  DIFF_SCALAR(num_blocks);
  DIFF_VECTOR(color_block_start);
  DIFF_VECTOR(block_width);
  DIFF_VECTOR(ell_off);
  DIFF_VECTOR(spin_of_pos);
  DIFF_VECTOR(pos_of_spin);
  DIFF_VECTOR(field_pos);
  DIFF_VECTOR(ell_col);
  DIFF_VECTOR(ell_val);
  DIFF_SCALAR(energy_scale_exp);
  DIFF_SCALAR(beta0_auto);
  DIFF_SCALAR(beta1_auto);
  return "";
}

std::string diff_quads(const asp::RowQuads &got, const asp::RowQuads &want) {
  DIFF_VECTOR(quad_ptr);
  DIFF_VECTOR(col);
  DIFF_VECTOR(val);
  DIFF_SCALAR(max_quads);
  return "";
}

// ---- the plain reference of A (check B) ---------------------------------------------------------

struct ReferenceA {
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  std::vector<double> val;
  double diag_sum = 0.0;
};

ReferenceA reference_a(const Csr &m) {
  struct Pair {
    double forward = 0.0, backward = 0.0;  // J_ij and J_ji, +0.0 where absent
  };
  std::vector<std::map<int32_t, Pair>> rows(m.n);
  ReferenceA ref;
  for (uint64_t i = 0; i < m.n; ++i) {
    for (int64_t k = m.indptr[i]; k < m.indptr[i + 1]; ++k) {
      const int32_t j = m.indices[k];
      if (static_cast<uint64_t>(j) == i) {
        ref.diag_sum = ref.diag_sum + m.data[k];
        continue;
      }
      rows[i][j].forward = m.data[k];
      rows[static_cast<size_t>(j)][static_cast<int32_t>(i)].backward = m.data[k];
    }
  }
  ref.ptr.assign(1, 0);
  for (uint64_t i = 0; i < m.n; ++i) {
    for (const auto &entry : rows[i]) {
      const double v = entry.second.forward + entry.second.backward;
      if (v == 0.0) continue;
      ref.col.push_back(entry.first);
      ref.val.push_back(v);
    }
    ref.ptr.push_back(static_cast<int64_t>(ref.col.size()));
  }
  return ref;
}

std::string diff_reference(const asp::SaHostLayout &got, const ReferenceA &want) {
  std::string d = diff_vector("a_ptr", got.a_ptr, want.ptr);
  if (d.empty()) d = diff_vector("a_col", got.a_col, want.col);
  if (d.empty()) d = diff_vector("a_val", got.a_val, want.val);
  if (d.empty()) d = diff_scalar("diag_sum", got.diag_sum, want.diag_sum);
  return d;
}

// ---- structure (check C) ------------------------------------------------------------------------

#define REQUIRE(cond, ...)                  \
  do {                                      \
    if (!(cond)) return text(__VA_ARGS__);  \
  } while (0)

std::string check_structure(const asp::SaHostLayout &L, const Csr &m) {
  const uint64_t n = m.n;
  REQUIRE(L.num_spins == n && L.a_ptr.size() == n + 1 && L.color.size() == n && L.pos_of_spin.size() == n,
          "sizes of the per-spin arrays");
  auto degree = [&](uint64_t i) { return static_cast<uint32_t>(L.a_ptr[i + 1] - L.a_ptr[i]); };
  // A: sorted columns, no diagonal, no zero, symmetric pattern is not required here (B pins A)
  uint32_t max_degree = 0;
  int32_t max_color = -1;
  for (uint64_t i = 0; i < n; ++i) {
    max_degree = std::max(max_degree, degree(i));
    REQUIRE(L.color[i] >= 0, "spin %llu has no colour", (unsigned long long)i);
    max_color = std::max(max_color, L.color[i]);
    for (int64_t k = L.a_ptr[i]; k < L.a_ptr[i + 1]; ++k) {
      const int32_t j = L.a_col[k];
      REQUIRE(j >= 0 && static_cast<uint64_t>(j) < n && static_cast<uint64_t>(j) != i, "A row %llu: bad column",
              (unsigned long long)i);
      REQUIRE(k == L.a_ptr[i] || L.a_col[k - 1] < j, "A row %llu: columns not ascending", (unsigned long long)i);
      REQUIRE(L.a_val[k] != 0.0, "A row %llu holds a zero", (unsigned long long)i);
      REQUIRE(L.color[static_cast<size_t>(j)] != L.color[i], "colouring: neighbours %llu and %d share colour %d",
              (unsigned long long)i, j, L.color[i]);
    }
  }
  REQUIRE(L.max_degree == max_degree, "max_degree %u, rows say %u", L.max_degree, max_degree);
  REQUIRE(static_cast<int64_t>(L.num_colors) == static_cast<int64_t>(max_color) + 1, "num_colors");
  // permutation
  const uint64_t positions = static_cast<uint64_t>(L.num_blocks) * 64;
  REQUIRE(L.spin_of_pos.size() == positions && L.field_pos.size() == positions, "sizes of the per-position arrays");
  uint64_t real = 0;
  for (uint64_t pos = 0; pos < positions; ++pos) {
    const uint32_t spin = L.spin_of_pos[pos];
    if (spin == asp::kDummySpin) {
      REQUIRE(bits_of(L.field_pos[pos]) == 0, "padding lane %llu has a field", (unsigned long long)pos);
      continue;
    }
    ++real;
    REQUIRE(spin < n && L.pos_of_spin[spin] == pos, "spin_of_pos / pos_of_spin disagree at position %llu",
            (unsigned long long)pos);
    REQUIRE(bits_of(L.field_pos[pos]) == bits_of(m.field[spin]), "field at position %llu", (unsigned long long)pos);
  }
  REQUIRE(real == n, "%llu real lanes for %llu spins", (unsigned long long)real, (unsigned long long)n);
  for (uint64_t i = 0; i < n; ++i) {
    REQUIRE(L.pos_of_spin[i] < positions && L.spin_of_pos[L.pos_of_spin[i]] == i,
            "pos_of_spin / spin_of_pos disagree at spin %llu", (unsigned long long)i);
  }
  // blocks: one colour each, a colour class is a run of blocks in (degree desc, index asc) order,
  // padding lanes only at the end of its last block; widths
  REQUIRE(L.color_block_start.size() == static_cast<size_t>(L.num_colors) + 1 && L.color_block_start[0] == 0 &&
              L.color_block_start[L.num_colors] == L.num_blocks,
          "color_block_start ends");
  REQUIRE(L.block_width.size() == L.num_blocks && L.ell_off.size() == static_cast<size_t>(L.num_blocks) + 1 &&
              L.ell_off[0] == 0,
          "sizes of the per-block arrays");
  for (uint32_t c = 0; c < L.num_colors; ++c) {
    REQUIRE(L.color_block_start[c] < L.color_block_start[c + 1], "colour %u has no block", c);
    bool ended = false;
    uint32_t previous = asp::kDummySpin;
    for (uint32_t b = L.color_block_start[c]; b < L.color_block_start[c + 1]; ++b) {
      uint32_t widest = 0;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t spin = L.spin_of_pos[b * 64ull + lane];
        if (spin == asp::kDummySpin) {
          ended = true;
          continue;
        }
        REQUIRE(!ended, "block %u: a spin after a padding lane", b);
        REQUIRE(static_cast<uint32_t>(L.color[spin]) == c, "block %u of colour %u holds spin %u of colour %d", b, c,
                spin, L.color[spin]);
        if (previous != asp::kDummySpin) {
          REQUIRE(degree(previous) > degree(spin) || (degree(previous) == degree(spin) && previous < spin),
                  "block %u: spins %u, %u out of (degree desc, index asc) order", b, previous, spin);
        }
        previous = spin;
        widest = std::max(widest, degree(spin));
      }
      REQUIRE(L.spin_of_pos[b * 64ull] != asp::kDummySpin, "block %u is all padding", b);
      REQUIRE(L.block_width[b] % 4 == 0 && L.block_width[b] >= widest && L.block_width[b] < widest + 4,
              "block %u: width %u for a longest row of %u", b, L.block_width[b], widest);
      REQUIRE(L.ell_off[b + 1] == L.ell_off[b] + L.block_width[b], "ell_off[%u]", b + 1);
    }
  }
  // sliced ELL through the slot formula of DESIGN.md §5.1: entries k = 4Q .. 4Q+3 of a lane are
  //   ell_col[(Q*64 + lane)*4 + j],  ell_val[((2Q + h)*64 + lane)*2 + j'],  k = 4q + j = 4q + 2h + j',
  //   Q = ell_off[b]/4 + q
  const uint64_t slabs = L.ell_off[L.num_blocks];
  const uint64_t total = (slabs + asp::kEllTailSlabs) * 64;
  REQUIRE(L.ell_col.size() == total && L.ell_val.size() == total, "ELL arrays hold %zu / %zu entries, expected %llu",
          L.ell_col.size(), L.ell_val.size(), (unsigned long long)total);
  for (uint32_t b = 0; b < L.num_blocks; ++b) {
    REQUIRE(L.ell_off[b] % 4 == 0, "ell_off[%u] is no multiple of 4", b);
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t pos = b * 64u + lane;
      const uint32_t spin = L.spin_of_pos[pos];
      const uint32_t deg = spin == asp::kDummySpin ? 0 : degree(spin);
      for (uint32_t k = 0; k < L.block_width[b]; ++k) {
        const uint64_t Q = L.ell_off[b] / 4 + k / 4;
        const uint32_t j = k % 4, h = (k % 4) / 2, jj = k % 2;
        const uint32_t col = L.ell_col[(Q * 64 + lane) * 4 + j];
        const double val = L.ell_val[((2 * Q + h) * 64 + lane) * 2 + jj];
        if (k < deg) {
          const int64_t at = L.a_ptr[spin] + k;
          REQUIRE(col == L.pos_of_spin[static_cast<size_t>(L.a_col[at])] && bits_of(val) == bits_of(L.a_val[at]),
                  "ELL row of spin %u, entry %u is not entry %u of its row of A", spin, k, k);
        } else {
          REQUIRE(col == pos && bits_of(val) == 0, "ELL padding of position %u, entry %u", pos, k);
        }
      }
    }
  }
  for (uint64_t at = slabs * 64; at < total; ++at) {
    REQUIRE(L.ell_col[at] == 0 && bits_of(L.ell_val[at]) == 0, "tail slabs not zero at %llu", (unsigned long long)at);
  }
  return "";
}

std::string check_row_quads(const asp::RowQuads &R, const asp::SaHostLayout &L) {
  const uint64_t n = L.num_spins;
  REQUIRE(R.quad_ptr.size() == n + 1 && R.quad_ptr[0] == 0, "quad_ptr size");
  uint32_t longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t deg = static_cast<uint64_t>(L.a_ptr[i + 1] - L.a_ptr[i]);
    const uint32_t quads = R.quad_ptr[i + 1] - R.quad_ptr[i];
    REQUIRE(quads == (deg + 3) / 4, "row %llu has %u quads for %llu entries", (unsigned long long)i, quads,
            (unsigned long long)deg);
    longest = std::max(longest, quads);
  }
  REQUIRE(R.max_quads == longest, "max_quads");
  REQUIRE(R.col.size() == 4ull * R.quad_ptr[n] && R.val.size() == R.col.size(), "sizes of col / val");
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t deg = static_cast<uint64_t>(L.a_ptr[i + 1] - L.a_ptr[i]);
    for (uint64_t k = 0; k < 4ull * (R.quad_ptr[i + 1] - R.quad_ptr[i]); ++k) {
      const uint64_t at = (R.quad_ptr[i] + k / 4) * 4 + k % 4;
      if (k < deg) {
        REQUIRE(R.col[at] == static_cast<uint32_t>(L.a_col[L.a_ptr[i] + k]) &&
                    bits_of(R.val[at]) == bits_of(L.a_val[L.a_ptr[i] + k]),
                "row quads of spin %llu, entry %llu", (unsigned long long)i, (unsigned long long)k);
      } else {
        REQUIRE(R.col[at] == i && bits_of(R.val[at]) == 0, "row-quad padding of spin %llu", (unsigned long long)i);
      }
    }
  }
  return "";
}

// ---- shuffled orders (check D) ------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., SC 2011), word 0 of the output block.
uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {c0, c1, c2, c3};
  for (int round = 0; round < 10; ++round) {
    const uint64_t lo = 0xD2511F53ull * c[0], hi = 0xCD9E8D57ull * c[2];
    const uint32_t next[4] = {static_cast<uint32_t>(hi >> 32) ^ c[1] ^ k0, static_cast<uint32_t>(hi),
                              static_cast<uint32_t>(lo >> 32) ^ c[3] ^ k1, static_cast<uint32_t>(lo)};
    std::memcpy(c, next, sizeof c);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c[0];
}

// One sweep's order against the law: level(i) = 1 + max level of the neighbours that come before i
// in (priority, index); a level's spins pairwise non-adjacent and in ascending (priority, index).
std::string check_levelisation(const asp::SaHostLayout &L, uint64_t seed, uint32_t sweep, const uint32_t *order,
                               const uint32_t *starts, uint32_t levels) {
  const uint64_t K = L.num_spins;
  REQUIRE(starts[0] == 0 && starts[levels] == K, "sweep %u: level_start ends", sweep);
  std::vector<uint64_t> key(K);
  for (uint64_t i = 0; i < K; ++i) {
    key[i] = (static_cast<uint64_t>(philox4x32_10_word0(static_cast<uint32_t>(i), sweep, 0xFFFFFFFEu, 0u,
                                                        static_cast<uint32_t>(seed),
                                                        static_cast<uint32_t>(seed >> 32)))
              << 32) | i;
  }
  std::vector<uint32_t> level(K, 0);  // 1-based; 0 = not seen
  for (uint32_t l = 0; l < levels; ++l) {
    REQUIRE(starts[l] < starts[l + 1], "sweep %u: level %u is empty", sweep, l);
    for (uint32_t q = starts[l]; q < starts[l + 1]; ++q) {
      const uint32_t i = order[q];
      REQUIRE(i < K && level[i] == 0, "sweep %u: position %u repeats or exceeds the spins", sweep, q);
      level[i] = l + 1;
      REQUIRE(q == starts[l] || key[order[q - 1]] < key[i], "sweep %u: level %u not in ascending (priority, index)",
              sweep, l);
    }
  }
  for (uint64_t i = 0; i < K; ++i) {
    uint32_t above = 0;
    for (int64_t k = L.a_ptr[i]; k < L.a_ptr[i + 1]; ++k) {
      const size_t j = static_cast<size_t>(L.a_col[k]);
      REQUIRE(level[j] != level[i], "sweep %u: neighbours %llu and %zu share level %u", sweep, (unsigned long long)i,
              j, level[i]);
      if (key[j] < key[i]) above = std::max(above, level[j]);
    }
    REQUIRE(level[i] == above + 1, "sweep %u: spin %llu is on level %u, the law says %u", sweep,
            (unsigned long long)i, level[i], above + 1);
  }
  return "";
}

std::string check_shuffled(const asp::SaHostLayout &L) {
  const uint64_t K = L.num_spins;
  const uint64_t seed = 0x123456789ABCDEFull;  // both key words in use
  const uint32_t first = 7, count = 33;
  std::vector<uint32_t> order(count * K), levels(count, 0), starts;
  uint32_t cap = 0;
  asp::shuffled_orders(L, seed, first, count, order.data(), &starts, &cap, levels.data());
  uint32_t deepest = 0;
  for (uint32_t s = 0; s < count; ++s) deepest = std::max(deepest, levels[s]);
  REQUIRE(cap == deepest + 1 && starts.size() == static_cast<size_t>(count) * cap, "cap %u for %u levels", cap, deepest);
  std::vector<uint32_t> one(K), one_starts;
  for (uint32_t s = 0; s < count; ++s) {
    uint32_t one_cap = 0, one_levels = 0;
    asp::shuffled_orders(L, seed, first + s, 1, one.data(), &one_starts, &one_cap, &one_levels);
    REQUIRE(one_levels == levels[s] && one_cap == one_levels + 1, "sweep %u: %u levels in the chunk, %u alone",
            first + s, levels[s], one_levels);
    REQUIRE(std::memcmp(one.data(), order.data() + s * K, K * sizeof(uint32_t)) == 0,
            "sweep %u: the chunk's order differs from the single call's", first + s);
    for (uint32_t l = 0; l < cap; ++l) {
      const uint32_t want = l <= one_levels ? one_starts[l] : static_cast<uint32_t>(K);
      REQUIRE(starts[static_cast<size_t>(s) * cap + l] == want, "sweep %u: level_start[%u]", first + s, l);
    }
    std::string d = check_levelisation(L, seed, first + s, order.data() + s * K, starts.data() + static_cast<size_t>(s) * cap,
                                       levels[s]);
    if (!d.empty()) return d;
  }
  return "";
}

// ---- greedy trees (check E) ---------------------------------------------------------------------

Csr small_problem(uint64_t n, uint64_t seed, bool one_sided) {
  Rng rng(seed);
  Rows rows(n);
  std::vector<double> field(n);
  for (uint64_t i = 0; i < n; ++i) field[i] = (i % 3 == 0) ? 0.0 : 0.05 * rng.weight();
  const uint64_t bonds = n < 2 ? 0 : 3 * n;
  for (uint64_t b = 0; b < bonds; ++b) {
    const int32_t i = static_cast<int32_t>(rng.below(n)), j = static_cast<int32_t>(rng.below(n));
    if (i == j || rows[i].count(j) || rows[j].count(i)) continue;
    // a few repeated magnitudes: ties in the bond order
    const double w = (b % 5 == 0) ? ((rng.next() & 1) ? 0.5 : -0.5) : rng.weight();
    rows[i][j] = w;
    if (!one_sided) rows[j][i] = w;
  }
  return to_csr(rows, field);
}

std::string build(const Csr &m, asp::SaHostLayout *out) {
  const int rc = asp::build_sa_layout(m.n, m.indptr.data(), m.indices.data(), m.data.data(), m.field.data(), out);
  return rc == ASP_OK ? "" : text("build_sa_layout returned %d: %s", rc, asp_last_error());
}

std::string check_greedy(const std::vector<const asp::SaHostLayout *> &layouts) {
  constexpr uint64_t kGuard = 0xDEADBEEFCAFEF00Dull;
  std::vector<std::vector<uint64_t>> many(layouts.size()), single(layouts.size());
  std::vector<uint64_t *> out(layouts.size());
  for (size_t p = 0; p < layouts.size(); ++p) {
    const size_t words = (layouts[p]->num_spins + 63) / 64;
    many[p].assign(words + 1, kGuard);  // one word more than the problem owns
    single[p].assign(words + 1, kGuard);
    out[p] = many[p].data();
  }
  asp::greedy_tree_signs_many(layouts.data(), out.data(), layouts.size());
  for (size_t p = 0; p < layouts.size(); ++p) {
    const size_t words = (layouts[p]->num_spins + 63) / 64;
    REQUIRE(asp::greedy_tree_signs(*layouts[p], single[p].data()) == ASP_OK, "greedy_tree_signs failed");
    REQUIRE(many[p][words] == kGuard && single[p][words] == kGuard, "problem %zu: written past its words", p);
    for (size_t w = 0; w < words; ++w) {
      REQUIRE(many[p][w] == single[p][w], "problem %zu (%llu spins): word %zu differs", p,
              (unsigned long long)layouts[p]->num_spins, w);
    }
    if (layouts[p]->num_spins % 64) {
      REQUIRE((single[p][words - 1] >> (layouts[p]->num_spins % 64)) == 0, "problem %zu: bits beyond the spins", p);
    }
  }
  return "";
}

void set_threads(unsigned threads) {
  if (threads == 0) {
    unsetenv("ASP_HOST_THREADS");
  } else {
    setenv("ASP_HOST_THREADS", std::to_string(threads).c_str(), 1);
  }
}

}  // namespace

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    if (std::strcmp(argv[a], "--keep-going") == 0) {
      g_keep_going = true;
    } else {
      std::fprintf(stderr, "usage: %s [--keep-going]\n", argv[0]);
      return 2;
    }
  }
  std::printf("host_check: plan build, shuffled orders and greedy trees on host threads (%u hardware threads)\n",
              std::thread::hardware_concurrency());
  std::fflush(stdout);

  const uint64_t sizes[] = {19999, 20000, 20011};
  const unsigned thread_counts[] = {3, 4, 7, 64};
  std::vector<asp::SaHostLayout> kept;  // for check E
  kept.reserve(8);
  for (const uint64_t n : sizes) {
    const Inputs in = make_inputs(n);
    const std::pair<const char *, const Csr *> forms[] = {{"symmetric", &in.symmetric},
                                                          {"upper", &in.upper},
                                                          {"one_sided", &in.one_sided},
                                                          {"nudged", &in.nudged},
                                                          {"holed", &in.holed}};
    asp::SaHostLayout symmetric_layout;
    for (const auto &form : forms) {
      const Csr &m = *form.second;
      const std::string tag = text("%s/%llu", form.first, (unsigned long long)n);
      const ReferenceA ref = reference_a(m);
      asp::SaHostLayout base, threaded;
      asp::RowQuads base_quads, quads;
      set_threads(1);
      std::string failure = build(m, &base);
      if (failure.empty() && asp::build_row_quads(base, &base_quads) != ASP_OK) failure = "build_row_quads failed";
      if (failure.empty()) failure = diff_reference(base, ref);
      report("B.reference/1-thread/" + tag, failure);
      for (const unsigned threads : thread_counts) {
        set_threads(threads);
        failure = build(m, &threaded);
        if (failure.empty() && asp::build_row_quads(threaded, &quads) != ASP_OK) failure = "build_row_quads failed";
        // B before A: a wrong merge is named as such, not only as "differs from one thread"
        report(text("B.reference/%u-threads/", threads) + tag, failure.empty() ? diff_reference(threaded, ref) : failure);
        failure = diff_layouts(threaded, base);
        if (failure.empty()) failure = diff_quads(quads, base_quads);
        report(text("A.threads/%u/", threads) + tag, failure);
        if (threads == 3) {
          failure = check_structure(threaded, m);
          if (failure.empty()) failure = check_row_quads(quads, threaded);
          report("C.structure/3-threads/" + tag, failure);
        }
      }
      // the hashes say "symmetric" whatever the matrix: the threaded exact confirmation alone sends
      // everything but the symmetric matrix through the general merge
      setenv("ASP_PLAN_HASHES_SAY_SYMMETRIC", "1", 1);
      set_threads(7);
      failure = build(m, &threaded);
      unsetenv("ASP_PLAN_HASHES_SAY_SYMMETRIC");
      report("A.confirmation/7/" + tag, failure.empty() ? diff_layouts(threaded, base) : failure);
      set_threads(0);  // the default: four threads
      failure = build(m, &threaded);
      report("A.threads/default/" + tag, failure.empty() ? diff_layouts(threaded, base) : failure);

      if (form.second == &in.symmetric) symmetric_layout = base;
      if (form.second == &in.upper) {
        report("B.upper-equals-symmetric/" + tag, diff_layouts(base, symmetric_layout));
      }
      if (form.second == &in.symmetric || form.second == &in.one_sided) {
        report("D.shuffled/" + tag, check_shuffled(base));
        kept.push_back(base);
      }
    }
  }

  // check E: 40 layouts, two of 0 spins and two of 1 spin among them, the large ones not first
  {
    const uint64_t small_sizes[] = {0, 1, 2, 3, 63, 64, 65, 130, 0, 500, 1, 1000, 257, 3000, 31, 4097, 700,
                                    128, 5, 2000, 90, 640, 33, 1500, 17, 8, 300, 1025, 77, 4000, 129, 66, 250, 12};
    std::vector<asp::SaHostLayout> small(sizeof small_sizes / sizeof small_sizes[0]);
    std::vector<const asp::SaHostLayout *> layouts;
    std::string failure;
    for (size_t p = 0; p < small.size() && failure.empty(); ++p) {
      failure = build(small_problem(small_sizes[p], 1000 + p, p % 4 == 3), &small[p]);
      layouts.push_back(&small[p]);
    }
    for (size_t p = 0; p < kept.size(); ++p) layouts.insert(layouts.begin() + 5 * (p + 1), &kept[p]);
    if (failure.empty() && layouts.size() != 40) failure = text("%zu layouts, not 40", layouts.size());
    report("E.greedy-many/40-layouts", failure.empty() ? check_greedy(layouts) : failure);
  }

  if (g_failures) {
    std::printf("host_check: %d checks FAILED\n", g_failures);
    return 1;
  }
  std::printf("host_check: all checks ok\n");
  return 0;
}
