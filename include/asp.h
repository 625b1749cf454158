/* asp.h — C ABI of libasp_hip.so, the MI355X (gfx950) implementation of the
 * sign-optimisation hot path of twesterhout/annealing-sign-problem.
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  Every entry point
 * names the reference interface it replaces (paths relative to the reference
 * checkout).  Unless a function says "device", pointers are HOST pointers and
 * the callee stages them through HBM itself.
 *
 * Error model: the two drop-in symbols keep the reference's signatures (no
 * error return, cbits/build_matrix.h:7-14); every failure — no GPU, HIP error,
 * violated precondition that was detected — is recorded and can be read with
 * asp_last_error().  All other functions return 0 on success and a negative
 * asp_status otherwise.  Nothing in this library falls back to a CPU path.
 */
#ifndef ASP_H
#define ASP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Status / errors                                                           */
/* ------------------------------------------------------------------------- */

typedef enum asp_status {
  ASP_OK = 0,
  ASP_ERR_NO_DEVICE = -1,  /* no HIP device visible                          */
  ASP_ERR_HIP = -2,        /* a HIP runtime call failed                      */
  ASP_ERR_INVALID = -3,    /* invalid argument / violated precondition       */
  ASP_ERR_TOO_LARGE = -4,  /* problem does not fit this implementation       */
  ASP_ERR_ALLOC = -5       /* host or device allocation failed               */
} asp_status;

/* Last error recorded on the calling thread ("" if none). */
const char *asp_last_error(void);
int asp_last_error_code(void);
void asp_clear_error(void);

/* Number of HIP devices (>= 0) or a negative asp_status. */
int asp_device_count(void);
/* 1 once this process has made a HIP call THROUGH THIS LIBRARY (any entry point that needs the
 * device), 0 before.  It knows nothing of HIP state created elsewhere in the process (a
 * profiler's preloaded tool library, the host's own HIP or torch.cuda calls): 0 means "not by
 * this library", and only a process whose GPU is untouched by anybody may fork workers that each
 * open the device (sampled_components --workers checks both). */
int asp_device_touched(void);
/* Select the device used by this library in the whole process (every entry point binds
 * its calling thread to it). */
int asp_set_device(int device);
/* The device this library computes on: the asp_set_device choice, else HIP's current device
 * of the calling thread; negative asp_status on failure. */
int asp_get_device(void);
/* Waits for the device(s) and releases what the library keeps alive BETWEEN calls: pooled
 * device memory and pooled streams.  Meant to be called once, after every handle (plans,
 * operators, builds) has been destroyed and before the process starts to exit, so that no HIP
 * call is left to static destructors or interpreter teardown, where the runtime or a profiler
 * attached to it may already be gone (the Python binding registers it with atexit and
 * destroys its live handles first).  The library stays usable afterwards, without pooling. */
int asp_shutdown(void);
/* Library version, "major.minor.patch". */
const char *asp_version(void);

/* ------------------------------------------------------------------------- */
/* (1) Drop-in replacements for cbits/build_matrix.h:3-14                    */
/*     (cffi cdef duplicate: annealing_sign_problem/build_extension.py:5-20) */
/* ------------------------------------------------------------------------- */

typedef struct ls_bits512 {
  uint64_t words[8];
} ls_bits512;

/* Replaces build_matrix (cbits/build_matrix.c:22-65).
 *
 * For every row r and each of its other_counts[r] connections e (flat,
 * row-major): look other_spins[e] up in the table spins[0..num_spins), which
 * is sorted ascending under the lexicographic order of words[0..7]
 * (cbits/build_matrix.c:7-20) and unique.
 *   hit  -> append (r, position, counts[r]*other_coeffs[e]*|psi[r]|*|other_psi[e]|)
 *           to (row_indices, col_indices, elements), preserving input order;
 *   miss -> field[r] += counts[r]*other_coeffs[e]*|psi[r]|*other_psi[e]
 *           (signed other_psi, left-to-right accumulation in row order).
 * Products are evaluated left to right without FMA contraction, so results are
 * bit-identical to the reference compiled without -ffast-math.
 * Caller allocates all outputs (capacity sum(other_counts) for the COO triple,
 * num_spins for field).  Returns the number of COO entries written; on failure
 * returns 0, leaves outputs untouched and records an error.
 */
uint64_t build_matrix(uint64_t num_spins, ls_bits512 const spins[],
                      int64_t const *counts, double const *psi,
                      ls_bits512 const *other_spins, double const *other_coeffs,
                      int64_t const *other_counts, double const *other_psi,
                      uint32_t *row_indices, uint32_t *col_indices,
                      double *elements, double *field);

/* Replaces extract_signs (cbits/build_matrix.c:67-76): bit i of signs[i/64]
 * is set iff psi[i] > 0 (zero and NaN clear it); ceil(num_spins/64) words are
 * fully overwritten. */
void extract_signs(uint64_t num_spins, double const *psi, uint64_t *signs);

/* ------------------------------------------------------------------------- */
/* (2) Device-resident form of the same coupling build (what bench.py times) */
/* ------------------------------------------------------------------------- */

typedef struct asp_build asp_build;

/* Allocate HBM for a build with num_spins rows and num_other = sum(other_counts)
 * connections.  NULL on failure. */
asp_build *asp_build_create(uint64_t num_spins, uint64_t num_other);
/* Host -> HBM copy of the seven input arrays of build_matrix. */
int asp_build_upload(asp_build *b, ls_bits512 const *spins, int64_t const *counts,
                     double const *psi, ls_bits512 const *other_spins,
                     double const *other_coeffs, int64_t const *other_counts,
                     double const *other_psi);
/* Run the kernels on resident inputs; *nnz receives the COO length.  The
 * device time of the launch sequence is measured with HIP events on the
 * library's stream and returned by asp_build_last_ms(). */
int asp_build_run(asp_build *b, uint64_t *nnz);
float asp_build_last_ms(asp_build const *b);
/* HBM -> host copy of the outputs of the last run (any pointer may be NULL). */
int asp_build_download(asp_build *b, uint32_t *row_indices, uint32_t *col_indices,
                       double *elements, double *field);
void asp_build_destroy(asp_build *b);

/* ------------------------------------------------------------------------- */
/* (3) Live coupling build: the two numba kernels of common.make_ising_model */
/* ------------------------------------------------------------------------- */

/* Replaces _clipped_search_sorted (annealing_sign_problem/common.py:116-128)
 * fused with the membership test (common.py:173) and
 * _make_ising_model_compute_elements (common.py:71-82), for 64-bit keys
 * (number_spins <= 64, asserted by the reference at common.py:86).
 *
 *   other_indices[e] = clip(searchsorted_left(keys, other_keys[e]), 0, K-1)
 *   member[e]        = other_keys[e] == keys[other_indices[e]]
 *   elements[e]      = (other_coeffs[e] * |member ? psi[idx] : 0|) * |psi[row(e)]|
 *   offsets          = [0, cumsum(other_counts)]
 * keys must be sorted ascending (np.unique output).  Any output may be NULL.
 */
int asp_ising_elements(uint64_t num_spins, uint64_t const *keys, double const *psi,
                       uint64_t num_other, uint64_t const *other_keys,
                       double const *other_coeffs, int64_t const *other_counts,
                       int64_t *other_indices, uint8_t *member, double *elements,
                       int64_t *offsets);

/* Device time (ms, HIP events) of the scan + kernel of this thread's last
 * asp_ising_elements call, without the host<->HBM copies. */
float asp_ising_elements_last_ms(void);

/* ------------------------------------------------------------------------- */
/* (3b) Hamiltonian action on bit-packed basis states, and the coupling      */
/*      build fused with it                                                  */
/* ------------------------------------------------------------------------- */

/* A sum of two-site terms on <= 64 spin-1/2 sites without lattice symmetries:
 * what the reference obtains from lattice_symmetries' ls.Operator built from
 * physical_systems/<model>.yaml (`terms: [{matrix, sites}]`, e.g.
 * heisenberg_kagome_16.yaml:5-12; call sites annealing_sign_problem/common.py:96,
 * 283,516-522).  Bit i of a key is site i; a 4x4 matrix acts on |b_a b_b> with
 * row/column index 2*b_a + b_b, `matrices[bond*16 + dst*4 + src]`.  Bonds are
 * listed in term order, then site-pair order.  Matrices are real (the reference
 * rejects |Im| > 1e-6, common.py:99-101). */
typedef struct asp_operator asp_operator;

int asp_operator_create(uint32_t number_spins, uint32_t num_bonds, uint8_t const *site_a,
                        uint8_t const *site_b, double const *matrices, asp_operator **out);
void asp_operator_destroy(asp_operator *op);

/* Symmetry-adapted basis in the trivial sector of a group of site permutations, with optional
 * global spin inversion of character spin_inversion = +1 / -1 (0: none) — the bases of
 * physical_systems/heisenberg_kagome_36.yaml:7-29, heisenberg_pyrochlore_2x2x2.yaml:1-17 and
 * heisenberg_kagome_18.yaml:4, which the reference gets from lattice_symmetries.
 * table[e * 64 + i] = destination site of site i under element e, for ALL elements of the group
 * (closed under composition; element 0 the identity).  Afterwards keys are orbit representatives
 * (the smallest state of an orbit), asp_operator_apply returns for every connection the
 * representative of the target and the coefficient c * chi(g) * norm(target) / norm(source),
 * norm(s)^2 = (sum of the stabiliser's characters) / |G|, and asp_operator_extend the sorted
 * unique representatives.  Equal targets within a row are not merged (asp_operator_ising
 * then runs its duplicate-keeping variant).
 * The character of a state is that of inversion iff its smallest flipped image lies strictly below
 * its smallest plain image (SymmetryGroup.state_info's rule).  With spin_inversion = -1 an orbit
 * whose stabiliser holds an element of character -1 has norm 0 and is no basis state: as a KEY it
 * makes asp_operator_apply, asp_operator_ising, asp_operator_ising_csr and asp_operator_extend
 * fail with ASP_ERR_INVALID (the message names the sector; outputs are unspecified then); as a
 * TARGET it stays in asp_operator_apply's output with its representative and coefficient exactly
 * 0, and is left out of asp_operator_extend's set. */
int asp_operator_set_symmetry(asp_operator *op, uint32_t num_permutations, uint8_t const *table,
                              int32_t spin_inversion);
/* (representative, character of a group element mapping the key onto it, norm) of n keys; any
 * output may be NULL.  norm 0: the key's orbit is not part of the sector. */
int asp_operator_state_info(asp_operator const *op, uint64_t n, uint64_t const *keys,
                            uint64_t *representatives, double *characters, double *norms);

/* y = H x, matrix-free, in a fixed-magnetisation basis without lattice symmetries
 * (csrc/plain_basis.hip): sk_32_1.yaml's C(32,16) = 6.0e8 states x 496 bonds are too many matrix
 * elements to keep resident (asp_sector_rows) but have a closed-form index.  States ascending;
 * asp_plain_basis_states writes them (device pointer, `dimension` entries).  Bonds must conserve
 * the magnetisation (off-diagonal weight on 01 <-> 10 only); 2..36 spins. */
typedef struct asp_plain_basis asp_plain_basis;
int asp_plain_basis_create(asp_operator const *op, int32_t hamming_weight, asp_plain_basis **out);
void asp_plain_basis_destroy(asp_plain_basis *pb);
uint64_t asp_plain_basis_dimension(asp_plain_basis const *pb);
int asp_plain_basis_states(asp_plain_basis const *pb, uint64_t *states_dev);
int asp_plain_matvec(asp_plain_basis const *pb, double const *x_dev, double *y_dev);

/* Positions of states in a long ascending list kept on the device (csrc/key_table.hip): what
 * `basis.batched_index(spins)` (common.py:813-818) is for a basis of tens of millions of
 * representatives.  index[q] = position of queries[q], or -1.  Host pointers; thread-safe. */
typedef struct asp_table asp_table;
int asp_table_create(uint64_t n, uint64_t const *sorted_keys, asp_table **out);
void asp_table_destroy(asp_table *t);
int asp_table_index(asp_table const *t, uint64_t m, uint64_t const *queries, int64_t *index);

/* A whole symmetry sector on the device (csrc/sector_basis.hip) — what the reference reads from
 * SpinED's output (common.py:783-803: /basis/representatives, /hamiltonian/eigenvectors) and
 * what those absent files would hold for heisenberg_kagome_36.yaml: 31.5 million representatives.
 * Every *_dev pointer is DEVICE memory of the bound device; the calls run on a stream of their
 * own and return when the work is done (the caller synchronises ITS streams before calling).
 *
 * asp_sector_enumerate: all states of `number_spins` spins with `hamming_weight` bits set (all
 * states when negative) that are the smallest member of their orbit and lie in the sector
 * (norm > 0), ascending, with their norms (norms_dev may be NULL).  *count receives the number
 * found; nothing is written when it exceeds `capacity` (capacity 0: sizing call), which then
 * fails with ASP_ERR_TOO_LARGE.  Up to 48 spins; works without symmetries too (every state its
 * own representative, norm 1). */
int asp_sector_enumerate(asp_operator const *op, int32_t hamming_weight, uint64_t capacity,
                         uint64_t *reps_dev, double *norms_dev, uint64_t *count);
/* Entries per row of the sector's matrix (off-diagonal transitions a state can take). */
uint32_t asp_sector_width(asp_operator const *op);
/* The operator in the basis `reps_dev` (sorted representatives, their norms) as an ELL matrix:
 * slot k of row i at [k * n + i]; idx = row index of the target's representative, val =
 * c * chi * norm(target) / norm(source) (the coefficient asp_operator_apply returns); unused
 * slots hold (i, 0.0); diag = the diagonal, summed bond by bond.  Targets outside `reps_dev`
 * (another magnetisation, norm 0) are dropped.  width >= asp_sector_width(op). */
int asp_sector_rows(asp_operator const *op, uint64_t n, uint64_t const *reps_dev,
                    double const *norms_dev, uint32_t width, uint32_t *idx_dev, double *val_dev,
                    double *diag_dev);
/* y = H x over those arrays: y[i] = diag[i] x[i] + sum_k val[k n + i] x[idx[k n + i]], k ascending. */
int asp_sector_matvec(uint64_t n, uint32_t width, uint32_t const *idx_dev, double const *val_dev,
                      double const *diag_dev, double const *x_dev, double *y_dev);

/* 1 when every row's targets are pairwise distinct for every input state (distinct flip
 * masks), which asp_operator_ising requires; 0 otherwise. */
int asp_operator_unique_targets(asp_operator const *op);
/* Upper bound of other_counts[i] (diagonal entry included). */
uint32_t asp_operator_max_connections(asp_operator const *op);

/* Replaces `hamiltonian.batched_apply` + the flattening of _batched_apply
 * (common.py:85-106) for n keys: per key one diagonal entry (the sum of the
 * bonds' diagonal matrix elements, added in bond order), then one entry per
 * non-zero off-diagonal element m[dst][src] in (bond, dst) order:
 *   other_keys[e] = key ^ flip(src ^ dst), other_coeffs[e] = m[dst][src].
 * other_counts[i] receives the number of entries of key i; *total their sum.
 * Fails with ASP_ERR_INVALID when *total > capacity (nothing is written then
 * except other_counts and *total). */
int asp_operator_apply(asp_operator const *op, uint64_t n, uint64_t const *keys,
                       uint64_t capacity, uint64_t *other_keys, double *other_coeffs,
                       int64_t *other_counts, uint64_t *total);

/* make_ising_model's arithmetic (common.py:131-208) without materialising the
 * connections: for sorted unique keys[K] and amplitudes psi[K] (already
 * L2-normalised over the cluster) computes
 *   M_ij = (H_ij * |psi_j|) * |psi_i|   for i, j both in the cluster,
 *   J    = 0.5 * (M + M^T), zeros dropped, as COO sorted by (row, col)
 * — the matrix `0.5 * (matrix + matrix.T); sort_indices(); tocoo()` of
 * common.py:194-196, bit for bit.  *nnz receives the length; row/col/val need
 * capacity >= *nnz (call with capacity 0 and NULL outputs to size them).
 * Operators whose rows reach pairwise distinct states (asp_operator_unique_targets) take one
 * fused pass.  Otherwise — symmetry-adapted bases, single-site flips — several connections of a
 * row may end in the same state, and the variant that keeps the reference's arithmetic for
 * them runs: duplicates of a row summed in connection order from 0 (scipy's csr + csr on
 * non-canonical input), then 0.5 * (Mhat_rj + Mhat_jr), entries pruned iff that sum is 0.  That
 * variant needs every coupling to have its mirror (Mhat_rj present iff Mhat_jr present: any
 * operator with a symmetric pattern); otherwise it fails with ASP_ERR_INVALID and
 * make_ising_model takes the asp_ising_elements route. */
int asp_operator_ising(asp_operator const *op, uint64_t num_spins, uint64_t const *keys,
                       double const *psi, uint64_t capacity, int32_t *row, int32_t *col,
                       double *val, uint64_t *nnz);
/* The same matrix as canonical CSR: indptr[num_spins + 1] instead of the row of every entry —
 * what asp_sa_plan_create and asp_sparsify_component take, without a counting pass over the
 * rows on the host (the sampled-cluster pipeline's form). */
int asp_operator_ising_csr(asp_operator const *op, uint64_t num_spins, uint64_t const *keys,
                           double const *psi, uint64_t capacity, int64_t *indptr, int32_t *col,
                           double *val, uint64_t *nnz);
/* Many clusters' coupling build in one call, specification ASP-ISING-SEG-1.  The
 * segment conventions are ASP-ELOC-1's (asp_operator_local_energy below): num_segments tables lie
 * concatenated in keys / psi [T = offsets[num_segments]], segment g is [offsets[g], offsets[g + 1]),
 * its keys ascending and unique, psi its amplitudes ALREADY normalised by the caller over that
 * segment (the library does not touch the normalisation); segments may be empty and a state may sit
 * in any number of them.  The law: for every segment g with n_g keys let (ip, c, v) be what
 *     asp_operator_ising_csr(op, n_g, keys + offsets[g], psi + offsets[g], ...)
 * returns; then indptr[offsets[g] + i] - indptr[offsets[g]] == ip[i] for i = 0 ... n_g, and the
 * entries indptr[offsets[g]] ... indptr[offsets[g + 1]] of col and val equal c and v, val bit for
 * bit.  indptr is ONE global i64[T + 1] starting at 0; col is SEGMENT-LOCAL (the position within the
 * segment's keys).  Both variants of asp_operator_ising are covered: the pair-fused pass for
 * asp_operator_unique_targets(op) == 1, and the duplicate-keeping one otherwise (duplicates summed
 * in connection order from 0, 0.5 * (Mhat_rj + Mhat_jr), pruned iff that sum is 0).  *nnz receives
 * the total.  Host pointers.
 * Before any device work and before any output is written: ASP_ERR_INVALID for a null handle, a
 * null nnz, null offsets with num_segments > 0, offsets[0] != 0 or decreasing offsets, null keys /
 * psi with T > 0 and a segment that is not ascending and unique (the message names the segment and
 * the index within it); ASP_ERR_TOO_LARGE for T >= 2^31 - 1 and for the LDS condition of
 * asp_operator_ising.  capacity == 0 with indptr, col and val all NULL is a sizing call; *nnz >
 * capacity or a missing output pointer gives ASP_ERR_INVALID with *nnz set and no output written.
 * A key of norm 0 in a -1 sector gives ASP_ERR_INVALID as in asp_operator_ising; a coupling without
 * its mirror in the duplicate variant gives ASP_ERR_INVALID, the message naming the first such
 * segment.  T == 0: *nnz = 0, indptr[0] = 0 when indptr is given, and no device is needed.  The
 * number of launches and of host synchronisations (two, or three in the duplicate variant) does
 * not depend on num_segments. */
int asp_operator_ising_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets,
                                uint64_t const *keys, double const *psi, uint64_t capacity,
                                int64_t *indptr, int32_t *col, double *val, uint64_t *nnz);

/* make_hamiltonian_extension's state set (common.py:516-522): the sorted unique
 * union of every key's targets (its own diagonal entry included).  *count receives
 * the size; out needs capacity >= *count (capacity 0 / NULL sizes it); *count > capacity is
 * ASP_ERR_INVALID with *count set and out not written.  Keys need not be sorted or unique, but
 * every key must lie below 2^number_spins: the set is sorted on the bits [0, number_spins), so a
 * key with a higher bit is refused with ASP_ERR_INVALID before any launch (*count = 0). */
int asp_operator_extend(asp_operator const *op, uint64_t n, uint64_t const *keys,
                        uint64_t capacity, uint64_t *out, uint64_t *count);
/* The extension of many clusters in one call, specification ASP-EXTEND-SEG-1: keys
 * [T = offsets[num_segments]] holds num_segments key sets one after the other, and
 * out[out_offsets[g] : out_offsets[g + 1]] is what asp_operator_extend(op, n_g, keys + offsets[g], ...)
 * returns — sorted, unique, for symmetry-adapted bases the representatives without the orbits of norm
 * 0.  A state may sit in any number of segments and comes out in each of them; keys within a segment
 * need not be sorted or unique; segments may be empty.  out_offsets is u64[num_segments + 1] from 0
 * and *count its last entry.  capacity == 0 with out == NULL is the sizing call (*count and
 * out_offsets set); *count > capacity or a missing out is ASP_ERR_INVALID with both set and out not
 * written.  Before any launch and before any output is written: ASP_ERR_INVALID for a null handle,
 * a null count or out_offsets, null offsets with num_segments > 0, offsets[0] != 0 or decreasing
 * offsets, null keys with T > 0 and a key with a bit at or above number_spins (the message names the
 * segment and the key); ASP_ERR_TOO_LARGE for T >= 2^32 - 1 and for T * max_connections >= 2^32 (the
 * bound on the connections that is known before a launch; the exact count is checked after the
 * counting pass as in asp_operator_extend).  A source key of norm 0 in a -1 sector is refused as in
 * asp_operator_extend.  T == 0 needs no device: *count = 0 and out_offsets all 0.  The number of
 * launches and of host synchronisations — TWO for the sizing call, THREE for a full call — does not
 * depend on num_segments. */
int asp_operator_extend_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets,
                                 uint64_t const *keys, uint64_t capacity, uint64_t *out,
                                 uint64_t *out_offsets, uint64_t *count);
/* The growth of many sampled clusters in one call, specification ASP-GROW-1.  Segment g
 * grows a cluster of at most sizes[g] >= 1 states around the basis state seeds[g] (for a symmetry-adapted
 * basis a representative of non-zero norm) by breadth-first passes t = 0, 1, ...: the frontier F_t
 * (F_0 = [seed]) is visited in ascending order; its states are added to the cluster until the size is
 * reached — then the segment ends after this pass —; the states before that one are applied
 * (asp_operator_apply's row order, own state first, in a symmetry-adapted basis the representatives
 * without the orbits of norm 0), and the k-th entry of the i-th source's row, if it is neither in the
 * cluster before the pass nor at a position <= i of F_t, is kept iff word 0 of Philox4x32-10(counter
 * (i, k, t, ids[g]), key (rng_seed low, high)) < floor(keep_probability * 2^32); F_{t+1} is the sorted set of
 * the kept ones.  A segment's result depends on (operator, seed, size, id, keep_probability, rng_seed) only.
 * out[out_offsets[g] : out_offsets[g + 1]] are segment g's states, ascending; out_offsets is
 * u64[num_segments + 1] from 0, *count its last entry, passes[g] (NULL: not wanted) the number of passes
 * in which segment g had a frontier.  The caller allocates capacity >= sum of sizes: an upper bound, so
 * there is no sizing call.  Before any launch and before any output is written: ASP_ERR_INVALID for a null
 * handle, a null count or out_offsets, null seeds, sizes or ids with num_segments > 0, a
 * keep_probability outside [0, 1] (or NaN), a size of 0, capacity below the sum of the sizes, a null out
 * and a seed with a bit at or above number_spins; ASP_ERR_TOO_LARGE for 2^32 - 1 or more segments or
 * states.  A pass whose applied sources times max_connections reach 2^32 is ASP_ERR_TOO_LARGE before that
 * pass's launches; a seed of norm 0 in a -1 sector is ASP_ERR_INVALID; in both cases no output is
 * written.  num_segments == 0 needs no device.  Per pass the number of launches and of host
 * synchronisations (two) does not depend on num_segments.  asp_operator_last_ms reports the duration. */
int asp_operator_grow_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *seeds,
                               uint64_t const *sizes, uint32_t const *ids, double keep_probability,
                               uint64_t rng_seed, uint64_t capacity, uint64_t *out, uint64_t *out_offsets,
                               uint64_t *count, uint32_t *passes /* [num_segments] or NULL */);

/* Boundary field of a cluster, specification ASP-FIELD-1: the miss branch of the
 * reference's coupling build (cbits/build_matrix.c:49) with counts = 1.  keys[num_spins] ascending
 * and unique with signed amplitudes psi (only |psi_r| is used); env_keys[num_env] ascending and
 * unique with signed amplitudes env_psi in the same normalisation.  For every row r, over the
 * entries asp_operator_apply returns for keys[r], in its order (equal targets not merged):
 *     acc = +0.0
 *     target in keys:                  nothing  (the diagonal entry included, whatever the
 *                                               environment says about that state)
 *     target = env_keys[p]:            acc = acc + ((coeff * |psi_r|) * env_psi[p])
 *     neither, and coeff != 0:         ++*unresolved  (contributes nothing)
 *     field[r] = scale * acc
 * every operation rounded on its own, the adds in that order: scale = 1 is the reference's field
 * bit for bit, scale = 2 (make_ising_model) makes c^2 (s'Js + h's) differ from the quantum energy
 * of the full vector with the cluster's signs replaced by s by a constant (c: the cluster's norm).
 * Host pointers; unresolved may be NULL.  ASP_ERR_INVALID before any device work for a null
 * handle, null keys / psi / field with num_spins > 0, null env_keys / env_psi with num_env > 0 and
 * keys that are not ascending; for a key of norm 0 in a -1 sector as asp_operator_ising.
 * num_spins = 0 runs nothing and needs no device; num_env = 0 is legal (field = scale * +0.0). */
int asp_operator_field(asp_operator const *op, uint64_t num_spins, uint64_t const *keys, double const *psi,
                       uint64_t num_env, uint64_t const *env_keys, double const *env_psi, double scale,
                       double *field, uint64_t *unresolved /* may be NULL */);
/* The boundary fields of many clusters in one call, specification ASP-FIELD-SEG-1.
 * num_segments clusters lie concatenated in keys / psi [T = offsets[num_segments]] and their
 * environments in env_keys / env_psi [E = env_offsets[num_segments]]: cluster g is
 * [offsets[g], offsets[g + 1]), its environment [env_offsets[g], env_offsets[g + 1]), each ascending
 * and unique, the amplitudes in the cluster's normalisation.  Segments of either kind may be empty; a
 * state may sit in any number of segments of either kind, and may be a cluster key of one segment and
 * an environment key of another; a row of segment g sees segment g's cluster and segment g's
 * environment only.  The law: for every segment g with n_g keys and e_g environment keys,
 * field[offsets[g] : offsets[g + 1]] and unresolved[g] are what
 *     asp_operator_field(op, n_g, keys + offsets[g], psi + offsets[g], e_g, env_keys + env_offsets[g],
 *                        env_psi + env_offsets[g], scale, ...)
 * returns: the field bit for bit (the sign of scale * +0.0 included), the count exactly.  With
 * n_g = 0 nothing is written for g and unresolved[g] = 0; with e_g = 0, field = scale * +0.0.  Both
 * variants of asp_operator_field are covered: lanes over the bonds for
 * asp_operator_unique_targets(op) == 1, the device connection list otherwise.  Host pointers;
 * unresolved (u64[num_segments]) may be NULL.
 * Before any device work and before any output is written: ASP_ERR_INVALID for a null handle, null
 * offsets or env_offsets with num_segments > 0, an offsets array that does not start at 0 or
 * decreases, null keys / psi / field with T > 0, null env_keys / env_psi with E > 0, and a cluster or
 * environment segment that is not ascending and unique (the message names the segment and the index
 * within it); ASP_ERR_TOO_LARGE for T >= 2^32 - 1 or E >= 2^32 - 1 (the hashes store index + 1 in 32
 * bits) and, in the connection-list variant, for T * max_connections >= 2^32.  A key of norm 0 in a
 * -1 sector gives ASP_ERR_INVALID as in asp_operator_field, the message naming the first such
 * segment, and no output is written.  T == 0 needs no device: unresolved is zeroed.  The number of
 * launches and of host synchronisations — ONE (the download), or TWO in the connection-list variant
 * (the size of the list, and the download) — does not depend on num_segments.  asp_operator_last_ms
 * reports the device time. */
int asp_operator_field_segments(asp_operator const *op, uint64_t num_segments,
                                uint64_t const *offsets,      /* u64[S+1] over keys / psi, T = offsets[S] */
                                uint64_t const *keys, double const *psi,
                                uint64_t const *env_offsets,  /* u64[S+1] over env_keys / env_psi, E = env_offsets[S] */
                                uint64_t const *env_keys, double const *env_psi,
                                double scale, double *field /* f64[T] */,
                                uint64_t *unresolved /* u64[S] or NULL */);

/* Local energies of signed amplitudes, specification ASP-ELOC-1:
 *     E_loc(s) = sum_s' H_ss' phi_s' / phi_s
 * for many small tables in one call.  num_segments tables lie concatenated in keys / phi
 * [T = offsets[num_segments]]: segment g is [offsets[g], offsets[g + 1]), its keys ascending and
 * unique, phi its signed amplitudes in any normalisation; segments may be empty and a state may sit
 * in any number of them (each with its own amplitude).  rows[num_rows] are indices into the table,
 * in any order, with repeats; the segment of a row is the one whose range holds rows[r].  For every
 * row, over the entries asp_operator_apply returns for keys[rows[r]], in its order (the diagonal
 * entry first; equal targets not merged):
 *     acc = +0.0 ; lost = 0
 *     target = keys[p], p in the row's segment:   acc = acc + (coeff * phi[p])
 *     otherwise, and coeff != 0:                  ++lost  (contributes nothing)
 *     hphi[r] = acc ; eloc[r] = acc / phi[rows[r]] ; missing[r] = lost
 * every operation rounded on its own, the adds in that order.  Negating phi over a whole segment
 * leaves eloc and negates hphi, bit for bit, wherever the sum is not zero (a sum that is exactly
 * zero is +0.0 either way).  Host pointers; each of hphi, eloc and missing may be NULL.  ASP_ERR_INVALID before any device work and before any output is written for a null
 * handle, null offsets with num_segments > 0, offsets[0] != 0 or decreasing offsets, null keys /
 * phi with T > 0, a segment that is not ascending and unique, null rows with num_rows > 0,
 * rows[r] >= T and, when eloc is wanted, a phi[rows[r]] that is zero, NaN or infinite; for a row
 * key of norm 0 in a -1 sector as asp_operator_field.  ASP_ERR_TOO_LARGE for T >= 2^32 - 1 or
 * num_rows >= 2^31 - 1.  num_rows = 0 runs nothing and needs no device. */
int asp_operator_local_energy(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets,
                              uint64_t const *keys, double const *phi, uint64_t num_rows,
                              uint64_t const *rows, double *hphi, double *eloc, uint32_t *missing);

/* Device time (ms, HIP events, no host<->HBM copies) of this thread's last
 * asp_operator_apply / _ising / _ising_segments / _extend / _field / _field_segments / _local_energy
 * call. */
float asp_operator_last_ms(void);

/* ------------------------------------------------------------------------- */
/* (3c) Global-cutoff sparsification + component extraction                  */
/* ------------------------------------------------------------------------- */

/* sparsify_using_global_cutoff (annealing_sign_problem/common.py:634-692) on a CSR matrix
 * (rows sorted by column, no duplicates):
 *   M'_ij = 0 where |M_ij| < reltol * max|M| unless spins i and j are both frozen   (:634-643)
 *   graph = non-zeros of 0.5 * (M' + M'^T)                                         (:660-662)
 *   keep[i] = 1 iff i is connected to `anchor` in that graph                        (:664-668)
 *   out_* = M[keep][:, keep], the UN-pruned block, as CSR with remapped columns    (:674)
 * Fails with ASP_ERR_INVALID when a frozen spin is not in the anchor's component (the
 * reference asserts it, :666).  *kept_spins and *out_nnz always receive the sizes; pass
 * capacity 0 and NULL out_* to get the mask only.  out_indptr needs *kept_spins + 1 entries. */
int asp_sparsify_component(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                           double const *data, uint8_t const *is_frozen, double reltol,
                           uint64_t anchor, uint8_t *keep, uint64_t *kept_spins,
                           uint64_t capacity, int64_t *out_indptr, int32_t *out_indices,
                           double *out_data, uint64_t *out_nnz);
/* The cutoff of many clusters in one call, specification ASP-SPARSIFY-SEG-1.  The
 * input conventions are the OUTPUT conventions of asp_operator_ising_segments: num_segments matrices
 * lie concatenated, segment g holds the spins [offsets[g], offsets[g + 1]) of T = offsets[num_segments];
 * indptr is ONE global i64[T + 1] starting at 0; indices are SEGMENT-LOCAL; rows sorted and
 * duplicate-free, stored zeros legal; is_frozen u8[T]; anchors[g] is local to segment g.  The law: for
 * every segment g with n_g > 0 let (keep_g, kept_g, ip, c, v) be what asp_sparsify_component returns
 * for the rebased segment with anchors[g]; then keep[offsets[g] : offsets[g + 1]] == keep_g,
 * kept_offsets[g + 1] - kept_offsets[g] == kept_g with kept_offsets[0] == 0, the rows kept_offsets[g] ...
 * kept_offsets[g + 1] of out_indptr, rebased, equal ip, their out_indices equal c (columns renumbered
 * WITHIN the segment's kept spins) and their out_data equal v bit for bit.  The threshold is PER
 * SEGMENT: reltol * max|data of segment g|, one rounded product (reltol * 0 for a segment without
 * non-zeros).  Empty segments are legal and their anchor is not read.
 * capacity == 0 with out_indptr, out_indices and out_data all NULL is the mask-only call: keep,
 * kept_offsets and *out_nnz are set.  *out_nnz > capacity or a missing output pointer gives
 * ASP_ERR_INVALID with keep, kept_offsets and *out_nnz set and no out_* written.  A frozen spin outside
 * its anchor's component gives ASP_ERR_INVALID, the message naming the FIRST such segment and its
 * number of stray spins; nothing is written to keep, kept_offsets or out_* then.
 * Before any device work and before any output is written: ASP_ERR_INVALID for a null kept_offsets or
 * out_nnz, null offsets or anchors with num_segments > 0, offsets[0] != 0 or decreasing offsets, null
 * indptr / is_frozen / keep with T > 0, indptr[0] != 0 or a non-monotone indptr, a column outside
 * [0, n_g), a row that is not sorted and duplicate-free (the message names the segment and the row)
 * and anchors[g] >= n_g with n_g > 0; ASP_ERR_TOO_LARGE for T >= 2^32 - 1.  T == 0 needs no device:
 * *out_nnz = 0, kept_offsets[0 ... num_segments] = 0 and out_indptr[0] = 0 when out_indptr is given.
 * Host pointers; out_indptr needs kept_offsets[num_segments] + 1 entries (T + 1 always suffice).  The
 * number of launches and of host synchronisations — ONE for the mask-only call, TWO for a full call —
 * does not depend on num_segments. */
int asp_sparsify_component_segments(uint64_t num_segments, uint64_t const *offsets,
                                    int64_t const *indptr, int32_t const *indices, double const *data,
                                    uint8_t const *is_frozen, double reltol, uint64_t const *anchors,
                                    uint8_t *keep, uint64_t *kept_offsets, uint64_t capacity,
                                    int64_t *out_indptr, int32_t *out_indices, double *out_data,
                                    uint64_t *out_nnz);
/* Device time (ms) of this thread's last asp_sparsify_component or asp_sparsify_component_segments
 * call, copies excluded. */
float asp_sparsify_last_ms(void);

/* ------------------------------------------------------------------------- */
/* (4) Annealer: replaces ising_glass_annealer.{Hamiltonian,anneal}          */
/*     call sites: common.py:204,242-248; full_hilbert_space.py:212-218      */
/* ------------------------------------------------------------------------- */

typedef struct asp_sa_plan asp_sa_plan;

/* Build the device-resident sweep plan for E(s) = sum_ij J_ij s_i s_j +
 * sum_i h_i s_i.  J is a square CSR matrix with sorted, duplicate-free column
 * indices per row (scipy "canonical format"); it may carry a diagonal and need
 * not be symmetric (the sweep uses J + J^T).  Host preprocessing: symmetrised
 * off-diagonal part, DSATUR colouring, colour-major permutation,
 * 64-row sliced-ELL slabs; all uploaded once.  NULL on failure. */
asp_sa_plan *asp_sa_plan_create(uint64_t num_spins, int64_t const *indptr,
                                int32_t const *indices, double const *data,
                                double const *field);
void asp_sa_plan_destroy(asp_sa_plan *p);

typedef struct asp_sa_info {
  uint64_t num_spins;
  uint64_t nnz_offdiag;     /* entries of offdiag(J + J^T) after dropping zeros */
  uint64_t ell_entries;     /* slab entries incl. padding (64 * sum of widths)  */
  uint32_t num_colors;
  uint32_t num_blocks;      /* 64-row blocks (colour classes padded)            */
  uint32_t max_degree;
  int32_t energy_scale_exp; /* S: tracked energies are in units of 2^-S         */
  double diag_sum;          /* sum_i J_ii                                       */
  double beta0_auto;        /* ln 2 / max_i dE_max(i)                           */
  double beta1_auto;        /* ln 100 / min over non-zero couplings             */
} asp_sa_info;
int asp_sa_plan_info(asp_sa_plan const *p, asp_sa_info *info);

/* The same host preprocessing WITHOUT touching a device (inspection, CPU tests):
 * fills *info and, when non-NULL, colors[K] (greedy colour of every spin) and
 * position[K] (index of the spin in the padded, colour-major order). */
int asp_sa_layout_host(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                       double const *data, double const *field, asp_sa_info *info,
                       int32_t *colors, uint32_t *position);

/* How often the host preprocessing (colouring, permutation, sliced ELL) has run in this process:
 * asp_sa_plan_create, asp_sa_layout_host and asp_sa_shuffled_order_host each count one; the two calls
 * below count none. */
uint64_t asp_sa_layout_build_count(void);

/* New numbers on the SAME pattern, in place and without the host preprocessing:
 * afterwards the plan is indistinguishable, bit for bit, from asp_sa_plan_create(K, indptr, indices,
 * data, field) — every field of asp_sa_plan_info, energies, anneals and traces in both orders, chains
 * created afterwards, ladder / exchange / resample / cluster moves, the greedy solver with every tree.
 * (nnz, indptr, indices) must equal the arrays the plan was created from, entry for entry; data == NULL
 * keeps the couplings, field == NULL the field (both NULL: ASP_ERR_INVALID; a plan without spins: a
 * no-op).  The device merges J_ij + J_ji of every coupling of the plan from the uploaded data and
 * scatters it into every value array the plan holds at that moment; the host layout and the scales
 * follow.  ASP_ERR_INVALID, with the plan answering exactly as before the call: a NULL plan (no device
 * needed), another pattern, a live asp_sa_chains handle of the plan (its tracked energies belong to the
 * old couplings), non-finite numbers or an overflowing bound (asp_sa_plan_create's messages), and a
 * changed pattern of J + J^T — a coupling of the plan whose new J_ij + J_ji is exactly 0 (a fresh plan
 * would drop it) or a stored pair that cancelled at creation and no longer does ("pattern mismatch"
 * starts the message of every pattern error). */
int asp_sa_plan_reweight(asp_sa_plan *p, uint64_t nnz, int64_t const *indptr, int32_t const *indices,
                         double const *data, double const *field);
/* Device time (ms, HIP events) of the plan's last successful asp_sa_plan_reweight: uploads, kernels
 * and the read-back of the row sums. */
float asp_sa_plan_reweight_last_ms(asp_sa_plan const *p);
/* A second plan with the structure and the numbers of *p, made without the host preprocessing: its own
 * stream, events, work buffers and arrays (it outlives *p), the launch settings of *p (asp_sa_set_launch,
 * _set_packed, _set_lds_limit, _set_wide, _set_team, _set_field_cache, _set_post, _set_shuffled_launch, _set_shuffled_teams,
 * _set_greedy_tree) and none of its chains.  What asp_sa_greedy_batch and the other batched calls need
 * to solve several reweighted copies of one model at once: they refuse one plan twice. */
int asp_sa_plan_clone(asp_sa_plan const *p, asp_sa_plan **out);

/* The plans of a whole round in one call, specification ASP-PLAN-SEG-1.  The input
 * conventions are the OUTPUT conventions of asp_operator_ising_segments and
 * asp_sparsify_component_segments, so the three calls chain: segment g holds the spins [offsets[g],
 * offsets[g + 1]) of T = offsets[num_segments]; indptr is ONE global i64[T + 1] starting at 0; indices
 * are SEGMENT-LOCAL; rows sorted and duplicate-free, stored zeros and a stored diagonal legal; field is
 * f64[T].  Host pointers.  The law: after a successful call out_plans[g] is indistinguishable from
 * asp_sa_plan_create(n_g, rebased indptr, indices, data, field of segment g) — every field of
 * asp_sa_plan_info, every device array of the plan byte for byte (asp_sa_plan_read_array), the stored
 * pattern (asp_sa_plan_reweight and asp_sa_plan_clone work), the environment read at creation
 * (ASP_SA_TEAM), energies, anneals in both orders, chains, the greedy solver with every tree.  An empty
 * segment yields what asp_sa_plan_create(0, ...) yields.  Every plan is an object of its own, destroyed
 * with asp_sa_plan_destroy; each segment adds one to asp_sa_layout_build_count.
 * On failure every out_plans[g] is NULL and nothing leaks.  Before any device work: ASP_ERR_INVALID
 * for a null out_plans or offsets, offsets[0] != 0 or decreasing offsets, null indptr / field with
 * T > 0, indptr[0] != 0 or a non-monotone indptr, null indices / data with stored entries;
 * ASP_ERR_TOO_LARGE for T or the number of stored entries >= 2^32 - 1.  A column out of range, a row
 * that is not canonical, a non-finite coupling or field and an overflowing bound fail with
 * asp_sa_plan_create's message behind "segment <g>: ", g the first such segment.  num_segments == 0
 * needs no device.  The device forms A = offdiag(J + J^T) and the rows' statistics for all segments
 * at once (a segment with a stored entry whose mirror is not stored takes the host's route instead);
 * the host colours and orders every segment on at most 16 threads; one kernel then writes every
 * plan's arrays, the padded ELL from the A that is still on the device.  7 launches, 2 fills, 12
 * copies and 2 host synchronisations, whatever num_segments. */
int asp_sa_plan_create_segments(uint64_t num_segments, uint64_t const *offsets, int64_t const *indptr,
                                int32_t const *indices, double const *data, double const *field,
                                asp_sa_plan **out_plans);
/* Device time (ms, HIP events) of this thread's last asp_sa_plan_create_segments call: its kernels,
 * copies excluded. */
float asp_sa_plan_segments_last_ms(void);

/* The device arrays of a plan, for asp_sa_plan_read_array. */
enum {
  ASP_SA_ARRAY_COLOR_BLOCK_START = 0, /* u32[num_colors + 1]                        */
  ASP_SA_ARRAY_BLOCK_WIDTH = 1,       /* u32[num_blocks]                            */
  ASP_SA_ARRAY_ELL_OFF = 2,           /* u64[num_blocks + 1], in 64-entry slabs     */
  ASP_SA_ARRAY_ELL_COL = 3,           /* u32[ell_entries + tail], quad-interleaved  */
  ASP_SA_ARRAY_ELL_COL4 = 4,          /* the same as LDS byte addresses, if held    */
  ASP_SA_ARRAY_ELL_VAL = 5,           /* f64[ell_entries + tail]                    */
  ASP_SA_ARRAY_SPIN_OF_POS = 6,       /* u32[num_blocks * 64]                       */
  ASP_SA_ARRAY_POS_OF_SPIN = 7,       /* u32[num_spins]                             */
  ASP_SA_ARRAY_FIELD_POS = 8          /* f64[num_blocks * 64]                       */
};
/* Copies one device array of the plan to dst (host).  *bytes is always set, to the size of the array:
 * 0 for an array the plan does not hold (ell_col4 where the wide layout does not fit; every ELL array
 * of a plan without spins).  ASP_ERR_INVALID for a null plan or byte count, an unknown id and a
 * capacity below *bytes (nothing is copied then). */
int asp_sa_plan_read_array(asp_sa_plan const *p, int which, void *dst, uint64_t capacity_bytes, uint64_t *bytes);

/* ---- coupling stencil: the couplings of a fixed set of states from new amplitudes alone ----------
 * Specification ASP-STENCIL-1.  Inputs: an operator, K sorted unique keys and the
 * canonical CSR pattern (indptr, indices) of the J that asp_operator_ising_csr(op, K, keys, psi0)
 * returned for some psi0.  The connections of row i are what asp_operator_apply lists for keys[i], in
 * its order (the diagonal entry first; representatives and their coefficients for a symmetry-adapted
 * basis); a connection whose target is not among the keys does not take part.  For finite amplitudes
 * psi[K], normalised by the caller:
 *     Mhat_ij = +0.0, then for the connections d of row i that land on j, in connection order,
 *               Mhat_ij = Mhat_ij + ((c_d * |psi_j|) * |psi_i|)
 *     J_ij    = 0.5 * (Mhat_ij + Mhat_ji)       (a side without a connection is +0.0)
 * every operation rounded on its own (__dmul_rn, __dadd_rn, no contraction); the entry exists iff the sum
 * is non-zero.  Whenever asp_operator_ising_csr(op, K, keys, psi) succeeds with the stencil's pattern,
 * these values equal the ones it returns bit for bit.  STORED pairs are the entries of the pattern,
 * SILENT pairs the pairs with at least one connection and no entry (their sum was exactly 0 for psi0).
 * For new amplitudes the pattern has changed iff a stored pair now sums to exactly 0 or a silent pair no
 * longer does: that is reported per draw (status 1), and nothing is written for that draw.
 *
 * asp_ising_stencil_create runs the action once, resolves the targets among the keys, groups the
 * connections of every row by target (connection order kept inside a group) and keeps the groups, the
 * places of every stored pair's forward and mirror group and the silent pairs on the device.
 * ASP_ERR_INVALID: a null argument, unsorted or duplicate keys, a non-canonical pattern, a pattern entry
 * that no connection produces, a pattern that holds (i, j) without (j, i), a key outside the sector, and
 * — for operators whose rows may reach a state twice — a group without its mirror group (one-directional
 * matrix elements: asp_operator_ising_csr sends the caller to the host route with the same code). */
typedef struct asp_ising_stencil asp_ising_stencil;
typedef struct asp_ising_stencil_counts {
  uint64_t num_spins;     /* K */
  uint64_t stored;        /* entries of the pattern */
  uint64_t connections;   /* connections whose target is among the keys */
  uint64_t groups;        /* (row, target) groups of them */
  uint64_t silent_pairs;  /* unordered pairs with a connection and no entry */
  uint64_t longest_group; /* connections of the longest group */
} asp_ising_stencil_counts;
int asp_ising_stencil_create(asp_operator const *op, uint64_t num_spins, uint64_t const *keys,
                             int64_t const *indptr, int32_t const *indices, asp_ising_stencil **out);
void asp_ising_stencil_destroy(asp_ising_stencil *st);
int asp_ising_stencil_info(asp_ising_stencil const *st, asp_ising_stencil_counts *out);
/* data[d][nnz] (pattern order) and status[d] (0 applied, 1 pattern changed: data[d] unspecified) of
 * `count` draws psi[d][K]: one upload, a fixed number of launches (one fold per group in fixed order, one
 * 0.5 * (a + b) per stored entry, the zero / non-zero counts per draw), one download of the values (the
 * 2 * count counters follow in a copy of their own), one synchronisation.  Non-finite
 * amplitudes fail the call (ASP_ERR_INVALID, the draw's index in the message) before any launch;
 * count == 0 and K == 0 need no device.  A stencil serves one thread at a time. */
int asp_ising_stencil_values(asp_ising_stencil *st, uint32_t count, double const *psi, double *data,
                             int32_t *status);
/* One draw of asp_sa_plan_reweight_stencil_batch: the plan takes the couplings of `psi` (K amplitudes)
 * and, unless field == NULL (keep), the field; data_out (nnz doubles, or NULL) receives the couplings;
 * status: 0 applied, 1 pattern changed (J's, or that of J + J^T) — the plan is exactly as it was. */
typedef struct asp_sa_stencil_item {
  asp_sa_plan *plan;
  double const *psi;
  double const *field;
  double *data_out;
  int32_t status;
} asp_sa_stencil_item;
/* asp_sa_plan_reweight(plan, nnz, indptr, indices, data_d, field_d) for every draw d with the values of
 * asp_ising_stencil_values, which never visit the host on their way into the plans: an applied plan equals
 * that call's result bit for bit (asp_sa_plan_info, the ELL values, the lazily uploaded row arrays where
 * they exist, the host mirrors, diag_sum in row order, the scales with rows folded in index order).  One
 * upload of all amplitudes (and one of the fields); per draw the merged values, row sums, row minima and
 * diagonal entries come back, and data_out where asked for; the number of host synchronisations does not
 * grow with count.  Every plan must have been created from, or cloned from a plan of, the stencil's
 * pattern; the plans are pairwise distinct and have no live asp_sa_chains handle.  ASP_ERR_INVALID for
 * the whole call, before any plan is touched and with the item's index in the message: a null stencil,
 * null items with count > 0, a null plan or psi, another pattern, one plan twice, live chains, non-finite
 * amplitudes or field, couplings that overflow.  A draw with status 1 does not stop the others. */
int asp_sa_plan_reweight_stencil_batch(asp_ising_stencil *st, asp_sa_stencil_item *items, uint32_t count);
/* Device time (ms, HIP events) of this thread's last successful asp_sa_plan_reweight_stencil_batch. */
float asp_sa_plan_reweight_stencil_last_ms(void);

/* Host-only (inspection, CPU tests): where the shared launches of the batched calls (asp_sa_anneal_batch,
 * asp_sa_chains_advance_batch, asp_sa_greedy_batch) place the workgroups of ONE launch class.  Member k
 * < count has groups[k] workgroups of about work[k] each.  The members go in descending work, stable,
 * each whole to the XCD (of eight) with the fewest workgroups so far, ties to the lowest index; the eight
 * lists are padded to the longest, *slots_per_xcd, with (0xFFFFFFFF, 0).  slots: the table as uploaded,
 * [8][*slots_per_xcd] pairs (member, group) of uint32 — workgroup b of the launch reads pair
 * (b % 8) * *slots_per_xcd + b / 8 —; capacity: the pairs it holds.  ASP_ERR_INVALID with nothing written
 * when the table needs more.  Placement changes speed only, never a result. */
int asp_sa_batch_slots_host(uint32_t count, double const *work, uint32_t const *groups,
                            uint32_t *slots_per_xcd, uint32_t *slots, uint64_t capacity);

/* Host-only: the visiting order of sweep `sweep` of the SHUFFLED variant (asp_sa_anneal_shuffled):
 * order[k] = k-th spin visited (level-major), level_of_position[k] = its level, *num_levels the
 * number of levels.  Any output may be NULL. */
int asp_sa_shuffled_order_host(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                               double const *data, double const *field, uint64_t seed,
                               uint32_t sweep, uint32_t *order, uint32_t *level_of_position,
                               uint32_t *num_levels);

/* Launch geometry override (0 = choose automatically).
 * replicas_per_group in {1,2,4,8}; threads multiple of 64, <= 1024. */
int asp_sa_set_launch(asp_sa_plan *p, int replicas_per_group, int threads);

/* Layout of the spins in the COLOUR order (the shuffled order ignores this setting and
 * asp_sa_set_wide): by default one LDS byte per spin position (bit m = replica m of the
 * workgroup); automatically one LDS BIT per position with one replica per workgroup when the
 * bytes do not fit the LDS of a workgroup (160 KiB at 74 bytes per block of 64 positions, tables
 * included: ~1.4e5 positions — the one threshold the comments below mean by "the capacity of a byte
 * per position"), and the same bit words kept in HBM when not even the bits fit (8 bytes per block:
 * beyond ~1.3e6; slow, but no size limit).  packed = 1 / 2 forces the LDS-bit / HBM-bit layout
 * (tests, measurements), 0 restores the automatic choice; asp_sa_set_lds_limit moves the thresholds
 * themselves.  Results never depend on the layout. */
int asp_sa_set_packed(asp_sa_plan *p, int packed);

/* With four replicas per workgroup and up to ~4e4 spins the kernel keeps a 32-bit word
 * per position (one byte per replica), which makes the sign of a coupling term a single SDWA
 * instruction.  allow = 0 keeps the byte layout (tests, measurements); default 1.
 * Beyond the capacity of a byte per position (asp_sa_set_packed's threshold, ~1.4e5) and with chains
 * enough for four per workgroup, four bits per position (42 bytes per block: up to ~2.4e5; flips are
 * LDS atomics); otherwise a bit per position and one chain per workgroup.
 * asp_sa_last_layout: 0 = bytes, 1 = bits in LDS, 2 = words, 3 = bits in HBM, 6 = nibbles, for
 * the last anneal/greedy call. */
int asp_sa_set_wide(asp_sa_plan *p, int allow);
int asp_sa_last_layout(asp_sa_plan const *p);
/* Tests, measurements: choose the spin layouts of this plan's sweeps, in both orders, as if the
 * device had `bytes` of LDS per workgroup.  0 restores the device's; values above it are clamped.
 * Only the choice between words, bytes, nibbles, bits and HBM (and, in the shuffled order, the chains
 * per workgroup and the lane packing that follow from it) looks at the limit: a launch still asks for
 * the LDS it needs, and the order build and the team sweep keep the device's.  A limit that not even
 * the shuffled order's HBM layout fits (its per-sweep tables stay in LDS) is ASP_ERR_TOO_LARGE with
 * nothing launched; the colour order's HBM layout fits any limit.  Handles hold nothing that depends
 * on the layout between segments: the limit may change while they are live.  asp_sa_plan_clone copies
 * it.  Results never depend on it. */
int asp_sa_set_lds_limit(asp_sa_plan *p, uint64_t bytes);
/* Spin layout of the plan's last sweep call in either order, in asp_sa_last_layout's codes
 * (0 bytes, 1 bits in LDS, 2 words, 3 words in HBM, 6 nibbles; lane packing reports 2; a team launch
 * its bits, 1).  asp_sa_last_layout itself is unchanged (5 for the shuffled order, 4 for a team
 * launch).  NULL plan: -1. */
int asp_sa_last_spin_layout(asp_sa_plan const *p);

/* Few chains on a large cluster (chains <= CUs / 2, e.g. the reference's default of 64
 * repetitions): each chain is spread over a TEAM of 2, 4 or 8 workgroups that split every colour
 * class, exchange one flip word per block and meet at a device-scope barrier per colour
 * (all of a team's workgroups must be resident together: the grid stays within the CU count,
 * team launches of one process take turns, and if the device is shared and a barrier times out the
 * call is repeated without teams — one process per GPU is assumed).  team = -1 chooses automatically (default), 0 never, 2/4/8 forces that
 * team size when the chains fit (tests, measurements).  Chains are bit-identical either way;
 * asp_sa_last_layout reports 4 for a team launch. */
int asp_sa_set_team(asp_sa_plan *p, int team);
/* How often the team barrier's watchdog gave up (the members of a team were not resident together:
 * another process or a long kernel held compute units): each trip costs the ~5 s the watchdog waits
 * plus the repeat of the call without teams, and used to be silent.  of_plan: calls of this plan
 * (NULL plan: 0); of_process: all plans of the process.  Either pointer may be NULL. */
int asp_sa_team_watchdog_trips(asp_sa_plan const *p, uint32_t *of_plan, uint64_t *of_process);

/* Field cache (default on): once a sweep flips few spins, a workgroup keeps the local fields
 * of every block in HBM and re-evaluates a block only after one of its neighbours flipped.
 * Pure optimisation of frozen sweeps; results are identical with it on or off. */
int asp_sa_set_field_cache(asp_sa_plan *p, int enable);

/* Tail sweeps (default automatic): the closed calls with four chains per workgroup in bytes or words
 * (asp_sa_anneal, asp_sa_anneal_trace) keep one `todo` bit per position once a sweep flips few spins,
 * and a sweep then evaluates only the listed rows — those with a neighbour that flipped in some chain
 * since their last evaluation, or with a proposal that was not a certain rejection — compacted into
 * visits of 64 rows from any blocks of the colour.  These launches run without the field cache.
 * n = -1: enter below c * num_spins / mean degree flips of the workgroup per sweep (c = 0.05:
 * DESIGN.md section 6), 0: never (the kernels without tail sweeps, with the field cache), n > 0: enter below
 * n flips.  Tail sweeps are left above twice the threshold and in front of a sweep whose beta is below
 * the one before it.  asp_sa_set_field_cache(p, 0) turns them off as well.  Launches whose LDS has
 * no room for the bitmap keep the kernels without tail sweeps.  Pure optimisation; results are
 * identical whatever n.  asp_sa_plan_clone copies it. */
int asp_sa_set_tail(asp_sa_plan *p, int n);
/* The last closed call of the plan (asp_sa_anneal / _trace): the fewest and the most sweeps one group
 * of chains ran as tail sweeps, and the most times one group entered them; zeros when the launch took a
 * kernel without tail sweeps.  Any pointer may be NULL. */
int asp_sa_last_tail(asp_sa_plan const *p, uint32_t *sweeps_min, uint32_t *sweeps_max, uint32_t *entries_max);

/* The pass after the sweeps (default on): for eight or more configurations whose sign bytes fit the
 * LDS (up to ~1.6e5 spins), the reported energies (and, in asp_sa_anneal / _trace, the unpermuted
 * configurations) come from one kernel that stages four configurations as the sweep's spin bytes
 * and sums the rows with the sweep's k-loop.  enable = 0 keeps the older energy and unpermute
 * kernels, which fewer configurations and larger plans use anyway (tests, measurements).
 * Pure optimisation; energies and configurations are identical with it on or off. */
int asp_sa_set_post(asp_sa_plan *p, int enable);

/* Run `repetitions` independent annealing chains (global replica ids
 * replica_offset .. replica_offset+repetitions-1) of num_sweeps sweeps, sweep t
 * at inverse temperature betas[t].  x0 == NULL: random initial spins from the
 * counter RNG; otherwise every chain starts from the packed configuration x0
 * (ceil(K/64) words, bit set = +1).  Outputs (host): out_x[repetitions *
 * ceil(K/64)] best configuration of each chain, out_e[repetitions] its energy.
 * The result depends only on (J, h, seed, betas, global replica id), not on the
 * launch geometry or the number of GPUs.  out_x / out_e may also be DEVICE pointers on the
 * library's device (the copies use hipMemcpyDefault): the multi-GPU layer gathers them over
 * RCCL without a host round trip. */
int asp_sa_anneal(asp_sa_plan *p, uint64_t seed, double const *betas,
                  uint32_t num_sweeps, uint32_t repetitions, uint32_t replica_offset,
                  uint64_t const *x0, uint64_t *out_x, double *out_e);
/* asp_sa_anneal that also returns every chain's energy after each sweep — the per-sweep
 * traces the older annealer API handed back as `(x, e_current[], e_best[]) = anneal(h, x0, seed,
 * number_sweeps, beta0, beta1)` (annealing_sign_problem/train.py:238-245,297).
 * out_trace[r * (num_sweeps + 1) + t] = tracked energy of chain r after t sweeps in units of
 * 2^-energy_scale_exp, relative to its initial configuration (entry 0 is 0); exact integer
 * bookkeeping of the accepted dE.  The best-so-far trace is its running
 * minimum. */
int asp_sa_anneal_trace(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
                        uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0,
                        uint64_t *out_x, double *out_e, int64_t *out_trace);

/* asp_sa_anneal with a fresh visiting order every sweep — what the reference's annealer almost
 * certainly does (its published success probabilities are reproduced by this order and by no
 * fixed one: DESIGN.md §6.1), and therefore the order the Python entry points use by default.
 * Sweep t visits the spins in ascending (priority, index), priority = word 0 of
 * Philox4x32-10(counter (i, t, 0xFFFFFFFE, 0), key seed); every chain uses the same order.
 * Proposal arithmetic, random words, energy bookkeeping, outputs and determinism are those of
 * asp_sa_anneal; only the order differs.  The orders are built ON THE DEVICE, a chunk of sweeps at
 * a time (csrc/sa_shuffled.hip: priorities, levels of the priority graph, the sweep's couplings
 * re-laid level by level in blocks of 4 .. 64 spins), beside the sweep kernel of the previous
 * chunk: a workgroup per sweep with its arrays in LDS for clusters up to ~1.2e4 spins, grids over
 * all sweeps of the chunk with one launch per level beyond.  Spins stay in LDS in original order
 * (a word, a byte, four bits or one bit per spin: up to ~6e5 spins) and in HBM beyond that.
 * out_x / out_e may be host or device pointers.  asp_sa_last_layout reports 5. */
int asp_sa_anneal_shuffled(asp_sa_plan *p, uint64_t seed, double const *betas, uint32_t num_sweeps,
                           uint32_t repetitions, uint32_t replica_offset, uint64_t const *x0,
                           uint64_t *out_x, double *out_e);
/* asp_sa_anneal_shuffled that also returns every chain's energy after each sweep: the per-sweep
 * traces of asp_sa_anneal_trace for the visiting order the Python entry points use by default.
 * out_trace (HOST, [repetitions][num_sweeps + 1]) has the meaning and units given there:
 * out_trace[r * (num_sweeps + 1) + t] = tracked energy of chain r of the call (global replica
 * replica_offset + r) after t sweeps in units of 2^-energy_scale_exp, relative to its initial
 * configuration (entry 0 is 0); the best-so-far trace is its running minimum, and its last value is
 * what asp_sa_last_stats reports as the tracked energy.  The value is stored where the sweep kernel
 * folds the sweep's exact integer energy change into the chain's tracked energy, after the last
 * level of the sweep: one 8-byte store per chain and sweep, gathered in a device buffer of the plan
 * and copied out once at the end.  Everything else — out_x, out_e, asp_sa_last_stats,
 * asp_sa_last_layout (5), asp_sa_last_shuffled* and the kernel form the launcher picks (spin layout,
 * chains per group, lane packing, teams) — is exactly that of asp_sa_anneal_shuffled with the same
 * arguments.  out_trace == NULL is ASP_ERR_INVALID, checked before any device work; a trace buffer
 * that cannot be allocated is ASP_ERR_ALLOC and no output is written.  num_sweeps == 0 writes the
 * single 0 of every chain, a plan without spins rows of zeros.  The batched launches
 * (ASP_SA_BATCH_SHUFFLED) have no trace form. */
int asp_sa_anneal_shuffled_trace(asp_sa_plan *p, uint64_t seed, double const *betas,
                                 uint32_t num_sweeps, uint32_t repetitions,
                                 uint32_t replica_offset, uint64_t const *x0, uint64_t *out_x,
                                 double *out_e, int64_t *out_trace);
/* Launch geometry of the shuffled sweep (0 = automatic): chains per workgroup in {1,2,4,8} and
 * wavefronts per workgroup in 1..8.  Results never depend on it. */
int asp_sa_set_shuffled_launch(asp_sa_plan *p, int chains_per_group, int wavefronts);
/* Teams of a shuffled-sweep workgroup (0 = automatic): with 2 the wavefronts split into two teams
 * that visit the same blocks for one half of the group's chains each (`wavefronts` above is then
 * per team, at most 4).  Results never depend on it. */
int asp_sa_set_shuffled_teams(asp_sa_plan *p, int teams);
/* Of the last asp_sa_anneal_shuffled call: the largest number of levels of a sweep. */
int asp_sa_last_shuffled(asp_sa_plan const *p, uint32_t *levels, float *order_ms);
/* Of the last shuffled call or batch item of this plan: spins per block of the level-major coupling
 * stream (64, or 4 .. 32 with lane packing: a wavefront then visits a block for 64 / spins_per_block
 * groups of chains at once — small levels filled with chains instead of padding lanes) and the
 * workgroups of its sweep launches.  Results never depend on either; ASP_SHUFFLED_LOG_S=2..6 in
 * the environment forces the block size, ASP_SHUFFLED_NO_PACKING=1 keeps blocks of 64. */
int asp_sa_last_shuffled_blocks(asp_sa_plan const *p, uint32_t *spins_per_block, uint32_t *workgroups);
/* Of the last shuffled call or batch item of this plan, how full its level-major blocks were (the
 * sweep of the call with the most blocks / quads): lane_fill = spins / lane slots (K over blocks x
 * spins per block: what is lost to levels that do not fill their last block), row_fill = couplings
 * of the rows (in quads) / coupling slots (blocks x their width: what is lost to a block being as
 * wide as its longest row).  The exec-mask counters of a profiler do not see either: a padding lane
 * and a padding coupling execute like real ones. */
int asp_sa_last_shuffled_fill(asp_sa_plan const *p, double *lane_fill, double *row_fill);

/* RESUMABLE chains: a device-resident set of chains of one plan that is advanced a
 * segment of sweeps at a time, inspected, checkpointed and continued — per-chain start
 * configurations (annealing_sign_problem/train.py:238-245,297 anneals from a caller's x0), early
 * stopping, re-heating, a change of visiting order in mid-run, a killed job that resumes.
 *
 * The continuation law: for any split n_1 + ... + n_k = N of a schedule betas[0..N) (segments of 0
 * sweeps included), create(p, seed, R, off, x0, 0), advance(betas + n_1 + .. + n_{i-1}, n_i, order) for
 * every i and result() return the words and doubles of asp_sa_anneal (order 0) / asp_sa_anneal_shuffled
 * (order 1) called with (p, seed, betas, N, R, off, x0); the traces, concatenated without each later
 * segment's entry 0, are those of the _trace calls, and the final tracked_best / accepted are that
 * call's asp_sa_last_stats.  Sweep k of a segment is sweep t = sweeps_done + k of the chain: in the
 * Philox counter of its random words and in the priorities of its shuffled visiting order (the order
 * build starts its chunks at any t); "best" carries across segments with the closed call's tie-break
 * (replaced on a strict improvement over the carried tracked_best only).
 *
 * Between calls a handle holds, per chain, two configurations in original spin order and three
 * integers — nothing that depends on the visiting order or on a launch choice —, so segments may
 * change `order`, and export -> import into another handle of the same plan continues the same chains.
 * Buffers are sized once, at create (a handle that is gathered or resampled adds a second set then:
 * below).  Launch forms: a segment in the shuffled order runs every form
 * of asp_sa_anneal_shuffled (spin layouts, chains per group, lane packing, asp_sa_set_shuffled_launch
 * / _teams); a segment in the colour order runs every spin layout and group size of asp_sa_anneal
 * (asp_sa_set_launch, _set_packed, _set_wide and _set_field_cache are honoured) but NO team launches:
 * asp_sa_set_team is ignored and few chains on a large cluster run one workgroup per chain.  Results
 * never depend on any of it.  A handle is used by one thread at a time, with its plan, and must be
 * destroyed before the plan is.
 *
 * Every argument is checked before any device work and before any output is written; ASP_ERR_INVALID:
 * a null plan / handle / out pointer, null betas with num_sweeps > 0, a negative or NaN beta, an order
 * other than 0 or 1, an x0_stride of 1 .. ceil(K/64) - 1, sweeps_done + num_sweeps > 2^32 - 2 (t = 2^32 - 1
 * is the random start's counter), a snapshot to import that lacks one of its five arrays.
 * repetitions = 0 and plans without spins behave as in the closed calls (nothing runs, energies 0). */
typedef struct asp_sa_chains asp_sa_chains;

/* x0 == NULL: the random start of asp_sa_anneal (the t = 2^32 - 1 draw).  x0_stride == 0: every chain
 * starts from the ceil(K/64) words at x0.  x0_stride >= ceil(K/64): chain r starts from
 * x0 + r * x0_stride — chain r is then the one chain of a handle created with repetitions = 1,
 * replica_offset + r and the shared start x0 + r * x0_stride.  Host pointers. */
int asp_sa_chains_create(asp_sa_plan *p, uint64_t seed, uint32_t repetitions, uint32_t replica_offset,
                         uint64_t const *x0, uint64_t x0_stride, asp_sa_chains **out);
void asp_sa_chains_destroy(asp_sa_chains *c);

/* Run sweeps t0 .. t0 + num_sweeps - 1 (t0 = sweeps done so far) at betas[0..num_sweeps).
 * order: 0 = colour (asp_sa_anneal's chain), 1 = shuffled (asp_sa_anneal_shuffled's).
 * out_trace: NULL, or HOST [repetitions][num_sweeps + 1]: the tracked energy at the start of the
 * segment (entry 0, NOT reset to 0) and after each of its sweeps, in the units of asp_sa_anneal_trace,
 * relative to the chain's very first configuration.  asp_sa_last_sweep_ms / _total_ms / _last_launch /
 * _last_layout of the plan describe the segment. */
int asp_sa_chains_advance(asp_sa_chains *c, double const *betas, uint32_t num_sweeps, uint32_t order,
                          int64_t *out_trace);

/* A LADDER segment ("Ladder law"): every chain runs at its OWN inverse temperature,
 * chain_betas: HOST [repetitions].  Afterwards chain r of the handle is in exactly the state it would
 * have after asp_sa_chains_advance with betas = {chain_betas[r]} x num_sweeps on a handle that holds
 * that one chain alone — replica id replica_offset + r, the same seed, start and sweeps_done: all five
 * state arrays, sweeps_done and row r of out_trace.  Hence equal entries are asp_sa_chains_advance on a
 * constant segment, bit for bit; ladder segments, ordinary segments, gather, resample, exchange and
 * export / import alternate freely on a handle; and nothing depends on a launch choice.  Launch forms:
 * those of asp_sa_chains_advance in either order (asp_sa_set_launch, _set_packed, _set_wide,
 * _set_field_cache and asp_sa_set_shuffled_launch are honoured, lane packing included), except that
 * the shuffled order always runs ONE team (asp_sa_set_shuffled_teams is ignored).
 * ASP_ERR_INVALID, before any device work and before any output is written: a null handle, null
 * chain_betas with repetitions > 0, an entry that is negative, NaN or infinite, an order other than 0
 * or 1, sweeps_done + num_sweeps > 2^32 - 2.  num_sweeps = 0 runs nothing and writes column 0 of the
 * trace; plans without spins and handles without chains run nothing. */
int asp_sa_chains_advance_ladder(asp_sa_chains *c, double const *chain_betas, uint32_t num_sweeps, uint32_t order,
                                 int64_t *out_trace);

/* MANY handles' ladder segments in one call ("Batched forms"; declared here beside the
 * single call, asp_sa_chains_item is described below).  Item i is exactly asp_sa_chains_advance_ladder
 * (chains, chain_betas, num_sweeps, order, out_trace): all five state arrays, sweeps_done and the trace
 * with the same bits, for any composition and order of the batch and however the items differ in
 * num_sweeps, order, sweeps_done, repetitions, seed or replica offset.  The handles share launches as in
 * asp_sa_chains_advance_batch, in the per-chain-beta forms of its kernels: order 0 — one launch per
 * wavefront count and layout class, the per-chain betas of all handles in one buffer; order 1 — segments
 * of equal length in the shared order and sweep launches, one team.  Traced items, plans with a forced
 * geometry or layout, clusters beyond a byte per position (order 0), a length no other item has
 * (order 1) and a group of one take asp_sa_chains_advance_ladder's path inside the call.  Ladder
 * batches, plain batches, single calls, gather, resample, exchange and export / import alternate freely
 * on a handle.  out_tracked_best / out_improved as in asp_sa_chains_item; asp_sa_chains_batch_last_ms
 * reports the sweep time of the call.
 * All items are validated before any device work and before any output is written; ASP_ERR_INVALID with
 * the item's index in the message: null items with count > 0, a null handle, null chain_betas with
 * repetitions > 0, an entry that is negative, NaN or infinite, an order above 1, non-zero flags, the
 * same handle twice, two handles of one plan, sweeps_done + num_sweeps > 2^32 - 2.  count = 0 needs no
 * device; handles without chains and plans without spins run nothing (column 0 of a trace is written).
 * Any OTHER error leaves the handles of the batch UNDEFINED, as for asp_sa_chains_advance_batch. */
typedef struct asp_sa_chains_ladder_item {
  asp_sa_chains *chains;
  double const *chain_betas;  /* HOST [repetitions] */
  uint32_t num_sweeps;
  uint32_t order;             /* 0 colour, 1 shuffled */
  uint32_t flags;             /* 0; anything else is ASP_ERR_INVALID */
  int64_t *out_trace;         /* NULL, or HOST [repetitions][num_sweeps + 1] */
  int64_t *out_tracked_best;  /* as asp_sa_chains_item */
  uint32_t *out_improved;
} asp_sa_chains_ladder_item;
int asp_sa_chains_advance_ladder_batch(asp_sa_chains_ladder_item const *items, uint32_t count);

/* The best configuration so far of every chain and its energy — what the closed call returns:
 * out_x[repetitions * ceil(K/64)], out_e[repetitions] (host or device pointers). */
int asp_sa_chains_result(asp_sa_chains *c, uint64_t *out_x, double *out_e);

/* Everything a continuation needs, as plain host arrays the caller allocates (any pointer may be NULL
 * on export; sweeps_done is always written): checkpoint to disk, inspect, or load into another handle
 * of the same plan with the same seed, repetitions and replica_offset (those three are the handle's,
 * not the snapshot's). */
typedef struct asp_sa_chains_snapshot {
  uint32_t sweeps_done;
  uint64_t *x_current;       /* [repetitions][ceil(K/64)], original spin order, bit set = +1 */
  uint64_t *x_best;          /* same shape */
  int64_t *tracked_current;  /* [repetitions], units of 2^-energy_scale_exp, relative to the chain's first state */
  int64_t *tracked_best;
  uint64_t *accepted;        /* accepted flips so far */
} asp_sa_chains_snapshot;
int asp_sa_chains_export(asp_sa_chains *c, asp_sa_chains_snapshot *s);
int asp_sa_chains_import(asp_sa_chains *c, asp_sa_chains_snapshot const *s);  /* all five arrays required */

/* MANY handles advanced in one call ("Batched segments") — early stopping,
 * checkpointing and re-heating for the production shape, many small clusters at once.  Item i is exactly
 * asp_sa_chains_advance(chains, betas, num_sweeps, order, out_trace): afterwards every handle holds the
 * same five state arrays and sweeps_done, bit for bit, for any composition and order of the batch and
 * however the items differ in num_sweeps, order, sweeps_done, repetitions, seed or replica offset; the
 * continuation law extends to batched segments, and single and batched segments may alternate on one
 * handle.  The handles that fit share launches the way asp_sa_anneal_batch's problems do: order 1 —
 * segments of equal length in the shared order and sweep launches of the closed batch, every handle
 * with its own first sweep index; order 0 — one launch per wavefront count and layout class.  State goes
 * in and out of all handles in one launch per direction and state type, not per handle.  Traced items,
 * plans with a forced geometry or layout, clusters beyond a byte per position (order 0) and a group of
 * one take asp_sa_chains_advance's path inside the call.
 *  - out_tracked_best / out_improved: what asp_sa_chains_export before and after the segment would
 *    tell — every chain's tracked_best after it, and the number of chains whose tracked_best fell
 *    strictly during it — gathered for the whole batch by one small kernel and one copy (no export per
 *    handle).  Items with num_sweeps = 0 get their outputs too, improved = 0.
 *  - All items are validated before any device work and before any output is written;
 *    ASP_ERR_INVALID with the item's index in the message: null items with count > 0, a null handle,
 *    null betas with num_sweeps > 0, a negative or NaN beta, an order above 1, non-zero flags, the same
 *    handle twice, two handles of one plan (a plan's work buffers serve one segment at a time),
 *    sweeps_done + num_sweeps > 2^32 - 2.  count = 0 needs no device; handles with no chains or no
 *    spins are fine.
 *  - Any OTHER error (a device or allocation failure after validation) leaves the handles of the batch
 *    UNDEFINED: some may hold the state after their segment while sweeps_done still counts the sweeps
 *    before it.  Import a snapshot into them, or destroy them; handles outside the batch are untouched. */
typedef struct asp_sa_chains_item {
  asp_sa_chains *chains;
  double const *betas;        /* num_sweeps values */
  uint32_t num_sweeps;
  uint32_t order;             /* 0 colour, 1 shuffled */
  uint32_t flags;             /* 0; anything else is ASP_ERR_INVALID */
  int64_t *out_trace;         /* NULL, or HOST [repetitions][num_sweeps + 1] as in asp_sa_chains_advance */
  int64_t *out_tracked_best;  /* NULL, or HOST [repetitions]: tracked_best after the segment */
  uint32_t *out_improved;     /* NULL, or one word: chains whose tracked_best fell strictly in this segment */
} asp_sa_chains_item;
int asp_sa_chains_advance_batch(asp_sa_chains_item const *items, uint32_t count);
/* Device time (ms) of the sweep launches of this thread's last asp_sa_chains_advance_batch call. */
float asp_sa_chains_batch_last_ms(void);

/* POPULATION ANNEALING on a handle (law "ASP-PA-1"): between two temperatures the
 * chains are reweighted by exp(-dbeta E) and resampled ON THE DEVICE, so that low-energy chains are
 * cloned into the slots of high-energy ones — no export, host arithmetic and import per handle and step.
 *
 * asp_sa_chains_gather: all five state arrays of slot j (x_current, x_best, tracked_current,
 * tracked_best, accepted) become those of slot source[j], for every j at once; source: HOST
 * [repetitions], any map (repeats, cycles, a reversal) — the primitive of user-defined schemes.
 * sweeps_done is unchanged; tracked energies are from then on relative to the first configuration of
 * the chain's LINEAGE; clones diverge afterwards because the random words of a sweep depend on the
 * slot's replica id.  ASP_ERR_INVALID, before any device work: a null handle, a null source, an entry
 * >= repetitions.
 *
 * asp_sa_chains_resample, for a handle of R chains:
 *  1. E_r = the reported energy (asp_sa_energy's double) of chain r's CURRENT configuration;
 *  2. w_r = expneg(dbeta * (E_r - min E)) with the annealer's expneg and one rounding per operation
 *     (the best chain has w = 1; dbeta * gap >= 23 gives w = 0);
 *  3. q_r = (uint64) floor(w_r 2^31), C_s = sum of q_r over r < s, T = C_R — integers from here on;
 *  4. v = word 0 of Philox4x32-10(counter (sweeps_done, draw, 0xFFFFFFFD, 0), key seed) — a counter no
 *     sweep, start or visiting order uses —, U = floor(v T / 2^32);
 *  5. systematic resampling: slot j takes source[j] = the s with R C_s <= j T + U < R C_{s+1} (source
 *     is non-decreasing, chain s gets floor or ceil of R q_s / T copies, dbeta = 0 is the identity);
 *  6. asp_sa_chains_gather with that map.
 * Outputs (HOST, each may be NULL): out_source[R], out_energy[R] (E_r before the step), out_q[R],
 * out_survivors (the number of distinct sources).  Handles with no chains or plans with no spins run
 * nothing: energies 0, q = 2^31, the identity.  ASP_ERR_INVALID: a null handle, a dbeta that is
 * negative, NaN or infinite; ASP_ERR_TOO_LARGE: more than 65536 chains (the products of step 5 fit 64
 * bits up to there); both before any device work.
 *
 * asp_sa_chains_resample_batch: many handles in one call — item i is exactly asp_sa_chains_resample
 * (chains, dbeta, draw, out_*), the same bits for any composition and order of the batch (the single
 * call IS the batch of one).  Energies run per plan on the plans' streams; weights, prefix sums,
 * selection and survivor counts are ONE launch with a workgroup per handle, the gather one launch per
 * state type over (handle, destination chain, words), and every output of the batch comes back in one
 * copy.  Validation is that of asp_sa_chains_advance_batch: every item before any device work and
 * before any output is written, the item's index in the message; null items with count > 0, non-zero
 * flags, the same handle twice and two handles of one plan are ASP_ERR_INVALID; count = 0 needs no
 * device.  Any OTHER error leaves the handles of the batch UNDEFINED, as documented there.  The first
 * gather or resample of a handle allocates a second set of its five state arrays, kept until destroy. */
int asp_sa_chains_gather(asp_sa_chains *c, uint32_t const *source);
int asp_sa_chains_resample(asp_sa_chains *c, double dbeta, uint32_t draw, uint32_t *out_source,
                           double *out_energy, uint64_t *out_q, uint32_t *out_survivors);
typedef struct asp_sa_chains_resample_item {
  asp_sa_chains *chains;
  double dbeta;             /* finite, >= 0 */
  uint32_t draw;            /* the caller's draw index (word 1 of the Philox counter) */
  uint32_t flags;           /* 0; anything else is ASP_ERR_INVALID */
  uint32_t *out_source;     /* NULL, or HOST [repetitions] */
  double *out_energy;       /* NULL, or HOST [repetitions]: reported energies before the step */
  uint64_t *out_q;          /* NULL, or HOST [repetitions]: integer weights */
  uint32_t *out_survivors;  /* NULL, or one word: distinct sources */
} asp_sa_chains_resample_item;
int asp_sa_chains_resample_batch(asp_sa_chains_resample_item const *items, uint32_t count);
/* Device time (ms) of this thread's last asp_sa_chains_resample(_batch) call: from its first launch
 * (the energies) to the end of the gather, HIP events on the call's stream. */
float asp_sa_chains_resample_last_ms(void);

/* PARALLEL TEMPERING on a handle (law "ASP-PT-1"): the slots of a handle are the rungs
 * of a temperature ladder (asp_sa_chains_advance_ladder), and a replica-exchange step swaps the
 * configurations of neighbouring rungs ON THE DEVICE.  For a handle of R chains, slot k at chain_betas[k]:
 *  1. E_r = the reported energy (asp_sa_energy's double) of chain r's CURRENT configuration — step 1 of
 *     asp_sa_chains_resample;
 *  2. the pairs are (k, k + 1) for every k = parity (mod 2) with k + 1 < R, parity 0 or 1: slots are
 *     paired by index (the caller keeps the ladder sorted; that is neither required nor checked);
 *  3. x_k = (beta_{k+1} - beta_k) * (E_k - E_{k+1}), one rounding per operation;
 *  4. the pair swaps iff x_k <= 0 or u < expneg(x_k) — the annealer's acceptance rule — with
 *     u = (v_k + 0.5) 2^-32, v_k = word 0 of Philox4x32-10(counter (k, sweeps_done, 0xFFFFFFFC, draw),
 *     key seed): a counter no proposal, start, visiting order or resampling uses.  The swap
 *     probability is min(1, exp((beta_{k+1} - beta_k)(E_{k+1} - E_k))), the standard exchange rule; a
 *     colder slot that holds the higher energy always swaps;
 *  5. source = the identity, except source[k] = k + 1 and source[k + 1] = k for a pair that swaps;
 *  6. asp_sa_chains_gather with that map: configurations move, temperatures stay with the slots; all
 *     five state arrays move (tracked energies are relative to a lineage); sweeps_done is unchanged.
 * Outputs (HOST, each may be NULL), back in one copy: out_source[R], out_energy[R] (E_r before the step),
 * out_accepted (the number of pairs that swapped).  R <= 1 or a parity without a pair: the identity,
 * accepted = 0.  Handles with no chains or plans with no spins run nothing: energies 0, the identity.
 * ASP_ERR_INVALID, before any device work and before any output is written: a null handle, null
 * chain_betas with repetitions > 0, parity > 1, an entry of chain_betas that is negative, NaN or
 * infinite.  asp_sa_last_total_ms of the plan is the device time of the step (energies to gather). */
int asp_sa_chains_exchange(asp_sa_chains *c, double const *chain_betas, uint32_t parity, uint32_t draw,
                           uint32_t *out_source, double *out_energy, uint32_t *out_accepted);

/* MANY handles' exchange steps in one call ("Batched forms"): item i is exactly
 * asp_sa_chains_exchange(chains, chain_betas, parity, draw, out_*) — steps 1-6 of ASP-PT-1 unchanged,
 * the same bits for any composition and order of the batch.  Energies run per plan on the plans'
 * streams; steps 2-5 of all handles are ONE launch over a table of rows (every slot's source and energy
 * word written by exactly one thread, one atomic add per accepted pair to the row's counter), the gather
 * one launch per state type over all handles, and energy | source | accepted of every handle come back
 * in one copy.  Validation as in asp_sa_chains_resample_batch — every item before any device work and
 * before any output is written, the item's index in the message: null items with count > 0, a null
 * handle, null chain_betas with repetitions > 0, an entry that is negative, NaN or infinite, parity > 1,
 * non-zero flags, the same handle twice, two handles of one plan.  count = 0 needs no device; handles
 * without chains and plans without spins run nothing (energies 0, the identity, accepted 0).  Any OTHER
 * error leaves the handles of the batch UNDEFINED. */
typedef struct asp_sa_chains_exchange_item {
  asp_sa_chains *chains;
  double const *chain_betas;  /* HOST [repetitions] */
  uint32_t parity, draw, flags;
  uint32_t *out_source;       /* NULL, or HOST [repetitions] */
  double *out_energy;         /* NULL, or HOST [repetitions]: reported energies before the step */
  uint32_t *out_accepted;     /* NULL, or one word: pairs that swapped */
} asp_sa_chains_exchange_item;
int asp_sa_chains_exchange_batch(asp_sa_chains_exchange_item const *items, uint32_t count);
/* Device time (ms) of this thread's last asp_sa_chains_exchange_batch call: from its first launch (the
 * energies) to the end of the gather, HIP events on the call's stream. */
float asp_sa_chains_exchange_last_ms(void);

/* ISOENERGETIC CLUSTER MOVES on a handle (law "ASP-ICM-1"; Houdayer's move): two chains
 * flip one connected cluster of the sites on which their current configurations differ — rejection-free,
 * and the only update here that is not local.  pairs: HOST u32[2 num_pairs], pair p = (a, b) =
 * (pairs[2p], pairs[2p + 1]); every slot < repetitions and named at most once over all pairs.  The caller
 * pairs slots of equal temperature (neither required nor checked).  Each pair, independently:
 *  1. d = x_current[a] XOR x_current[b] (bits from num_spins on cleared), n = popcount(d); n = 0: nothing
 *     changes for the pair (size 0, delta 0);
 *  2. v = word 0 of Philox4x32-10(counter (a, sweeps_done, 0xFFFFFFFB, draw), key seed) — a counter no
 *     proposal, start, visiting order, resampling or exchange uses —, U = floor(v n / 2^32); the seed site
 *     i0 is the U-th set bit of d in ascending site index, counted from 0;
 *  3. C = the connected component of i0 in the graph of A = offdiag(J + J^T) induced on {i : d_i = 1};
 *  4. for every i in C: acc = +0.0; for the entries of row i of A in ascending column with d_j = 0:
 *     acc = fma(A_ij, s_j^a, acc); g = acc + h_i; dE_i = s_i^a = +1 ? -2 g : 2 g; q_i = (int64)
 *     rint(dE_i 2^S), one rounding per operation as in a proposal of the annealer; Q = sum of q_i over C
 *     (replica b's sum is exactly -Q);
 *  5. x_current[a] ^= C, x_current[b] ^= C, tracked_current[a] += Q, tracked_current[b] -= Q;
 *  6. for a and for b: tracked_current < tracked_best (strictly) makes the current configuration and
 *     energy the best ones.  accepted and sweeps_done do not change; slots in no pair are untouched.
 * The same call again (same draw, no sweep in between) restores x_current and tracked_current bit for bit.
 * Outputs (HOST [num_pairs], each may be NULL), back in one copy with the touched slots' tracked energies:
 * out_differing (n), out_size (|C|), out_delta (Q).  In place, on the plan's stream.  ASP_ERR_INVALID,
 * before any device work and before any output is written: a null handle, null pairs with num_pairs > 0,
 * an entry that is not below repetitions (its index in the message), a slot named twice (both indices).
 * num_pairs = 0, a handle without chains and a plan without spins run nothing and need no device. */
int asp_sa_chains_cluster_move(asp_sa_chains *c, uint32_t const *pairs, uint32_t num_pairs, uint32_t draw,
                               uint32_t *out_differing, uint32_t *out_size, int64_t *out_delta);
/* Device time (ms) of this thread's last asp_sa_chains_cluster_move call (its kernel, HIP events on the
 * plan's stream); 0 when nothing ran. */
float asp_sa_chains_cluster_move_last_ms(void);
/* Where the move keeps its three bit planes (differing, member, frontier) per pair — for tests and timing:
 * 0 automatic (LDS when they fit, else HBM), 1 LDS (ASP_ERR_TOO_LARGE at the move when they do not fit),
 * 2 a per-pair slab in HBM.  Results never depend on it. */
int asp_sa_chains_set_cluster_planes(asp_sa_chains *c, int where);

/* MANY handles' cluster moves in one call ("Batched form"): item i is exactly
 * asp_sa_chains_cluster_move(chains, pairs, num_pairs, draw, out_*) — steps 1-6 of ASP-ICM-1 unchanged, the
 * same bits for any composition and order of the batch (every quantity of the law is a set, an integer sum
 * or a row sum in fixed column order).  One table of rows, one per (item, pair), is uploaded and at most
 * three kernels run on one stream of the call, ordered after what is pending on the plans' streams: the
 * pairs of handles of at most 32 words (2048 spins) take a WAVEFRONT each, four to a workgroup, the three
 * bit planes in 3 x 64 words of LDS; the others a workgroup each as in the single call, with the planes in
 * LDS or — asp_sa_chains_set_cluster_planes keeps its meaning per handle — in the plan's HBM slab.
 * n | size, Q and the touched slots' tracked energies of every pair come back in one copy.
 * flags: ASP_CLUSTER_NO_PACKED forces the workgroup form for the item (tests and timing; no result
 * depends on it).  Validation as in asp_sa_chains_exchange_batch — every item before any device work and
 * before any output is written, the item's index in the message: null items with count > 0, unknown
 * flags, a null handle, null pairs with num_pairs > 0, an entry that is not below repetitions, a slot
 * named twice within an item, the same handle twice, two handles of one plan.  count = 0 needs no device;
 * items with num_pairs = 0, handles without chains and plans without spins run nothing (outputs 0).  Any
 * OTHER error leaves the handles of the batch UNDEFINED. */
#define ASP_CLUSTER_NO_PACKED 1u
typedef struct asp_sa_chains_cluster_item {
  asp_sa_chains *chains;
  uint32_t const *pairs;     /* HOST u32[2 num_pairs] */
  uint32_t num_pairs, draw, flags;
  uint32_t *out_differing;   /* NULL, or HOST [num_pairs] */
  uint32_t *out_size;        /* NULL, or HOST [num_pairs] */
  int64_t *out_delta;        /* NULL, or HOST [num_pairs] */
} asp_sa_chains_cluster_item;
int asp_sa_chains_cluster_move_batch(asp_sa_chains_cluster_item const *items, uint32_t count);
/* Device time (ms) of this thread's last asp_sa_chains_cluster_move_batch call: from its first launch to
 * its last, HIP events on the call's stream; 0 when nothing ran. */
float asp_sa_chains_cluster_move_batch_last_ms(void);

/* MANY independent problems in one call — the shape of the reference's production job: tens of
 * thousands of sampled clusters, each solved with 64 repetitions x 5120 sweeps
 * (Makefile:9,115-127; experiments/sampled_connected_components.py:764-767; common.py:236-239).
 * Item i is exactly asp_sa_anneal(plan, seed, betas, num_sweeps, repetitions, replica_offset,
 * NULL, out_x, out_e): every chain is bit-identical to that call's.  The groups of all problems
 * become the workgroups of a few shared launches (one per wavefront count), so a batch of small
 * clusters fills the chip instead of leaving > 90 % of it idle launch by launch.  Plans must
 * be distinct.  Problems that need the bit-packed spin layouts, and a batch of one, take the
 * single-problem path inside the call.  Items with ASP_SA_BATCH_SHUFFLED in `flags` are
 * asp_sa_anneal_shuffled calls (a fresh visiting order every sweep): the items with the same
 * number of sweeps SHARE their launches — per chunk of sweeps one order build over (problem, sweep)
 * and one sweep launch per kernel class (chains per group, spin layout, lane packing) over
 * (problem, workgroup), workgroups of one problem on one XCD —, so a batch of small clusters fills
 * its wavefronts with chains (blocks of 4 .. 32 spins) and the chip with problems. */
#define ASP_SA_BATCH_SHUFFLED 1u
typedef struct asp_sa_batch_item {
  asp_sa_plan *plan;
  uint64_t seed;
  double const *betas;  /* num_sweeps values */
  uint32_t num_sweeps;
  uint32_t repetitions;
  uint32_t replica_offset;
  uint32_t flags;       /* 0, or ASP_SA_BATCH_SHUFFLED: the item is an asp_sa_anneal_shuffled call */
  uint64_t *out_x;      /* repetitions * ceil(K/64) words */
  double *out_e;        /* repetitions */
} asp_sa_batch_item;
int asp_sa_anneal_batch(asp_sa_batch_item const *items, uint32_t count);
/* Device time (ms) of the sweep launches of this thread's last asp_sa_anneal_batch call. */
float asp_sa_batch_last_ms(void);

/* Replaces ising_glass_annealer.greedy_solve (call site common.py:250; the only in-tree
 * description is the commented prototype at common.py:298-438): couplings are visited
 * strongest first and clusters of already-signed spins are merged so that the visited
 * coupling is satisfied (host, union-find with parity); then strict-descent sweeps
 * (flip iff dE < 0, the sweep kernel without random numbers) run on the device until no
 * spin flips or max_sweeps is reached.  Deterministic.  out_x: ceil(K/64) words. */
int asp_sa_greedy(asp_sa_plan *p, uint32_t max_sweeps, uint64_t *out_x, double *out_e,
                  uint32_t *out_sweeps);

/* Many asp_sa_greedy calls in ONE: the host trees of all items run on a small
 * thread pool inside the call (at most 8 threads), their signs are uploaded and permuted together,
 * every problem is one workgroup of a few shared launches (k_sa_descent_batch, one launch per
 * wavefront count) that leaves its sweep loop ON THE DEVICE after the first sweep that flipped
 * nothing, and configurations, energies and sweep counts come back in one copy each.
 *  - Item i's out_x and out_e are exactly what asp_sa_greedy(plan, max_sweeps, ...) returns: the
 *    same words and the same double, for any composition and order of the batch.
 *  - out_sweeps (may be NULL) is the EXACT number of sweeps performed, t: the index (from 1) of the
 *    first sweep that flipped nothing, or max_sweeps if none did.  asp_sa_greedy reports whole
 *    chunks of 8 instead: min(max_sweeps, 8 * (ceil((t - 1) / 8) + 1)) for the same problem (a
 *    fixed point of the deterministic sweep stays fixed).  max_sweeps = 0 returns the tree's
 *    configuration and its energy.
 *  - All items are validated before anything runs or any output is written: a null plan, a null
 *    out_x or out_e, flags other than 0 and two items sharing a plan are ASP_ERR_INVALID, with the
 *    item's index in the message.  count = 0 is fine (no device needed), and so are plans with
 *    K = 0 (energy 0, no sweeps, out_x untouched).
 *  - Items that do not fit the shared launches — more spins than a byte per position holds in the
 *    LDS (~1.3e5), a plan with a forced launch geometry, layout or team size, a batch of one —
 *    take asp_sa_greedy's path inside the call, team sweeps included.  Results, out_sweeps among
 *    them, never depend on which path ran.
 * A plan is used by one thread at a time, as everywhere. */
typedef struct asp_sa_greedy_item {
  asp_sa_plan *plan;
  uint32_t max_sweeps;
  uint32_t flags;        /* 0; anything else is ASP_ERR_INVALID */
  uint64_t *out_x;       /* ceil(K/64) words */
  double *out_e;         /* 1 */
  uint32_t *out_sweeps;  /* may be NULL */
} asp_sa_greedy_item;
int asp_sa_greedy_batch(asp_sa_greedy_item const *items, uint32_t count);
/* Of this thread's last asp_sa_greedy_batch call, in ms (either pointer may be NULL): wall time of
 * the host trees on the pool plus device time of the device trees (asp_sa_set_greedy_tree), and device
 * time of the descent launches (HIP events around the
 * shared launches, plus the last chunk's of every item that ran alone). */
int asp_sa_greedy_batch_last_ms(float *tree_ms, float *descent_ms);

/* Host-only: the cluster-merging half of asp_sa_greedy (no relaxation, no device). */
int asp_sa_greedy_tree_host(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                            double const *data, double const *field, uint64_t *out_x);

/* The same tree ON THE DEVICE (csrc/greedy_tree.hip): the configuration of
 * ASP-GREEDY-1's steps 1-3, ceil(K/64) words, equal to asp_sa_greedy_tree_host's word for word.  The bonds
 * are built and sorted by shared launches (a stable radix sort of ~bits(|w|)), every problem is one
 * workgroup of k_greedy_tree — the signed forest in LDS when it fits the plan's limit, in a slab of HBM
 * otherwise —, and the orientation by the field and the packing are one more launch.
 * asp_sa_greedy_tree_batch: many plans in shared launches; item i equals the single call, for any order
 * and composition of the batch.  ASP_ERR_INVALID, before any device work and before any output is
 * written: a null plan, a null out_x, the same plan twice (a batch names the item's index).  count = 0
 * needs no device; a plan with K = 0 runs nothing and leaves its out_x untouched; a plan without bonds
 * returns the field-oriented all-isolated configuration. */
int asp_sa_greedy_tree(asp_sa_plan *p, uint64_t *out_x);
int asp_sa_greedy_tree_batch(asp_sa_plan *const *plans, uint32_t count, uint64_t *const *out_x);
/* Which tree asp_sa_greedy and asp_sa_greedy_batch build for this plan (clamped to 0 .. 2): 0 the host
 * tree (default), 1 the device tree with the forest placed by size, 2 the device tree with the forest
 * forced into HBM.  A batch may mix them; results, out_sweeps included, never depend on it.  The device
 * trees of a batch's shared launches are written straight into the buffer the state permute reads. */
int asp_sa_set_greedy_tree(asp_sa_plan *p, int where);
/* Device time (ms, HIP events) of the tree launches of this thread's last asp_sa_greedy_tree(_batch),
 * asp_sa_greedy or asp_sa_greedy_batch call that built device trees; asp_sa_greedy_batch_last_ms's
 * tree_ms is the wall time of the host pool plus this.  The split (any pointer may be NULL): bonds and
 * sort, k_greedy_tree, orientation and packing. */
float asp_sa_greedy_tree_last_ms(void);
int asp_sa_greedy_tree_last_split_ms(float *bonds_sort_ms, float *tree_ms, float *orient_ms);

/* Device time (ms, HIP events on the launch stream) of the sweep kernel of the
 * last asp_sa_anneal call, and of everything device-side in that call. */
float asp_sa_last_sweep_ms(asp_sa_plan const *p);
float asp_sa_last_total_ms(asp_sa_plan const *p);

/* Diagnostics of the last asp_sa_anneal call: per chain the best tracked energy
 * (fixed point, units of 2^-S, relative to the chain's start) and the number of
 * accepted flips.  `count` = that call's repetitions.  Either may be NULL. */
int asp_sa_last_stats(asp_sa_plan const *p, uint32_t count, int64_t *tracked,
                      uint64_t *accepted);
/* Launch geometry used by the last asp_sa_anneal call. */
int asp_sa_last_launch(asp_sa_plan const *p, int *replicas_per_group, int *threads,
                       int *groups);

/* E(x) for `count` packed configurations (host in, host out). */
int asp_sa_energy(asp_sa_plan *p, uint32_t count, uint64_t const *x, double *out_e);

/* ------------------------------------------------------------------------- */
/* Bond statistics (csrc/bond_stats.hip, specification ASP-BONDS-1,          */
/* DESIGN.md 3.6): common.py:439-478, 940-960 and 963-1002 of the reference  */
/* ------------------------------------------------------------------------- */

/* A square CSR matrix J (K rows; the columns of a row unique, in any order; the diagonal and explicit
 * zeros may be stored) and one sign bit per spin (bit i of word i / 64 set: s_i = +1) kept on the
 * device.  A BOND is a stored entry with j != i and J_ij != 0 — (i, j) and (j, i) are two bonds — and
 * it is FRUSTRATED iff (s_i == s_j) == (J_ij > 0), i.e. J_ij s_i s_j > 0.  Every result is an integer
 * count, an extremum of bit patterns or a sorted copy: exact, whatever the launch geometry.
 * Host pointers.  K = 0 and a matrix without bonds are valid and give zeros; an indptr that is not
 * monotone, a column outside [0, K) and data that is not finite are ASP_ERR_INVALID, 2^30 spins or
 * more ASP_ERR_TOO_LARGE.  (That the columns of a row are unique is the caller's promise.) */
typedef struct asp_bonds asp_bonds;
typedef struct asp_bonds_summary {
  uint64_t num_spins, stored, bonds, frustrated, rows_with_bonds, strongest_frustrated;
  double max_abs, min_abs;
} asp_bonds_summary;
/* stored: entries of the matrix; max_abs and min_abs over the bonds, 0 without bonds;
 * strongest_frustrated: rows whose strongest bond is frustrated. */

/* Uploads the matrix and the signs and runs the row pass. */
int asp_bonds_create(uint64_t num_spins, int64_t const *indptr, int32_t const *indices,
                     double const *data, uint64_t const *sign_words, asp_bonds **out);
/* Other signs on the resident matrix: runs the row pass again. */
int asp_bonds_set_signs(asp_bonds *b, uint64_t const *sign_words);
int asp_bonds_get_summary(asp_bonds const *b, asp_bonds_summary *out);
/* Per row (K entries each, any pointer may be NULL): the largest |J_ij| with j != i, or 0 without a
 * bond (common.get_strongest_off_diag); the smallest column that attains it, or -1; whether that bond
 * is frustrated.  The strongest bond is the one of largest MAGNITUDE (the reference's
 * cluster_statistics takes the argmax of the signed matrix). */
int asp_bonds_rows(asp_bonds const *b, double *strongest, int32_t *strongest_col,
                   uint8_t *strongest_frustrated);
/* Bonds per bin of |J|: edges[num_bins + 1] finite and strictly ascending, 1 <= num_bins <= 4096; bin
 * k holds edges[k] <= |J| < edges[k + 1], the last bin also |J| == edges[num_bins] (np.histogram's
 * rule).  normal[num_bins] and frustrated[num_bins]; *below and *above (either may be NULL) receive
 * the bonds outside the edges. */
int asp_bonds_histogram(asp_bonds const *b, uint32_t num_bins, double const *edges, uint64_t *normal,
                        uint64_t *frustrated, uint64_t *below, uint64_t *above);
/* |J| of all bonds in descending order, bit for bit np.sort(np.abs(bonds))[::-1]; fails with
 * ASP_ERR_INVALID when capacity < summary.bonds. */
int asp_bonds_magnitudes(asp_bonds const *b, uint64_t capacity, double *out);
void asp_bonds_destroy(asp_bonds *b);
/* Device time (ms, HIP events) of the kernels of this thread's last asp_bonds_create,
 * asp_bonds_set_signs, asp_bonds_histogram, asp_bonds_magnitudes or asp_sector_bonds_create call;
 * copies between host and device are not in it. */
float asp_bonds_last_ms(void);

/* The same handle for the Ising model of a whole symmetry sector, built on the device from DEVICE
 * pointers: the ELL arrays of asp_sector_rows (slot k of row i at [k * n + i]) and the ground state.
 *   H_ij = sum, in slot order from +0.0, of val over the slots of row i with idx == j (the unused
 *          slots (i, 0.0) fall out with the diagonal); H_ji likewise from row j;
 *   M_ij = (H_ij |psi_j|) |psi_i|,  J_ij = 0.5 (M_ij + M_ji),  every operation rounded on its own;
 * row i holds the distinct targets j != i of its slots with J_ij != 0, in the order of their first
 * slot; s_i = +1 iff psi_i >= 0.  The input arrays are only read and are not needed afterwards. */
int asp_sector_bonds_create(uint64_t n, uint32_t width, uint32_t const *idx_dev, double const *val_dev,
                            double const *psi_dev, asp_bonds **out);

/* ------------------------------------------------------------------------- */
/* Sign scores (csrc/sign_scores.hip, specification ASP-SCORE-1, DESIGN.md   */
/* 3.11): common.py:211-229 of the reference for many configurations at once */
/* ------------------------------------------------------------------------- */

/* Scores of `count` packed configurations x[c * x_stride + word] of one K-spin model (bit i of word
 * i / 64 set: s_i = +1; W = ceil(K / 64) words each, x_stride >= W; bits at positions >= K are masked)
 * against exact (K0 = num_scored bits) and weights (K0 doubles, NULL: all 1.0).  Position i < K0 compares
 * bit select[i] of x with bit i of exact; select == NULL: K0 = K and the identity (num_scored is then
 * not read).  Per configuration
 *   matches = #{ i < K0 : g_i == e_i }                                   (out_matches[count], exact)
 *   signed  = the pairwise tree, strides ASCENDING 1, 2, 4, ..., over t_i = +w_i on a match and -w_i
 *             otherwise, padded with +0.0 to the next power of two       (out_signed[count])
 * and once per call total = the same tree over w_i (out_total[1]).  Every add is rounded on its own and
 * nothing is multiplied, so the bits depend on no launch choice; a zero may carry either sign.  Host
 * pointers; each output may be NULL.  Checked before any device work and before any output is written —
 * ASP_ERR_INVALID: a null x (count > 0, K > 0), exact (K0 > 0) or items; x_stride in 1 .. W - 1 (0 is W);
 * a select entry outside [0, K); a weight that is negative, NaN or infinite; ASP_ERR_TOO_LARGE:
 * K0 >= 2^31.  count = 0 needs no device and writes nothing; K0 = 0 gives matches 0 and +0.0 twice. */
int asp_sign_scores(uint64_t num_spins, uint32_t count, uint64_t const *x, uint64_t x_stride,
                    uint64_t num_scored, int32_t const *select, uint64_t const *exact,
                    double const *weights, uint64_t *out_matches, double *out_signed, double *out_total);
typedef struct asp_sign_scores_item {
  uint64_t num_spins;
  uint32_t count;
  uint64_t const *x;
  uint64_t x_stride;
  uint64_t num_scored;
  int32_t const *select;
  uint64_t const *exact;
  double const *weights;
  uint64_t *out_matches;
  double *out_signed;
  double *out_total;
} asp_sign_scores_item;
/* Many models with their configurations: one upload, launches whose number does not depend on `count`,
 * one download.  Item i receives the bits of the single call, for any order and composition of the
 * batch; a refusal names the item's index.  A batch of 0 items needs no device. */
int asp_sign_scores_batch(asp_sign_scores_item const *items, uint32_t count);
/* out[a * count + b] = popcount((x_a xor x_b) over bits < K): symmetric, zero diagonal, exact.
 * ASP_ERR_TOO_LARGE: count > 32768 or K >= 2^32. */
int asp_sign_distances(uint64_t num_spins, uint32_t count, uint64_t const *x, uint64_t x_stride, uint32_t *out);
/* The same for the configurations RESIDENT in a chains handle, in original spin order — which = 0: every
 * chain's best, 1: its current one (ASP_ERR_INVALID above 1) — without exporting them; count is the
 * handle's repetitions.  Only reads the handle: the chains after the call are bit for bit the chains
 * without it. */
int asp_sa_chains_scores(asp_sa_chains *c, uint32_t which, uint64_t num_scored, int32_t const *select,
                         uint64_t const *exact, double const *weights, uint64_t *out_matches,
                         double *out_signed, double *out_total);
int asp_sa_chains_distances(asp_sa_chains *c, uint32_t which, uint32_t *out);
/* Device time (ms, HIP events) of the kernels of this thread's last call of the five above; copies
 * between host and device are not in it. */
float asp_sign_scores_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Consensus signs (csrc/sign_vote.hip, law ASP-VOTE-1): not */
/* in the reference, which keeps the chain of lowest energy and nothing else */
/* ------------------------------------------------------------------------- */

/* One model of a vote: `count` = R packed configurations x[r * x_stride + word] of a K-spin model (the
 * bits of the scores above: W = ceil(K / 64) words each, x_stride >= W, 0 is W; bits at positions >= K
 * are ignored), weights (R doubles, NULL: all 1.0), a reference ref (W words; NULL: x[anchor]), the flag
 * align and the number of rounds.  One round with reference ref:
 *   d_r     = popcount((x_r xor ref) over bits < K)                        (out_distance[R])
 *   flip_r  = align && 2 d_r > K          (a tie does not flip)            (out_flipped[R], 0 or 1)
 *   a_ri    = bit i of x_r, xor flip_r
 *   ones_i  = #{ r : a_ri = 1 }                                            (out_ones[K], exact)
 *   plus_i  = the sum of w_r over the r with a_ri = 1, ASCENDING r from +0.0  (out_plus[K])
 *   minus_i = the same over the r with a_ri = 0                            (out_minus[K])
 *   c_i     = 1 if plus_i > minus_i, 0 if plus_i < minus_i, bit i of ref on equality (all weights
 *             zero included); the tail bits of c's last word are 0        (out_consensus[W])
 *   changed = #{ i : c_i != ref_i }                                        (out_changed[1])
 * Round t + 1 takes c of round t for ref; the outputs are those of the last round, and changed = 0 says
 * that c is a fixed point.  Every add is rounded on its own and nothing is multiplied, so the bits
 * depend on no launch choice.  align = 0 is for models with a field, where the global flip is no
 * symmetry.  Host pointers; each output may be NULL. */
typedef struct asp_sign_vote_item {
  uint64_t num_spins;
  uint32_t count;
  uint64_t const *x;
  uint64_t x_stride;
  double const *weights;
  uint64_t const *ref;
  uint32_t anchor;
  uint32_t align;
  uint32_t rounds;
  uint32_t *out_distance;
  uint8_t *out_flipped;
  uint32_t *out_ones;
  double *out_plus;
  double *out_minus;
  uint64_t *out_consensus;
  uint32_t *out_changed;
} asp_sign_vote_item;
/* Many models: one upload, two launches a round of the item with the most rounds (their number does not
 * depend on `count`), one download; the rounds follow one another on the device.  Item i receives the
 * bits of a batch of that item alone, for any order and composition of the batch.  Checked before any
 * device work and before any output is written, a refusal naming the item's index — ASP_ERR_TOO_LARGE:
 * K >= 2^31, count > 2^20; ASP_ERR_INVALID: null items; a null x (count > 0, K > 0); x_stride in
 * 1 .. W - 1; a weight that is negative, NaN or infinite; ref == NULL with anchor >= count (count > 0);
 * rounds outside 1 .. 16.  A batch of 0 items and an item with count = 0 need no device and write
 * nothing; K = 0 writes zeros to out_distance and out_flipped and changed = 0. */
int asp_sign_vote_batch(asp_sign_vote_item const *items, uint32_t count);
/* The same for the configurations RESIDENT in chains handles, in original spin order — which = 0: every
 * chain's best, 1: its current one (ASP_ERR_INVALID above 1, and for a null handle) — without exporting
 * them; K and count are the handle's spins and repetitions.  Many handles share the launches; one handle
 * is a batch of one and then runs on its plan's stream.  Only reads the handles, so the same handle may
 * appear twice, and the chains after the call are bit for bit the chains without it. */
typedef struct asp_sa_chains_vote_item {
  asp_sa_chains *chains;
  uint32_t which;
  double const *weights;
  uint64_t const *ref;
  uint32_t anchor;
  uint32_t align;
  uint32_t rounds;
  uint32_t *out_distance;
  uint8_t *out_flipped;
  uint32_t *out_ones;
  double *out_plus;
  double *out_minus;
  uint64_t *out_consensus;
  uint32_t *out_changed;
} asp_sa_chains_vote_item;
int asp_sa_chains_vote_batch(asp_sa_chains_vote_item const *items, uint32_t count);
/* Device time (ms, HIP events) of the kernels of this thread's last call of the two above; copies
 * between host and device are not in it. */
float asp_sign_vote_last_ms(void);

#ifdef __cplusplus
}
#endif
#endif /* ASP_H */
