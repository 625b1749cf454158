"""csrc/sector_basis.hip and csrc/plain_basis.hip, entry by entry against the numpy / scipy host
route at the WIDTHS of the production models: sites beyond bit 32, 144 and 384 lattice maps (all
three filter passes), up to 48 sites (28 high bits), 72 and 96 transitions (both words of the row
mask), single-site flips, 16-bit low words with classes longer than a workgroup, 17 to 20 high
bits, and the degenerate ends (2 and 3 sites, weights 0 and n).  The cases are those of
tests/sector_cases.py — few states because the Hamming weight is low, not the site count —;
tests/test_sector_cases.py asserts on the CPU that they reach these paths."""
import numpy as np
import pytest

import sector_cases as cases

pytestmark = pytest.mark.gpu


def _ids(table):
    return [case.name for case in table]


def _enumerate_and_compare(case):
    from annealing_sign_problem_amd import sector_ed

    reference = cases.host(case)
    reps, norms = sector_ed.enumerate_sector(reference.operator)
    assert np.array_equal(reps.cpu().numpy().view(np.uint64), reference.states)
    assert norms.cpu().numpy().tobytes() == reference.norms.tobytes()
    return reference, reps, norms


@pytest.mark.parametrize("case", cases.SECTOR_CASES, ids=_ids(cases.SECTOR_CASES))
def test_sector_representatives_norms_and_every_matrix_element_equal_the_host_route(case):
    """Representatives and norms byte for byte; the ELL matrix (duplicates summed) against the
    transpose of `to_sparse` to 1e-13 x max|h| — every entry is the host's IEEE sequence
    (c * (chi * norm)) / norm, only the order in which equal targets are summed differs, and the
    host's diagonal carries the rounding of (d * norm) / norm —; the padding slots; one product;
    the Lanczos ground state with the bounds of tests/test_gpu_sector.py."""
    import scipy.sparse
    import torch

    from annealing_sign_problem_amd import sector_ed

    reference, reps, norms = _enumerate_and_compare(case)
    h = reference.h
    k = h.shape[0]
    matrix = sector_ed.SectorMatrix(reference.operator, reps, norms)
    assert matrix.n == k and matrix.width >= int(reference.filled.max())
    idx = matrix.idx.cpu().numpy().astype(np.int64)
    val = matrix.val.cpu().numpy()
    diag = matrix.diag.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < k
    row = np.broadcast_to(np.arange(k)[None, :], idx.shape)
    slot = np.arange(matrix.width)[:, None]
    # a row's connections fill its first slots (none of them is zero: c, chi and both norms are
    # not); every slot after them holds (i, 0.0)
    padding = slot >= reference.filled[None, :]
    assert np.all(val[~padding] != 0.0)
    assert np.array_equal(idx[padding], row[padding])
    assert np.all(val[padding] == 0.0) and not np.any(np.signbit(val[padding]))
    ell = scipy.sparse.coo_matrix((val.ravel(), (row.ravel(), idx.ravel())), shape=(k, k)).tocsr()  # sums duplicates
    assembled = ell + scipy.sparse.diags(diag, format="csr")
    difference = abs(assembled - h.T.tocsr())
    worst = float(difference.max()) if difference.nnz else 0.0
    print("%s: %d states, max |device - host| = %.3e (max |h| = %g)" % (case.name, k, worst, reference.largest))
    assert worst <= 1e-13 * reference.largest
    x = np.random.default_rng(3).standard_normal(k)
    y = matrix.matvec(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.allclose(y, h @ x, rtol=0, atol=1e-11 * reference.largest_row_sum)
    assert k >= 100   # every sector of the table is large enough for the ground-state check
    energy, _, info = sector_ed.lanczos_ground_state(matrix, tol=1e-11, max_iterations=300)
    want = reference.ground_state_energy
    assert abs(energy - want) < 1e-9 * abs(want), (energy, want)
    assert info["residual"] < 1e-7, info


@pytest.mark.parametrize("case", cases.ENUMERATION_CASES, ids=_ids(cases.ENUMERATION_CASES))
def test_spin_inversion_away_from_half_filling_lists_the_states_the_host_lists(case):
    """The inverted images have weight n - w: they are never candidates, but a candidate is
    dropped when one of them is smaller — on the device as on the host.  (The operator of such
    a basis leaves it, so there is no matrix to compare: `to_sparse` raises.)"""
    reference, reps, _ = _enumerate_and_compare(case)
    assert reps.shape[0] == reference.states.shape[0] > 0


def _plain(case):
    from annealing_sign_problem_amd import sector_ed

    reference = cases.host(case)
    matrix = sector_ed.PlainBasisMatrix(reference.operator)
    assert matrix.n == reference.states.shape[0]
    assert np.array_equal(matrix.states().cpu().numpy().view(np.uint64), reference.states)
    return reference, matrix


def _assert_columns_equal(matrix, h, which, chunk=128):
    """Columns `which` of the device's H — products with unit vectors — EQUAL those of `h`."""
    import torch

    h = h.tocsc()
    which = np.asarray(which, dtype=np.int64)
    x = torch.zeros(matrix.n, dtype=torch.float64, device="cuda")
    for start in range(0, which.shape[0], chunk):
        part = which[start:start + chunk]
        got = torch.empty((part.shape[0], matrix.n), dtype=torch.float64, device="cuda")
        for at, j in enumerate(part.tolist()):
            x[j] = 1.0
            matrix.matvec(x, out=got[at])
            x[j] = 0.0
        unequal = got.cpu().numpy().T != h[:, part].toarray()
        assert not unequal.any(), ("columns", part[np.flatnonzero(unequal.any(axis=0))][:10])


def _random_product(reference, matrix):
    import torch

    x = np.random.default_rng(2).standard_normal(matrix.n)
    y = matrix.matvec(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.allclose(y, reference.h @ x, rtol=0, atol=1e-11 * reference.largest_row_sum)


@pytest.mark.parametrize("case", cases.SMALL_PLAIN_CASES, ids=_ids(cases.SMALL_PLAIN_CASES))
def test_plain_product_of_short_chains_equals_the_host_matrix_column_by_column(case):
    """Every weight 0 .. n of 2 to 13 sites: `rank8` alone (lo_bits < 8), one-state bases.  Each
    off-diagonal entry is one product with 1.0 and the chains' elements are dyadic fractions (the
    diagonal sums are exact in any order), so the matrices are EQUAL."""
    reference, matrix = _plain(case)
    _assert_columns_equal(matrix, reference.h, np.arange(matrix.n), chunk=2048)
    matrix.release()


@pytest.mark.parametrize("case", cases.CHAIN_PLAIN_CASES, ids=_ids(cases.CHAIN_PLAIN_CASES))
def test_plain_product_with_17_and_19_high_bits_equals_the_host_route(case):
    reference, matrix = _plain(case)
    _random_product(reference, matrix)
    matrix.release()


@pytest.mark.parametrize("case", cases.LARGE_PLAIN_CASES, ids=_ids(cases.LARGE_PLAIN_CASES))
def test_plain_product_with_16_bit_low_words_equals_the_host_route(case):
    """States, a random product, whole columns — EXACTLY: the first and the last state and, for
    every populated high word, the states of its first and last rank — and the three-vector
    Lanczos with the bounds of tests/test_gpu_sector.py."""
    from annealing_sign_problem_amd import sector_ed

    reference, matrix = _plain(case)
    _random_product(reference, matrix)
    lo_bits = cases.plain_word_bits(reference.operator.basis.number_spins)[0]
    high = reference.states >> np.uint64(lo_bits)
    first = np.flatnonzero(np.concatenate([[True], high[1:] != high[:-1]]))
    last = np.concatenate([first[1:] - 1, [matrix.n - 1]])
    which = np.unique(np.concatenate([[0, matrix.n - 1], first, last]))
    _assert_columns_equal(matrix, reference.h, which)
    energy, _, info = sector_ed.lanczos_two_pass(matrix, tol=1e-10)
    want = reference.ground_state_energy
    assert abs(energy - want) < 1e-8 * abs(want), (energy, want, info)
    assert info["residual"] < 1e-6, info
    matrix.release()
