"""CPU: the numpy restatement of the bond statistics (tests/bond_cases.py, specification ASP-BONDS-1 in
DESIGN.md §3.6) against the reference's own formulas on the golden Ising models, ``bonds.log_edges``
against ``np.histogram`` in log space, the wrong readings of the law that the named cases tell apart,
and the conditions the cases must meet for the GPU tests to mean something."""
import numpy as np
import pytest
import scipy.sparse

import bond_cases
from conftest import golden

GOLDENS = ("ring4", "kagome16_cluster", "sk16_cluster")


def _golden_csr(name):
    g = golden("make_ising_%s.npz" % name)
    n = g["spins"].shape[0]
    matrix = scipy.sparse.coo_matrix((g["data"], (g["row"], g["col"])), shape=(n, n)).tocsr()
    matrix.sort_indices()
    return matrix, g["x0"], n


def _reference(matrix, x0, n):
    """common.py:975-999 of the reference, restated: the frustrated mask of the off-diagonal non-zeros,
    the log-space edges and the two 49-bin histograms."""
    signs = 2.0 * np.unpackbits(np.ascontiguousarray(x0, dtype="<u8").view(np.uint8), bitorder="little")[:n] - 1.0
    coo = matrix.tocoo()
    keep = (coo.row != coo.col) & (coo.data != 0)  # setdiag(0); eliminate_zeros()
    row, col, data = coo.row[keep], coo.col[keep], coo.data[keep]
    is_frustrated = signs[row] * signs[col] * data > 0
    max_coupling = np.log(np.max(np.abs(data)))
    min_coupling = max(max_coupling - 20, np.log(np.min(np.abs(data))))
    frustrated = np.log(np.abs(data[is_frustrated]))
    frustrated = frustrated[(min_coupling <= frustrated) & (frustrated <= max_coupling)]
    normal = np.log(np.abs(data[np.invert(is_frustrated)]))
    normal = normal[(min_coupling <= normal) & (normal <= max_coupling)]
    bins = np.linspace(min_coupling, max_coupling, 50)
    frustrated_pdf, _ = np.histogram(frustrated, bins=bins, density=False)
    normal_pdf, _ = np.histogram(normal, bins=bins, density=False)
    return data, is_frustrated, min_coupling, max_coupling, bins, normal_pdf, frustrated_pdf


@pytest.mark.parametrize("name", GOLDENS)
def test_law_reproduces_the_reference_formulas(name):
    from annealing_sign_problem_amd.bonds import log_edges

    matrix, x0, n = _golden_csr(name)
    data, is_frustrated, lo, hi, _, normal_pdf, frustrated_pdf = _reference(matrix, x0, n)
    law = bond_cases.bond_law(matrix.indptr, matrix.indices, matrix.data, x0)
    assert law["bonds"] == data.shape[0] > 0
    assert np.array_equal(law["is_frustrated"], is_frustrated)  # (both in CSR storage order)
    assert np.array_equal(law["magnitude"], np.abs(data))
    assert law["frustrated"] == np.count_nonzero(is_frustrated)
    # common.py:955-959
    assert np.array_equal(bond_cases.magnitudes_law(law), np.sort(np.abs(data))[::-1])
    assert lo < hi
    normal, frustrated, below, above = bond_cases.histogram_law(law, log_edges(lo, hi, 50))
    assert np.array_equal(normal, normal_pdf) and np.array_equal(frustrated, frustrated_pdf)
    assert above == 0 and below == data.shape[0] - int(normal_pdf.sum() + frustrated_pdf.sum())
    # get_strongest_off_diag of the reference (common.py:525-541): the largest |J_ij|, j != i
    dense = np.abs(matrix.toarray())
    np.fill_diagonal(dense, 0.0)
    assert np.array_equal(law["strongest"], dense.max(axis=1))


@pytest.mark.parametrize("name", GOLDENS)
def test_log_edges_bins_as_np_histogram_in_log_space(name):
    from annealing_sign_problem_amd.bonds import log_edges

    matrix, x0, n = _golden_csr(name)
    data, _, lo, hi, bins, _, _ = _reference(matrix, x0, n)
    edges = log_edges(lo, hi, 50)
    assert edges.shape == (50,) and np.all(np.diff(edges) >= 0)
    if name != "ring4":  # (ring4's couplings are all 1/3 up to rounding: its 50 edges span three doubles)
        assert np.all(np.diff(edges) > 0)
    for k, b in enumerate(bins[:-1]):  # the smallest double whose logarithm reaches the edge
        assert np.log(edges[k]) >= b and np.log(np.nextafter(edges[k], 0.0)) < b
    assert np.log(edges[-1]) <= bins[-1] < np.log(np.nextafter(edges[-1], np.inf))
    magnitude = np.abs(data)
    logs = np.log(magnitude)
    inside = (lo <= logs) & (logs <= hi)
    for value, log_value, is_inside in zip(magnitude, logs, inside):
        position = np.searchsorted(edges, value, side="right")
        position = 49 if value == edges[-1] else position
        if not is_inside:
            assert position < 1 or position > 49
            continue
        counts, _ = np.histogram([log_value], bins=bins)
        assert counts[position - 1] == 1 and counts.sum() == 1


def _summary(law):
    return {k: law[k] for k in ("bonds", "frustrated", "rows_with_bonds", "strongest_frustrated", "max_abs", "min_abs")}


def _differs(name, variant):
    arrays = bond_cases.cases()[name]
    right, wrong = bond_cases.law(name), bond_cases.bond_law(*arrays, variant=variant)
    return (_summary(right) != _summary(wrong) or not np.array_equal(right["strongest_col"], wrong["strongest_col"])
            or not np.array_equal(right["strongest"], wrong["strongest"])
            or not np.array_equal(right["strongest_frustrated_rows"], wrong["strongest_frustrated_rows"]))


@pytest.mark.parametrize("variant,case", [
    ("ge_zero", "stored_zeros"),
    ("diagonal_counted", "diagonal"),
    ("signed_argmax", "negative_strongest"),
    ("tie_largest_col", "tie"),
    ("row_sign_only", "k129"),
])
def test_named_case_tells_the_wrong_variant_apart(variant, case):
    assert _differs(case, variant)


def test_tie_and_negative_strongest_are_what_their_names_say():
    law = bond_cases.law("tie")
    assert law["strongest"][0] == 1.5 and law["strongest_col"][0] == 2
    assert law["strongest_col"][3] == 1 and law["strongest"][3] == 2.0  # (the diagonal 9.0 does not count)
    law = bond_cases.law("negative_strongest")
    assert law["strongest"][0] == 3.0 and law["strongest_col"][0] == 1
    law = bond_cases.law("stored_zeros")
    assert law["stored"] == 8 and law["bonds"] == 2 and law["frustrated"] == 1


# (one bin has no inner edge: '<=' on inner edges cannot show there)
_BIN_RULES = [(variant, h) for variant in ("right_open_last", "le_inner") for h in bond_cases.HISTOGRAMS
              if not (variant == "le_inner" and len(h[2]) == 2)]


@pytest.mark.parametrize("variant,histogram", _BIN_RULES, ids=["%s-%s" % (v, h[0]) for v, h in _BIN_RULES])
def test_histogram_case_tells_the_wrong_bin_rule_apart(variant, histogram):
    _, case, edges = histogram
    law = bond_cases.law(case)
    right = bond_cases.histogram_law(law, edges)
    wrong = bond_cases.histogram_law(law, edges, variant=variant)
    assert any(not np.array_equal(a, b) for a, b in zip(right, wrong))


def test_flipping_every_sign_is_a_symmetry_of_the_law():
    """'bit set <=> -1' is the one reading no case can tell apart: J_ij s_i s_j does not change when every
    sign flips.  What the convention decides is which of two DIFFERENT words a caller must pass, and
    that is checked where words are made: `pack` here is annealer.signs_to_bits bit for bit."""
    from annealing_sign_problem_amd import annealer as sa

    for name in ("k65", "k129", "row_lengths", "tie"):
        assert not _differs(name, "bit_is_minus")
    for n in (1, 63, 64, 65, 129):
        signs = np.random.default_rng(n).choice([-1.0, 1.0], size=n)
        assert np.array_equal(bond_cases.pack(signs), sa.signs_to_bits(signs))
        assert np.array_equal(bond_cases.unpack(bond_cases.pack(signs), n), signs)
    # a single flipped spin is NOT a symmetry: the bits are read per spin
    indptr, indices, data, bits = bond_cases.cases()["k65"]
    flipped = bits.copy()
    flipped[1] ^= np.uint64(1)  # spin 64, the tail word
    assert bond_cases.bond_law(indptr, indices, data, flipped)["frustrated"] != bond_cases.law("k65")["frustrated"]


def test_conditions_on_the_cases():
    cases = bond_cases.cases()
    assert {len(c[0]) - 1 for c in cases.values()} >= {0, 1, 63, 64, 65, 129}
    lengths = np.diff(cases["row_lengths"][0])
    assert lengths[:7].tolist() == [0, 1, 63, 64, 65, 129, 300]
    indptr, indices, data, _ = cases["big"]
    assert 69000 < len(indptr) - 1 < 71000 and indptr[-1] > 2 ** 20
    assert np.array_equal(np.sort(np.abs(data))[::-1][:5], np.full(5, 3.0))  # repeated magnitudes
    # unsorted columns, and columns unique within every row, in every case
    k129 = cases["k129"]
    assert any(np.any(np.diff(k129[1][a:b]) < 0) for a, b in zip(k129[0][:-1], k129[0][1:]))
    for name, (indptr, indices, data, bits) in cases.items():
        assert bits.shape[0] == (len(indptr) - 1 + 63) // 64, name
        if name != "big":
            for a, b in zip(indptr[:-1], indptr[1:]):
                assert len(set(indices[a:b].tolist())) == b - a, name
    indptr, indices, data, _ = cases["big"]
    assert scipy.sparse.csr_matrix((data, indices, indptr), shape=(len(indptr) - 1,) * 2).has_canonical_format
    a = scipy.sparse.csr_matrix(cases["non_symmetric"][2::-1], shape=(4, 4))
    assert (a != a.T).nnz > 0
    sub = bond_cases.law("subnormal")
    assert sub["min_abs"] == np.nextafter(0.0, 1.0) and sub["max_abs"] == 2e-308 < np.finfo(float).tiny
    for name in bond_cases.MIXED:
        law = bond_cases.law(name)
        assert 0.1 <= law["frustrated"] / law["bonds"] <= 0.9, name
    assert bond_cases.law("k129_all_plus")["frustrated"] not in (0, bond_cases.law("k129_all_plus")["bonds"])


@pytest.mark.parametrize("name,case,edges", bond_cases.HISTOGRAMS, ids=[h[0] for h in bond_cases.HISTOGRAMS])
def test_conditions_on_the_histogram_cases(name, case, edges):
    law = bond_cases.law(case)
    m = law["magnitude"]
    nb = len(edges) - 1
    assert nb in (1, 49, 4096) and np.all(np.diff(edges) > 0)
    normal, frustrated, below, above = bond_cases.histogram_law(law, edges)
    assert below >= 1 and above >= 1
    assert np.count_nonzero(m == edges[0]) >= 1 and np.count_nonzero(m == edges[-1]) >= 1
    if nb > 1:  # (one bin has no inner edge)
        assert np.count_nonzero(np.isin(m, edges[1:-1])) >= 1
    inside = int(normal.sum() + frustrated.sum())
    assert inside + below + above == law["bonds"]
    assert 0.1 <= inside / law["bonds"] <= 0.9
    assert normal.sum() > 0 and frustrated.sum() > 0
