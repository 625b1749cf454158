"""No device: the sequential restatement `eloc_law` of specification ASP-ELOC-1 in
tests/eloc_cases.py against a dense restatement (`Operator.to_sparse`), its flip invariance, the Rayleigh
identity against `Operator.expectation`, and what every case is there to reach."""
import numpy as np
import pytest

import eloc_cases as cases


def _vector(op, seed):
    rng = np.random.default_rng(seed)
    return cases.signed_amplitudes(rng, op.basis.number_states)


@pytest.mark.parametrize("name,op", cases.full_basis_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_law_is_the_dense_product_within_the_derived_bound(name, op):
    """Over a full basis nothing is missing and `hphi_r = sum_s' H_s's phi_s'`: column r of the matrix whose rows
    are the output states, i.e. `(M^T phi)_r` — for the Hermitian operators here also `(M phi)_r`.  The bound is
    `n_r * 2^-52 * sum_e |coeff_e * phi_e|` (eloc_cases.derived_bound), not a measured one."""
    states = op.basis.states
    phi = _vector(op, 3)
    hphi, eloc, missing, count, magnitude = cases.eloc_law(op, states, phi, with_terms=True)
    assert not missing.any()
    matrix = op.to_sparse().real
    dense = matrix.T @ phi
    bound = cases.derived_bound(count, magnitude)
    assert np.all(np.abs(hphi - dense) <= bound)
    assert np.all(np.abs(hphi - matrix @ phi) <= bound)  # Hermitian
    assert cases.same_bits(eloc, hphi / phi)
    # the check can fail: one amplitude changed moves a row beyond the bound
    other = phi.copy()
    other[0] *= 1.0 + 1e-9
    moved = cases.eloc_law(op, states, other)[0]
    assert np.any(np.abs(moved - dense) > bound)


@pytest.mark.parametrize("name,op", cases.full_basis_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_rayleigh_identity(name, op):
    """`sum phi_r hphi_r / sum phi_r^2` is Operator.expectation: the numerator differs from the exact one by at
    most `sum_r |phi_r| bound_r`, plus the rounding of an N-term dot product on either side."""
    states = op.basis.states
    phi = _vector(op, 5)
    hphi, _, _, count, magnitude = cases.eloc_law(op, states, phi, with_terms=True)
    energy = float(np.dot(phi, hphi) / np.dot(phi, phi))
    want = op.expectation(phi)
    assert abs(want.imag) == 0.0
    assert abs(energy - want.real) <= cases.rayleigh_bound(phi, hphi, count, magnitude)


@pytest.mark.parametrize("name", ["three segments", "empty segments", "one state in 300 segments",
                                  "4097 segments of 1-3 keys", "ring20 all-to-all, inversion -1", "single-site flips"])
def test_flipping_a_segment_leaves_eloc_and_negates_hphi_bit_for_bit(name):
    t = cases.table(name)
    hphi, eloc, missing = t.law()
    segments = sorted(set(t.row_segments.tolist()))
    chosen = segments[::2]
    f_hphi, f_eloc, f_missing = t.law(phi=cases.flipped(t, chosen))
    sign = np.where(np.isin(t.row_segments, chosen), -1.0, 1.0)
    assert cases.flip_holds(hphi, eloc, f_hphi, f_eloc, sign)
    assert np.array_equal(f_missing, missing)
    assert np.count_nonzero(sign < 0) > 0 and np.count_nonzero(hphi) > 0
    if name == "4097 segments of 1-3 keys":  # rows whose sum is exactly zero: +0.0 whatever the signs
        assert np.count_nonzero(hphi[sign < 0] == 0) > 0


def test_a_state_has_signs_of_its_own_in_every_segment():
    t = cases.table("one state in 300 segments")
    key = t.keys[t.rows.astype(np.int64)]
    assert np.unique(key).size == 1 and t.rows.size == 300
    assert np.unique(t.phi[t.rows.astype(np.int64)]).size == 300
    hphi, eloc, missing = t.law()
    sizes = np.diff(t.offsets.astype(np.int64))
    assert sizes.min() == 1 and sizes.max() > 10
    alone = sizes[t.row_segments] == 1
    # alone in its segment: only the diagonal is found
    _, _, coeffs, starts = cases.connections(t.operator, key[:1])
    count, diagonal = starts[1], coeffs[0]
    assert np.all(missing[alone] == count - 1)
    # (diagonal * phi) / phi: a product and a quotient, each rounded once
    assert diagonal != 0 and np.all(np.abs(eloc[alone] - diagonal) <= 2.0 ** -52 * abs(diagonal))
    assert np.unique(eloc).size > 100


def test_cases_reach_what_they_are_there_for():
    bonds = [cases.num_bonds(cases.table(n).operator) for n in ("kagome16 24 bonds", "j1j2 64 bonds",
                                                                "sk16 first 65 bonds", "sk16 120 bonds")]
    assert bonds == [24, 64, 65, 120]
    sk = cases.table("sk16 one row of 65 connections")
    _, _, missing, count, _ = cases.eloc_law(sk.operator, sk.keys, sk.phi, sk.offsets, sk.rows, with_terms=True)
    assert count.tolist() == [65] and missing.tolist() == [0] and sk.keys.size == 65
    assert [cases.table("kagome16 K=%d" % k).keys.size for k in cases.SIZES] == [1, 63, 64, 65, 301, 4097]
    one = cases.table("kagome16 K=1")
    reached = cases.connections(one.operator, one.keys)[3][1] - 1
    assert reached > 0 and one.law()[2].tolist() == [reached]  # everything but the diagonal is missing
    many = cases.table("4097 segments of 1-3 keys")
    sizes = np.diff(many.offsets.astype(np.int64))
    assert sizes.size == 4097 and set(sizes.tolist()) == {1, 2, 3} and many.rows.size == 4097
    assert np.unique(many.keys).size < many.keys.size  # states shared between segments
    empty = np.diff(cases.table("empty segments").offsets.astype(np.int64))
    assert empty[0] == 0 and empty[-1] == 0 and empty[2] == 0 and empty[3] == 0 and empty[1] > 0
    high = cases.table("ring64 bit 63")
    assert np.any(high.keys >> np.uint64(63))
    # list form: norm-0 targets (coefficient exactly 0, never counted), and a representative reached twice by
    # one row with both hits found
    for name in ("ring20 all-to-all, inversion -1", "ring22 inversion -1"):
        t = cases.table(name)
        inverse, other, coeffs, starts = cases.connections(t.operator, t.keys[t.rows.astype(np.int64)])
        zero = coeffs == 0
        assert zero.any() and not cases.positions(np.unique(t.keys), other[zero])[1].any()
        second = t.row_segments == 1
        assert second.any() and not t.law()[2][second].any() and t.law()[2][~second].any()
    for name in ("ring20 all-to-all, inversion -1", "single-site flips"):
        t = cases.table(name)
        inverse, other, coeffs, starts = cases.connections(t.operator, t.keys[t.rows.astype(np.int64)])
        twice = False
        for u in range(starts.size - 1):
            hit = other[starts[u]:starts[u + 1]][coeffs[starts[u]:starts[u + 1]] != 0]
            twice = twice or np.unique(hit).size < hit.size
        assert twice, name
    inverse, other, coeffs, starts = cases.connections(cases.table("ring20 all-to-all, inversion -1").operator,
                                                       cases.table("ring20 all-to-all, inversion -1").keys[:40])
    assert np.diff(starts).max() > 64  # more than one chunk of the list
    assert set(cases.NAMES) == set(cases.BUILDERS) and len(cases.NAMES) == len(cases.BUILDERS)


def test_the_header_and_the_design_state_this_law():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "asp.h")) as f:
        header = f.read()
    with open(os.path.join(root, "DESIGN.md")) as f:
        design = f.read()
    for text in (header, design):
        assert "ASP-ELOC-1" in text and "acc = acc + (coeff" in text
    assert "### 3.7 " in design


def test_awkward_targets_keep_the_rows_regular():
    t = cases.table("three segments")
    rows = np.arange(0, t.keys.size, 7, dtype=np.uint64)
    phi = cases.awkward_amplitudes(t.keys.size)
    phi[rows.astype(np.int64)] = t.phi[rows.astype(np.int64)]
    hphi, eloc, _ = t.law(phi=phi, rows=rows)
    assert np.all(np.isfinite(eloc)) and np.count_nonzero(hphi) > 0
    assert np.any(phi == 0) and np.any(np.signbit(phi) & (phi == 0)) and np.any(np.abs(phi[phi != 0]) < 1e-307)
