"""tests/stencil_cases.py — the numpy restatement of ASP-STENCIL-1 that tests/test_gpu_stencil.py compares
the device with — against scipy's ``0.5 * (M + M.T)`` (make_ising_model's host route) on hand-built
connection lists: duplicate columns, explicit zeros, one-sided entries, a duplicate of the diagonal,
sums that depend on the order, -0.0, subnormals, 2^±500, targets outside the cluster.  No device."""
import numpy as np
import pytest

import stencil_cases as cases


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(cases.HAND_BUILT))
def test_the_law_equals_scipy_on_unit_amplitudes(name):
    offsets, targets, coeffs = cases.HAND_BUILT[name]
    psi = np.ones(len(offsets) - 1)
    got = cases.couplings(offsets, targets, coeffs, psi)
    want = cases.scipy_couplings(offsets, targets, coeffs, psi)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    assert np.array_equal(_bits(got[2]), _bits(want[2])), name


@pytest.mark.parametrize("name", sorted(cases.HAND_BUILT))
def test_the_law_equals_scipy_on_signed_amplitudes(name):
    """Amplitudes enter through their magnitudes, each product rounded: powers of two and odd factors."""
    offsets, targets, coeffs = cases.HAND_BUILT[name]
    n = len(offsets) - 1
    for psi in (np.array([-0.5, 2.0, -4.0][:n]), np.array([1.0 / 3.0, -0.7, 1.9][:n])):
        got = cases.couplings(offsets, targets, coeffs, psi)
        want = cases.scipy_couplings(offsets, targets, coeffs, psi)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert np.array_equal(_bits(got[2]), _bits(want[2])), name


def test_the_features_the_cases_are_named_for():
    """Each hand-built list really has what its name says — otherwise the comparison proves little."""
    one = np.ones(3)
    offsets, targets, coeffs = cases.HAND_BUILT["order-dependent"]
    mhat = cases.folds(offsets, targets, coeffs, one)
    assert mhat[(0, 1)] == 0.0 and mhat[(2, 2)] == 0.0            # 1e16 + 1 - 1e16 in connection order
    assert (coeffs[1] + coeffs[3]) + coeffs[2] == 1.0             # another order gives another number
    assert mhat[(1, 0)] in (2.0, 4.0)
    indptr, indices, data = cases.couplings(offsets, targets, coeffs, one)
    assert (2, 2) not in {(i, int(j)) for i in range(3) for j in indices[indptr[i]:indptr[i + 1]]}
    offsets, targets, coeffs = cases.HAND_BUILT["subnormals"]
    indptr, indices, data = cases.couplings(offsets, targets, coeffs, one)
    assert 0.0 in data.tolist()                                   # an entry whose half rounds to 0 stays an entry
    assert any(0.0 < v < 2.3e-308 for v in data.tolist())
    offsets, targets, coeffs = cases.HAND_BUILT["minus zero"]
    indptr, indices, data = cases.couplings(offsets, targets, coeffs, one)
    assert not np.signbit(data).any() or (data != 0.0).all()      # a fold from +0.0 never ends on -0.0
    assert np.diff(indptr).tolist() == [0, 1, 0]                  # -0.0 alone is no entry; (0, 2) + (2, 0) cancels
    offsets, targets, coeffs = cases.HAND_BUILT["large and small"]
    indptr, indices, data = cases.couplings(offsets, targets, coeffs, one)
    assert np.isfinite(data).all() and data.max() >= 2.0 ** 500 and np.abs(data).min() <= 2.0 ** -499
    offsets, targets, coeffs = cases.HAND_BUILT["one-sided"]
    indptr, indices, data = cases.couplings(offsets, targets, coeffs, one)
    assert np.array_equal(indices[indptr[1]:indptr[2]], [0, 1, 2])  # row 1 has only its diagonal connection


def test_values_on_a_given_pattern_and_pattern_changes():
    offsets, targets, coeffs = cases.HAND_BUILT["duplicate columns"]
    psi0 = np.array([0.5, -1.5, 0.75])
    indptr, indices, data0 = cases.couplings(offsets, targets, coeffs, psi0)
    # other amplitudes, the same pattern: the values of a fresh build, nothing changed
    psi = np.array([-2.0, 0.3, 1.1])
    data, changed = cases.values(offsets, targets, coeffs, psi, indptr, indices)
    fresh = cases.couplings(offsets, targets, coeffs, psi)
    assert not changed and np.array_equal(fresh[1], indices) and np.array_equal(_bits(fresh[2]), _bits(data))
    assert cases.silent_pairs(offsets, targets, indptr, indices) == {(2, 2)}  # its one connection has c = 0
    # a stored pair that now sums to exactly 0
    for zero in (0.0, -0.0):
        data, changed = cases.values(offsets, targets, coeffs, np.array([1.0, zero, 1.0]), indptr, indices)
        assert changed
    # a silent pair that fires: the pattern of psi0 = (1, 0, 1) has no row 1; psi = (1, 1, 1) has
    indptr0, indices0, _ = cases.couplings(offsets, targets, coeffs, np.array([1.0, 0.0, 1.0]))
    assert indptr0[2] == indptr0[1]
    assert (0, 1) in cases.silent_pairs(offsets, targets, indptr0, indices0)
    _, changed = cases.values(offsets, targets, coeffs, np.ones(3), indptr0, indices0)
    assert changed
    _, changed = cases.values(offsets, targets, coeffs, np.array([3.0, 0.0, -2.0]), indptr0, indices0)
    assert not changed


def test_resolve():
    keys = np.array([3, 5, 9], dtype=np.uint64)
    assert cases.resolve(keys, np.array([9, 4, 3, 10, 0, 5], dtype=np.uint64)).tolist() == [2, -1, 0, -1, -1, 1]
    assert cases.resolve(keys[:0], keys).tolist() == [-1, -1, -1]
