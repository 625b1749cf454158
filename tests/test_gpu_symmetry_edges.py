"""The symmetric-basis action on the GPU (csrc/operator_apply.hip: state_info, k_source_norms,
k_symmetrise, k_symmetrise_rows, k_merge_rows, k_sym_rows) at the edges listed in
tests/symmetry_cases.py — inversion -1 with its orbits of norm 0, group sizes around the wavefront,
64 sites, tables beyond 64 KiB and 160 KiB of LDS, rows beyond 64 and 128 connections, single-site
flips — against the numpy restatement (operators.Operator.batched_apply,
symmetry.SymmetryGroup.state_info, helpers.reference_route_ising), bit for bit, with
ASP_SYMMETRISE_ROWS unset, 1 and 0.  tests/test_symmetry_cases.py checks the restatement itself and
that every case reaches its edge."""
import ctypes
import functools

import numpy as np
import pytest

import symmetry_cases as cases

pytestmark = pytest.mark.gpu

IDS = [case.name for case in cases.CASES]
OUTSIDE = tuple(case for case in cases.CASES if case.zero_norms)
INVALID = -3  # ASP_ERR_INVALID


@pytest.fixture(params=[None, "1", "0"], ids=["rows unset", "rows=1", "rows=0"])
def rows_mode(request, monkeypatch):
    """ASP_SYMMETRISE_ROWS, read by the library at every call: unset (k_symmetrise_rows when the
    group's tables fit 160 KiB of LDS), 1 (the same) and 0 (k_source_norms + k_symmetrise)."""
    if request.param is None:
        monkeypatch.delenv("ASP_SYMMETRISE_ROWS", raising=False)
    else:
        monkeypatch.setenv("ASP_SYMMETRISE_ROWS", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _ising(case):
    from helpers import reference_route_ising

    x = cases.expected(case)
    return reference_route_ising(x.operator, x.keys, x.psi)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _assert_apply(dev, op, keys):
    other, coeffs, counts = dev.apply(keys)
    want_other, want_coeffs, want_counts = op.batched_apply(keys)
    assert not np.any(want_coeffs.imag)
    assert np.array_equal(counts, want_counts) and _same(other, want_other[:, 0])
    # tobytes: the sign of a zero coefficient (a target of norm 0) included
    assert _same(coeffs, want_coeffs.real)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_state_info_equals_numpy(case, rows_mode):
    x = cases.expected(case)
    rep, character, norm = x.operator.device().state_info(x.states)
    want_rep, want_character, want_norm = x.info
    assert _same(rep, want_rep) and _same(norm, want_norm)
    inside = want_norm > 0
    assert np.array_equal(character[inside], want_character[inside])
    if x.group.spin_inversion < 0:
        assert np.any(character[inside] == -1)
        # the wrapper takes the character from the sign of character * norm: +1 at norm 0
        assert np.all(character[~inside] == 1)
    else:
        assert np.all(character == 1)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_apply_equals_numpy(case, rows_mode):
    x = cases.expected(case)
    dev = x.operator.device()
    assert not dev.unique_targets
    other, coeffs, counts = dev.apply(x.keys)
    assert np.array_equal(counts, x.counts) and _same(other, x.other)
    assert _same(coeffs, x.coeffs)
    assert np.all(np.isfinite(coeffs))
    # single rows and a slice of three: workgroups whose trailing wavefronts have no row
    k = x.keys.size
    for piece in (x.keys[:1], x.keys[k // 2:k // 2 + 1], x.keys[-1:], x.keys[k // 3:k // 3 + 3]):
        _assert_apply(dev, x.operator, piece)
    if x.high_keys is not None:  # sources at or above 2^63 (images of keys)
        _assert_apply(dev, x.operator, x.high_keys)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_extension_is_the_sorted_unique_representatives_of_non_zero_norm(case, rows_mode):
    x = cases.expected(case)
    dev = x.operator.device()
    got = dev.extend(x.keys)
    assert _same(got, x.extension)
    assert np.all(x.group.state_info(got)[2] > 0)
    for piece in (x.keys[:1], x.keys[-3:]) + (() if x.high_keys is None else (x.high_keys,)):
        other, _, _ = x.operator.batched_apply(piece)
        rep, _, norm = x.group.state_info(other[:, 0])
        assert _same(dev.extend(piece), np.unique(rep[norm > 0]))


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_coupling_build_equals_the_reference_route(case, rows_mode):
    x = cases.expected(case)
    dev = x.operator.device()
    want = _ising(case)
    assert want.nnz > x.keys.size and np.all(np.isfinite(want.data))
    row, col, val = dev.ising(x.keys, x.psi)
    assert np.all(np.isfinite(val))
    assert np.array_equal(row, want.row) and np.array_equal(col, want.col)
    assert _same(val, want.data)
    indptr, ccol, cval = dev.ising_csr(x.keys, x.psi)
    want_indptr = np.concatenate([[0], np.cumsum(np.bincount(want.row, minlength=x.keys.size))])
    assert np.array_equal(indptr, want_indptr) and np.array_equal(ccol, want.col)
    assert _same(cval, want.data)


@pytest.mark.parametrize("case", OUTSIDE, ids=[c.name for c in OUTSIDE])
def test_a_source_of_norm_zero_is_rejected(case, rows_mode):
    """One state outside the sector among the keys: the host raises ValueError; the device must
    fail with ASP_ERR_INVALID and name the sector, not divide by the zero norm."""
    from annealing_sign_problem_amd import _lib

    x = cases.expected(case)
    dev = x.operator.device()
    keys = np.unique(np.append(x.keys[:40], np.uint64(x.outside)))
    assert keys.size == min(40, x.keys.size) + 1
    psi = np.full(keys.size, 1.0 / np.sqrt(keys.size))
    with pytest.raises(ValueError, match="outside the symmetry sector"):
        x.operator.batched_apply(keys)
    for call in (lambda: dev.apply(keys), lambda: dev.ising(keys, psi), lambda: dev.ising_csr(keys, psi),
                 lambda: dev.extend(keys), lambda: dev.apply(keys[keys == np.uint64(x.outside)])):
        with pytest.raises(_lib.AspError, match="sector") as error:
            call()
        assert error.value.code == INVALID
    # the raw C calls
    lib, ptr = _lib.load(), _lib.ptr
    n, capacity = keys.size, keys.size * dev.max_connections
    other, coeffs = np.zeros(capacity, np.uint64), np.zeros(capacity, np.float64)
    counts, total = np.zeros(n, np.int64), ctypes.c_uint64(0)
    row, col = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
    indptr, nnz, count = np.zeros(n + 1, np.int64), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.asp_operator_apply(dev._handle, n, ptr(keys), capacity, ptr(other), ptr(coeffs),
                                  ptr(counts), ctypes.byref(total)) == INVALID
    assert lib.asp_operator_ising(dev._handle, n, ptr(keys), ptr(psi), capacity, ptr(row), ptr(col),
                                  ptr(coeffs), ctypes.byref(nnz)) == INVALID
    assert lib.asp_operator_ising_csr(dev._handle, n, ptr(keys), ptr(psi), capacity, ptr(indptr),
                                      ptr(col), ptr(coeffs), ctypes.byref(nnz)) == INVALID
    assert lib.asp_operator_extend(dev._handle, n, ptr(keys), capacity, ptr(other),
                                   ctypes.byref(count)) == INVALID
    assert "sector" in _lib.last_error()
    # and the handle still works
    _assert_apply(dev, x.operator, x.keys[:3])


def _log_amplitudes(spins):
    spins = np.asarray(spins, dtype=np.uint64).reshape(len(spins), -1)[:, 0]
    return np.log(np.abs(np.sin(spins.astype(np.float64) * 1e-3)) + 0.1) + 0j


@pytest.mark.parametrize("name", ["ring12 inversion -1", "ring22 inversion -1"])
def test_cluster_model_and_its_extension_in_a_minus_sector(name, rows_mode):
    """make_ising_model + make_hamiltonian_extension where connections point at orbits of norm 0:
    the extended cluster holds basis states only and its couplings are the host restatement's."""
    import scipy.sparse

    from annealing_sign_problem_amd import common
    from helpers import reference_route_ising

    x = cases.expected(cases.BY_NAME[name])
    op, group = x.operator, x.group
    start = x.keys[:2] if name.startswith("ring12") else x.keys
    model = common.make_ising_model(start, op, log_psi=_log_amplitudes(start))
    bigger = common.make_hamiltonian_extension(model, _log_amplitudes)
    other, _, _ = op.batched_apply(start)
    rep, _, norm = group.state_info(other[:, 0])
    assert np.any(norm == 0)
    assert _same(bigger.spins, np.unique(rep[norm > 0]))
    assert np.all(group.state_info(bigger.spins)[2] > 0)
    psi = np.ascontiguousarray(np.exp(_log_amplitudes(bigger.spins)).real)
    psi /= common.norm2(psi)
    want = reference_route_ising(op, bigger.spins, psi)
    got = scipy.sparse.coo_matrix(bigger.ising_hamiltonian.exchange)
    assert np.all(np.isfinite(got.data)) and got.nnz > bigger.spins.size
    assert np.array_equal(got.row, want.row) and np.array_equal(got.col, want.col)
    assert _same(got.data, want.data)
    if name.startswith("ring12"):
        # extending until nothing new appears reaches exactly the sector's 15 representatives
        for _ in range(20):
            further = common.make_hamiltonian_extension(bigger, _log_amplitudes)
            if further.spins.size == bigger.spins.size:
                break
            bigger = further
        assert bigger.spins.size == 15 and _same(bigger.spins, x.keys)
