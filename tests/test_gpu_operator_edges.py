"""GPU: the plain-basis half of csrc/operator_apply.hip — `asp_operator_apply`, `asp_operator_ising`,
`asp_operator_ising_csr`, `asp_operator_extend` without a symmetry group — on the cases of
tests/operator_cases.py: the key hash's wrapped chain, equal fingerprints and key 0; bond counts
around the 64-lane chunk; the diagonal's order of summation; rows of more than 64 and 128 couplings;
three kept entries per lane; reverse-only pairs and the retry loop of `DeviceOperator.ising`;
cancelled pairs, -0.0 elements; the duplicate-keeping route without a group; K, n and N on the
workgroup and scan-tile sizes; the extension on unsorted input, the all-ones key, 2 and 33 sites;
2016 bonds (tests/test_operator_cases.py asserts on the CPU that the cases reach all that and tell
every named wrong variant apart).  The laws are the numpy restatements of that module, equal to the
oracle and to the reference route bit for bit; integers are compared with array_equal, doubles byte
for byte: the specification fixes the arithmetic, there is no tolerance."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import operator_cases as cases

pytestmark = pytest.mark.gpu

IDS = [case.name for case in cases.CASES]
GUARD_U64 = 0xA5A5A5A5A5A5A5A5
GUARD_I32 = -0x5A5A5A5B          # the bytes 0xA5A5A5A5
GUARD_I64 = -0x5A5A5A5A5A5A5A5B  # the bytes 0xA5 ... A5
GUARD_F64 = -7.25


def _assert_same(name, what, mine, theirs):
    """Byte for byte; the first differing entry is reported."""
    mine, theirs = np.ascontiguousarray(mine), np.ascontiguousarray(theirs)
    assert mine.dtype == theirs.dtype and mine.shape == theirs.shape, (name, what, mine.dtype, theirs.dtype,
                                                                       mine.shape, theirs.shape)
    if mine.tobytes() != theirs.tobytes():
        item = mine.dtype.itemsize
        differs = np.any(mine.view(np.uint8).reshape(-1, item) != theirs.view(np.uint8).reshape(-1, item), axis=1)
        first = int(np.nonzero(differs)[0][0])
        raise AssertionError("%s: %s differs at %d of %d entries, first at %d: %r, expected %r"
                             % (name, what, int(differs.sum()), mine.shape[0], first, mine[first], theirs[first]))


def _refused(x, call):
    from annealing_sign_problem_amd import _lib

    code, words = x.refusal
    with pytest.raises(_lib.AspError, match=words) as caught:
        call()
    assert caught.value.code == code


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_apply_equals_the_law(case):
    x, e = case.make(), cases.expected(case.name)
    dev = x.operator.device()
    assert dev.unique_targets == (cases.flip_owner(x.table) is not None)
    assert dev.max_connections == cases.max_connections(x.table)
    other, coeffs, counts = dev.apply(x.keys)
    _assert_same(case.name, "other_counts", counts, e.counts)
    _assert_same(case.name, "other_keys", other, e.other)
    _assert_same(case.name, "other_coeffs", coeffs, e.coeffs)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_ising_equals_the_law(case):
    x, e = case.make(), cases.expected(case.name)
    dev = x.operator.device()
    if x.refusal:
        return _refused(x, lambda: dev.ising(x.keys, x.psi))
    row, col, val = dev.ising(x.keys, x.psi)
    assert row.shape[0] == e.row.shape[0], (case.name, row.shape[0], e.row.shape[0])
    _assert_same(case.name, "row", row, e.row)
    _assert_same(case.name, "col", col, e.col)
    _assert_same(case.name, "val", val, e.val)
    if case.name.startswith("reverse-only"):
        # more couplings than the first capacity of DeviceOperator.ising: its retry loop ran
        assert val.shape[0] > x.keys.shape[0] * dev.max_connections


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_ising_csr_equals_the_law(case):
    x, e = case.make(), cases.expected(case.name)
    dev = x.operator.device()
    if x.refusal:
        return _refused(x, lambda: dev.ising_csr(x.keys, x.psi))
    indptr, col, val = dev.ising_csr(x.keys, x.psi)
    _assert_same(case.name, "indptr", indptr, e.indptr)
    assert indptr[x.keys.shape[0]] == val.shape[0] == e.val.shape[0]
    _assert_same(case.name, "col", col, e.col)
    _assert_same(case.name, "val", val, e.val)
    if case.name.startswith("reverse-only"):
        assert val.shape[0] > x.keys.shape[0] * dev.max_connections


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_extend_equals_the_law(case):
    x, e = case.make(), cases.expected(case.name)
    _assert_same(case.name, "extension", x.operator.device().extend(x.extend_keys), e.extension)


# -- make_ising_model, whichever route it takes ------------------------------------------------------
def _log_amplitudes(psi):
    """Complex logarithms whose exponentials have the signs of psi (no zeros among them)."""
    assert np.all(psi != 0)
    return np.log(np.abs(psi)) + 1j * np.pi * (psi < 0)


def _normalised(log_psi):
    from annealing_sign_problem_amd import common

    psi = np.ascontiguousarray(np.exp(log_psi, dtype=np.complex128).real)   # what make_ising_model sees
    return psi / common.norm2(psi)


def _assert_model_is_the_law(name, model, table, keys, psi):
    row, col, val = cases.ising(table, keys, psi)
    m = scipy.sparse.coo_matrix(model.ising_hamiltonian.exchange)
    assert np.array_equal(m.row, row) and np.array_equal(m.col, col), name
    _assert_same(name, "J", m.data, val)
    assert np.array_equal(model.spins, keys)


@pytest.mark.parametrize("name", cases.END_TO_END)
def test_make_ising_model_returns_the_law(name):
    """The fused build where it applies (through the retry loop for the reverse-only operators), the
    host route where the device refuses (a missing mirror, 2016 bonds): J is the law's either way;
    and the same through reweight_ising_model and the segmented make_ising_models."""
    from annealing_sign_problem_amd import common

    x = cases.BY_NAME[name].make()
    log_psi = _log_amplitudes(x.psi)
    psi = _normalised(log_psi)
    model = common.make_ising_model(x.keys, x.operator, log_psi=log_psi)
    _assert_model_is_the_law(name, model, x.table, x.keys, psi)
    again = _log_amplitudes(x.psi[::-1].copy())
    reweighted = common.reweight_ising_model(model, log_psi=again)
    _assert_model_is_the_law(name + ", reweighted", reweighted, x.table, x.keys, _normalised(again))
    half = x.keys.shape[0] // 2
    models = common.make_ising_models([x.keys, x.keys[:half]], x.operator, log_psis=[log_psi, log_psi[:half]])
    _assert_model_is_the_law(name + ", segment 0", models[0], x.table, x.keys, psi)
    _assert_model_is_the_law(name + ", segment 1", models[1], x.table, x.keys[:half], _normalised(log_psi[:half]))


def test_other_size_refusals_are_not_turned_into_the_host_route():
    """Only the LDS refusal of the emit pass is; every other ASP_ERR_TOO_LARGE stays an error."""
    from annealing_sign_problem_amd import _lib, common

    assert common._takes_host_route(_lib.AspError(-3, "couplings have no mirror element"))
    assert common._takes_host_route(_lib.AspError(-4, "2016 bonds need 290400 bytes of LDS per workgroup"))
    assert not common._takes_host_route(_lib.AspError(-4, "more than 2^31-1 spins"))
    assert not common._takes_host_route(_lib.AspError(-2, "a HIP call failed"))
    assert not common._takes_host_route(_lib.AspError(-5, "out of memory"))


# -- the capacity protocol of the C calls, into guard-filled buffers -----------------------------------
class _Raw:
    def __init__(self, name):
        from annealing_sign_problem_amd import _lib

        self._lib = _lib
        self.lib = _lib.load()
        self.x, self.e = cases.BY_NAME[name].make(), cases.expected(name)
        self.handle = self.x.operator.device()._handle
        self.keys = np.ascontiguousarray(self.x.keys)
        self.psi = np.ascontiguousarray(self.x.psi)
        self.k = self.keys.shape[0]

    def ptr(self, a):
        return self._lib.ptr(a)

    def apply(self, capacity, other, coeffs, counts):
        total = ctypes.c_uint64(GUARD_U64)
        rc = self.lib.asp_operator_apply(self.handle, self.k, self.ptr(self.keys), capacity, self.ptr(other),
                                         self.ptr(coeffs), self.ptr(counts), ctypes.byref(total))
        return rc, int(total.value)

    def ising(self, capacity, row, col, val):
        nnz = ctypes.c_uint64(GUARD_U64)
        rc = self.lib.asp_operator_ising(self.handle, self.k, self.ptr(self.keys), self.ptr(self.psi), capacity,
                                         self.ptr(row), self.ptr(col), self.ptr(val), ctypes.byref(nnz))
        return rc, int(nnz.value)

    def ising_csr(self, capacity, indptr, col, val):
        nnz = ctypes.c_uint64(GUARD_U64)
        rc = self.lib.asp_operator_ising_csr(self.handle, self.k, self.ptr(self.keys), self.ptr(self.psi), capacity,
                                             self.ptr(indptr), self.ptr(col), self.ptr(val), ctypes.byref(nnz))
        return rc, int(nnz.value)

    def extend(self, keys, capacity, out):
        count = ctypes.c_uint64(GUARD_U64)
        rc = self.lib.asp_operator_extend(self.handle, keys.shape[0], self.ptr(keys), capacity, self.ptr(out),
                                          ctypes.byref(count))
        return rc, int(count.value)


def _guards(size):
    return (np.full(size, GUARD_U64, np.uint64), np.full(size, GUARD_I32, np.int32), np.full(size, GUARD_I64, np.int64),
            np.full(size, GUARD_F64, np.float64))


def _untouched(*arrays):
    return all(np.all(a == {np.dtype(np.uint64): GUARD_U64, np.dtype(np.int32): GUARD_I32,
                            np.dtype(np.int64): GUARD_I64, np.dtype(np.float64): GUARD_F64}[a.dtype]) for a in arrays)


@pytest.mark.parametrize("name", cases.RAW)
def test_apply_capacity_protocol(name):
    raw = _Raw(name)
    e, n = raw.e, int(raw.e.other.shape[0])
    counts = np.full(raw.k, GUARD_I64, np.int64)
    assert raw.apply(0, None, None, counts) == (0, n)                          # the sizing call
    assert np.array_equal(counts, e.counts)
    for capacity in (n - 1, 0):                                                # refused: one short, and none at all
        other, _, _, coeffs = _guards(n + 5)
        counts = np.full(raw.k, GUARD_I64, np.int64)
        assert raw.apply(capacity, other, coeffs, counts) == (-3, n)
        assert "do not fit" in raw._lib.last_error()
        assert _untouched(other, coeffs) and np.array_equal(counts, e.counts)  # (asp.h: counts and total are written)
        for capacity_ok, with_counts in ((n, True), (n + 5, True), (n, False)):   # ... and the handle still answers
            other, _, _, coeffs = _guards(n + 5)
            counts = np.full(raw.k, GUARD_I64, np.int64) if with_counts else None
            assert raw.apply(capacity_ok, other, coeffs, counts) == (0, n)
            _assert_same(name, "other_keys", other[:n], e.other)
            _assert_same(name, "other_coeffs", coeffs[:n], e.coeffs)
            assert _untouched(other[n:], coeffs[n:])                           # nothing past the count
            assert counts is None or np.array_equal(counts, e.counts)


@pytest.mark.parametrize("name", cases.RAW)
def test_ising_capacity_protocol(name):
    raw = _Raw(name)
    e, nnz = raw.e, int(raw.e.val.shape[0])
    assert nnz > 1
    assert raw.ising(0, None, None, None) == (0, nnz)                          # the sizing call
    for capacity in (nnz - 1, 1):
        _, row, _, val = _guards(nnz + 5)
        col = row.copy()
        assert raw.ising(capacity, row, col, val) == (-3, nnz)
        assert "do not fit" in raw._lib.last_error()
        assert _untouched(row, col, val)
        for capacity_ok in (nnz, nnz + 5):
            _, row, _, val = _guards(nnz + 5)
            col = row.copy()
            assert raw.ising(capacity_ok, row, col, val) == (0, nnz)
            _assert_same(name, "row", row[:nnz], e.row)
            _assert_same(name, "col", col[:nnz], e.col)
            _assert_same(name, "val", val[:nnz], e.val)
            assert _untouched(row[nnz:], col[nnz:], val[nnz:])


@pytest.mark.parametrize("name", cases.RAW)
def test_ising_csr_capacity_protocol(name):
    raw = _Raw(name)
    e, nnz = raw.e, int(raw.e.val.shape[0])
    assert raw.ising_csr(0, None, None, None) == (0, nnz)                      # the sizing call
    for capacity in (nnz - 1, 1):
        _, col, indptr, val = _guards(nnz + 5)
        indptr = indptr[:raw.k + 2].copy()
        assert raw.ising_csr(capacity, indptr, col, val) == (-3, nnz)
        assert _untouched(indptr, col, val)
        for capacity_ok in (nnz, nnz + 5):
            _, col, indptr, val = _guards(nnz + 5)
            indptr = np.full(raw.k + 2, GUARD_I64, np.int64)
            assert raw.ising_csr(capacity_ok, indptr, col, val) == (0, nnz)
            _assert_same(name, "indptr", indptr[:raw.k + 1], e.indptr)
            assert indptr[raw.k] == nnz and indptr[raw.k + 1] == GUARD_I64
            _assert_same(name, "col", col[:nnz], e.col)
            _assert_same(name, "val", val[:nnz], e.val)
            assert _untouched(col[nnz:], val[nnz:])


@pytest.mark.parametrize("name", cases.RAW + ("extension: unsorted input with repeats",))
def test_extend_capacity_protocol(name):
    raw = _Raw(name)
    keys = np.ascontiguousarray(raw.x.extend_keys)
    e, count = raw.e, int(raw.e.extension.shape[0])
    assert raw.extend(keys, 0, None) == (0, count)                             # the sizing call
    for capacity in (count - 1, 1):
        out = np.full(count + 5, GUARD_U64, np.uint64)
        assert raw.extend(keys, capacity, out) == (-3, count)
        assert "do not fit" in raw._lib.last_error() and _untouched(out)
        for capacity_ok in (count, count + 5):
            out = np.full(count + 5, GUARD_U64, np.uint64)
            assert raw.extend(keys, capacity_ok, out) == (0, count)
            _assert_same(name, "extension", out[:count], e.extension)
            assert _untouched(out[count:])


def test_extend_refuses_keys_beyond_the_sites():
    """The set is sorted on the bits [0, number_spins): a key with a higher bit would come out in
    the wrong place.  Refused with ASP_ERR_INVALID before any launch; the handle still answers."""
    raw = _Raw("extension: 33 sites")
    assert raw.x.number_spins == 33
    keys = np.ascontiguousarray(raw.x.extend_keys)
    for bad in (1 << 33, 1 << 63, (1 << 33) | int(keys[0])):
        spoiled = keys.copy()
        spoiled[len(spoiled) // 2] = bad
        out = np.full(raw.e.extension.shape[0], GUARD_U64, np.uint64)
        assert raw.extend(spoiled, out.shape[0], out) == (-3, 0)
        assert "at or above site 33" in raw._lib.last_error() and _untouched(out)
        assert raw.extend(spoiled, 0, None) == (-3, 0)                         # the sizing call too
    out = np.full(raw.e.extension.shape[0], GUARD_U64, np.uint64)
    assert raw.extend(keys, out.shape[0], out) == (0, out.shape[0])
    _assert_same("extension: 33 sites", "extension", out, raw.e.extension)
    # 64 sites: every key is legal
    top = _Raw("full matrices, 32 bonds, 64 sites")
    out = np.full(top.e.extension.shape[0], GUARD_U64, np.uint64)
    assert top.extend(np.ascontiguousarray(top.x.extend_keys), out.shape[0], out) == (0, out.shape[0])
    _assert_same("64 sites", "extension", out, top.e.extension)
