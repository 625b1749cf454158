"""GPU: `build_matrix`, `extract_signs` and the `asp_build_*` handle of csrc/build_matrix.hip on the
cases of tests/build_cases.py — the inputs its special paths were written for: a needle with a tail
on a table without one, key 0 and needle 0, full home buckets and the wrap past the last bucket, a
block's output position on the 64 / 2048 / 131072 boundaries, the two rows of a wavefront, rows that
do not exist, more than 64 super-chunks, subnormals, -0.0 and counts beyond 2^53
(tests/test_build_cases.py asserts on the CPU that the cases reach them and tell every named wrong
variant apart).  The checker is oracle.build_matrix / oracle.extract_signs, pinned to the reference;
everything is compared byte for byte.

Not covered: the second step (`t += 256`) of the clean-up of the other parity's super-chunk totals,
which needs more than 256 super-chunks (33 million connections), and inputs containing NaN or
infinity (tests/build_cases.py says why)."""
import ctypes
import gc

import numpy as np
import pytest

import oracle

import build_cases as cases

pytestmark = pytest.mark.gpu

OUTPUTS = ("row", "col", "elements", "field")


def _ids(table):
    return [case.name for case in table]


def _assert_same(name, got, expected):
    """(row, col, elements, field) byte for byte; the first differing entry is reported."""
    for what, mine, theirs in zip(OUTPUTS, got, expected):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape, (name, what, mine.shape, theirs.shape)
        if mine.tobytes() != theirs.tobytes():
            item = mine.dtype.itemsize
            differs = np.any(mine.view(np.uint8).reshape(-1, item) != theirs.view(np.uint8).reshape(-1, item), axis=1)
            first = int(np.nonzero(differs)[0][0])
            raise AssertionError("%s: %s differs at %d of %d entries, first at %d: %r, expected %r"
                                 % (name, what, int(differs.sum()), mine.shape[0], first, mine[first], theirs[first]))


@pytest.mark.parametrize("case", cases.BUILD_CASES, ids=_ids(cases.BUILD_CASES))
def test_build_matrix_equals_the_oracle(case):
    from annealing_sign_problem_amd import _build_matrix

    x = case.make()
    nnz, *expected = cases.build_oracle(case)
    got = _build_matrix.build_matrix(*x.args)
    assert got[0].shape[0] == nnz, (case.name, got[0].shape[0], nnz)
    _assert_same(case.name, got, expected)


def test_build_matrix_equals_the_oracle_beyond_64_super_chunks():
    """The one large case: 8.5 million connections, 65 super-chunks and a little.  Most of its time
    is the host's: making 550 MB of needles and the oracle's binary searches."""
    from annealing_sign_problem_amd import _build_matrix

    x = cases.LARGE_CASE.make()
    try:
        assert x.num_other == cases.LARGE_N > 64 * cases.SUPER
        nnz, *expected = oracle.build_matrix(*x.args)
        got = _build_matrix.build_matrix(*x.args)
        assert got[0].shape[0] == nnz
        assert np.array_equal(got[0], expected[0]) and np.array_equal(got[1], expected[1])
        _assert_same(cases.LARGE_CASE.name, got, expected)
    finally:
        del x
        gc.collect()


@pytest.mark.parametrize("case", cases.SIGN_CASES, ids=_ids(cases.SIGN_CASES))
def test_extract_signs_equals_the_oracle(case):
    """Through the reference's call shape, into words that hold garbage: every word is written
    whole, the bits above n are zero, and the word after the last is not touched."""
    from annealing_sign_problem_amd import _build_matrix as bm

    psi = np.ascontiguousarray(case.make())
    n = psi.shape[0]
    words = (n + 63) // 64
    out = np.full(words + 1, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    bm.lib.extract_signs(n, psi, out)
    expected = oracle.extract_signs(psi)
    assert np.array_equal(out[:words], expected), (case.name, np.nonzero(out[:words] != expected)[0][:5].tolist())
    assert int(out[words - 1]) >> ((n - 1) % 64 + 1) == 0
    assert out[words] == 0xDEADBEEFDEADBEEF
    assert np.array_equal(bm.extract_signs(psi), expected)


def _upload(lib, handle, x):
    from annealing_sign_problem_amd import _lib

    arrays = [np.ascontiguousarray(a) for a in x.args]
    return lib.asp_build_upload(handle, *[_lib.ptr(a) for a in arrays])


def test_build_handle_with_another_table_of_the_same_shape():
    """One handle, three super-chunks: A (single-word table) three times, B (the same K and row
    lengths, a multi-word table, other hits) twice, A once more.  Every run is the oracle's
    result, nnz included: nothing of the table before is left in the hash slots, the parity of the
    super-chunk totals swaps, and the search instantiation follows the upload.  The download
    writes the first nnz entries and nothing after them."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    by_name = {case.name: case for case in cases.BUILD_CASES}
    a, b = by_name["handle upload A"], by_name["handle upload B"]
    k, n = cases.HANDLE_K, cases.HANDLE_N
    assert -(-n // cases.SUPER) >= 2
    handle = lib.asp_build_create(ctypes.c_uint64(k), ctypes.c_uint64(n))
    assert handle
    try:
        for case, runs in ((a, 3), (b, 2), (a, 1)):
            _lib.check(_upload(lib, handle, case.make()))
            want_nnz, *expected = cases.build_oracle(case)
            assert 0 < want_nnz < n
            for run in range(runs):
                nnz = ctypes.c_uint64(0)
                _lib.check(lib.asp_build_run(handle, ctypes.byref(nnz)))
                assert nnz.value == want_nnz, (case.name, run, nnz.value, want_nnz)
                row, col = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0x5A5A5A5A, np.uint32)
                elements, field = np.full(n, -7.25), np.full(k, -7.25)
                _lib.check(lib.asp_build_download(handle, _lib.ptr(row), _lib.ptr(col), _lib.ptr(elements),
                                                  _lib.ptr(field)))
                _assert_same("%s, run %d" % (case.name, run),
                             (row[:want_nnz], col[:want_nnz], elements[:want_nnz], field), expected)
                assert np.all(row[want_nnz:] == 0xA5A5A5A5) and np.all(col[want_nnz:] == 0x5A5A5A5A)
                assert np.all(elements[want_nnz:] == -7.25)
    finally:
        lib.asp_build_destroy(handle)


def test_build_refusals_start_no_kernel():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    _lib.require_gpu()
    x = {case.name: case for case in cases.BUILD_CASES}["search K=33"].make()
    k, n = x.spins.shape[0], x.num_other
    # sizes beyond the index types: null, with a message, before anything is allocated
    for rows, connections in ((1 << 31, 0), (1, 1 << 40)):
        lib.asp_clear_error()
        assert not lib.asp_build_create(ctypes.c_uint64(rows), ctypes.c_uint64(connections))
        assert lib.asp_last_error_code() != 0 and "out of range" in _lib.last_error()
    handle = lib.asp_build_create(ctypes.c_uint64(k), ctypes.c_uint64(n + 1))
    assert handle
    try:
        nnz = ctypes.c_uint64(77)
        assert lib.asp_build_run(handle, ctypes.byref(nnz)) != 0          # nothing uploaded
        assert "before asp_build_upload" in _lib.last_error() and nnz.value == 77
        assert _upload(lib, handle, x) != 0                                # sum(other_counts) = n, not n + 1
        assert "sum(other_counts)" in _lib.last_error()
        assert lib.asp_build_run(handle, ctypes.byref(nnz)) != 0          # ... and still nothing uploaded
        assert nnz.value == 77
    finally:
        lib.asp_build_destroy(handle)
    lib.asp_clear_error()
