"""GPU: csrc/sparsify.hip, csrc/ising_elements.hip, csrc/key_table.hip and the device-wide scan of
csrc/asp_common.hip through their public entry points, on the cases of tests/prep_cases.py — the
sizes and values at which such kernels go wrong (tests/test_prep_cases.py asserts on the CPU that the
cases reach them and tell every named wrong variant apart).  Everything is compared exactly:
integers with array_equal, doubles byte for byte.

The scan has no entry point of its own: the `offsets` of asp_ising_elements are its <int64_t>
instantiation at every K of the table, the kept block's indptr and renumbered columns of
asp_sparsify_component its <uint32_t> instantiation."""
import ctypes

import numpy as np
import pytest

import prep_cases as cases

pytestmark = pytest.mark.gpu


def _ids(table):
    return [case.name for case in table]


def _mask_only(x, reltol):
    """asp_sparsify_component in its mask-only call shape: null outputs, capacity 0.  (The arrays
    are marshalled as common.sparsify_component marshals them, which has no such mode.)"""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    m = x.matrix
    k = m.shape[0]
    indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(m.indices, dtype=np.int32)
    data = np.ascontiguousarray(m.data, dtype=np.float64)
    frozen = np.ascontiguousarray(x.frozen, dtype=np.uint8)
    keep = np.full(k, 0xAA, dtype=np.uint8)
    kept, nnz = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(lib.asp_sparsify_component(
        ctypes.c_uint64(k), _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data), _lib.ptr(frozen),
        ctypes.c_double(float(reltol)), ctypes.c_uint64(x.anchor), _lib.ptr(keep), ctypes.byref(kept),
        ctypes.c_uint64(0), None, None, None, ctypes.byref(nnz)))
    return keep, int(kept.value), int(nnz.value)


@pytest.mark.parametrize("case", cases.SPARSIFY_CASES, ids=_ids(cases.SPARSIFY_CASES))
def test_sparsify_component_equals_the_oracle(case):
    from annealing_sign_problem_amd import common

    x = case.make()
    for reltol in x.reltols:
        keep_o, block_o = cases.sparsify_oracle(case, reltol)
        keep, block = common.sparsify_component(x.matrix, x.frozen, reltol, x.anchor)
        where = (case.name, reltol)
        assert keep.dtype == bool and np.array_equal(keep, keep_o), where
        assert block.shape == block_o.shape, where
        assert np.array_equal(block.indptr, block_o.indptr), where
        assert np.array_equal(block.indices, block_o.indices), where
        assert block.data.dtype == np.float64 and block.data.tobytes() == block_o.data.tobytes(), where
        mask, kept, nnz = _mask_only(x, reltol)
        assert np.array_equal(mask, keep_o.astype(np.uint8)), where
        assert kept == int(keep_o.sum()) and nnz == block_o.nnz, where


def test_sparsify_component_reports_a_frozen_spin_beyond_a_pruned_bridge():
    """The frozen spin that the correct law leaves outside (tests/prep_cases.frozen_bridges takes it
    out of the frozen set) is reported when it is put back, as the oracle asserts."""
    import oracle
    from annealing_sign_problem_amd import _lib, common

    case = {c.name: c for c in cases.SPARSIFY_CASES}["frozen bridges"]
    x = case.make()
    keep, _ = cases.sparsify_oracle(case, 1e-3)
    frozen = x.frozen.copy()
    frozen[np.nonzero(~keep)[0][0]] = True
    with pytest.raises(AssertionError):
        oracle.sparsify_component(x.matrix, frozen, 1e-3, x.anchor)
    with pytest.raises(_lib.AspError, match="1 frozen spins"):
        common.sparsify_component(x.matrix, frozen, 1e-3, x.anchor)


@pytest.mark.parametrize("case", cases.ISING_CASES, ids=_ids(cases.ISING_CASES))
def test_ising_elements_equal_the_restatement(case):
    from annealing_sign_problem_amd import common

    x = case.make()
    expected = cases.ising_elements(*x.args)
    got = common.ising_elements(*x.args)
    for name, mine, theirs in zip(("other_indices", "member", "elements", "offsets"), got, expected):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape, (case.name, name)
        if mine.tobytes() != theirs.tobytes():
            first = int(np.nonzero(mine.view(np.uint8).reshape(mine.shape[0], -1) !=
                                   theirs.view(np.uint8).reshape(theirs.shape[0], -1))[0][0])
            raise AssertionError("%s: %s differs first at %d: %r, expected %r"
                                 % (case.name, name, first, mine[first], theirs[first]))


@pytest.mark.parametrize("case", cases.TABLE_CASES, ids=_ids(cases.TABLE_CASES))
def test_table_index_equals_the_restatement(case):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    _lib.require_gpu()
    x = case.make()
    keys = np.ascontiguousarray(x.keys, dtype=np.uint64)
    handle = ctypes.c_void_p()
    _lib.check(lib.asp_table_create(ctypes.c_uint64(keys.shape[0]), _lib.ptr(keys), ctypes.byref(handle)))
    try:
        for queries in x.queries:
            queries = np.ascontiguousarray(queries, dtype=np.uint64)
            out = np.full(queries.shape[0], -7, dtype=np.int64)
            _lib.check(lib.asp_table_index(handle, ctypes.c_uint64(queries.shape[0]), _lib.ptr(queries),
                                           _lib.ptr(out)))
            expected = cases.table_index(keys, queries)
            assert np.array_equal(out, expected), (case.name, queries.shape[0],
                                                   np.nonzero(out != expected)[0][:5].tolist())
    finally:
        lib.asp_table_destroy(handle)
