"""Plan re-use (include/asp.h: asp_sa_plan_reweight, asp_sa_plan_clone, asp_sa_layout_build_count,
asp_sa_plan_reweight_last_ms): what can be checked without a device — the symbols, the
header against the bindings, the null-plan refusals that run before any device work, and the counter of
the host preprocessing."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_plan_reweight", "asp_sa_plan_clone", "asp_sa_layout_build_count",
           "asp_sa_plan_reweight_last_ms")


def test_library_exports_and_header_declares_the_four_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_plan_reweight\s*\(\s*asp_sa_plan\s*\*\s*p\s*,\s*uint64_t\s+nnz\s*,\s*int64_t\s+const\s*\*"
                     r"\s*indptr\s*,\s*int32_t\s+const\s*\*\s*indices\s*,\s*double\s+const\s*\*\s*data\s*,"
                     r"\s*double\s+const\s*\*\s*field\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_plan_clone\s*\(\s*asp_sa_plan\s+const\s*\*\s*p\s*,\s*asp_sa_plan\s*\*\*\s*out\s*\)\s*;", header)
    assert re.search(r"uint64_t\s+asp_sa_layout_build_count\s*\(\s*void\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_plan_reweight_last_ms\s*\(\s*asp_sa_plan\s+const\s*\*\s*p\s*\)\s*;", header)
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_sa_plan_reweight"] == (ctypes.c_int, [p, u64, p, p, p, p])
    assert _lib.SIGNATURES["asp_sa_plan_clone"] == (ctypes.c_int, [p, ctypes.POINTER(p)])
    assert _lib.SIGNATURES["asp_sa_layout_build_count"] == (u64, [])
    assert _lib.SIGNATURES["asp_sa_plan_reweight_last_ms"] == (ctypes.c_float, [p])


def test_null_plan_is_invalid_without_a_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = lib.asp_device_touched()
    data = np.ones(1)
    assert lib.asp_sa_plan_reweight(None, ctypes.c_uint64(1), None, None, _lib.ptr(data), None) == INVALID
    assert b"null plan" in lib.asp_last_error()
    out = ctypes.c_void_p()
    assert lib.asp_sa_plan_clone(None, ctypes.byref(out)) == INVALID
    assert b"null plan" in lib.asp_last_error() and not out.value
    assert lib.asp_sa_plan_reweight_last_ms(None) == 0.0
    assert lib.asp_device_touched() == touched  # refused before any device work


def test_build_count_counts_the_host_preprocessing():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    J = scipy.sparse.csr_matrix(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, -2.0], [0.0, -2.0, 0.5]]))
    indptr, indices = J.indptr.astype(np.int64), J.indices.astype(np.int32)
    data, field = J.data.astype(np.float64), np.zeros(3)
    before = lib.asp_sa_layout_build_count()
    for done in (1, 2, 3):
        info = _lib.SaInfo()
        _lib.check(lib.asp_sa_layout_host(ctypes.c_uint64(3), _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                          _lib.ptr(field), ctypes.byref(info), None, None))
        assert lib.asp_sa_layout_build_count() == before + done
    assert info.nnz_offdiag == 4 and info.diag_sum == 0.5


def test_python_surface_and_validation_without_a_device():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, influence_of_noise

    assert issubclass(sa.PatternMismatch, ValueError) and "PatternMismatch" in sa.__all__
    for method in (sa.Hamiltonian.reweight, sa.Hamiltonian.reweighted):
        parameters = inspect.signature(method).parameters
        assert list(parameters) == ["self", "data", "field", "indptr", "indices"]
        assert all(parameters[name].default is None for name in ("field", "indptr", "indices"))
    parameters = inspect.signature(common.reweight_ising_model).parameters
    assert list(parameters) == ["model", "log_psi", "log_psi_fn", "external_field", "out"]
    parameters = inspect.signature(influence_of_noise.influence_of_noise).parameters
    assert list(parameters)[:6] == ["hamiltonian", "ground_state", "noise_levels", "repetitions", "batch", "reuse"]
    assert parameters["batch"].default == 16 and parameters["reuse"].default is True
    # a pattern that differs is refused before a plan is asked for
    ham = sa.Hamiltonian(scipy.sparse.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), np.zeros(2))
    with pytest.raises(sa.PatternMismatch):
        ham.reweight(np.ones(3))
    with pytest.raises(sa.PatternMismatch):
        ham.reweight(np.ones(2), indices=np.array([1, 1]))
    with pytest.raises(sa.PatternMismatch):
        ham.reweight(np.ones(2), indptr=np.array([0, 2, 2]))
    with pytest.raises(ValueError):
        ham.reweight(None)
    assert ham._plan is None and ham.exchange.data.tolist() == [1.0, 1.0]
