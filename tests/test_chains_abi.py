"""The resumable-chains C ABI (asp_sa_chains) without a device: the header declares
the handle, the snapshot and the six entry points, the library exports them, the ctypes mirror has the
header's layout, the argument checks that need no plan return ASP_ERR_INVALID with a message and write
nothing, and the Python surface rejects wrong `x0` shapes before anything touches the library."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["asp_sa_chains_create", "asp_sa_chains_destroy", "asp_sa_chains_advance", "asp_sa_chains_result",
           "asp_sa_chains_export", "asp_sa_chains_import"]
INVALID = -3


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_the_handle_the_snapshot_and_the_entry_points():
    header = _header()
    assert re.search(r"typedef struct asp_sa_chains asp_sa_chains;", header)
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
    assert re.search(r"int\s+asp_sa_chains_create\s*\(\s*asp_sa_plan \*p,\s*uint64_t seed,\s*uint32_t repetitions,\s*"
                     r"uint32_t replica_offset,\s*uint64_t const \*x0,\s*uint64_t x0_stride,\s*asp_sa_chains \*\*out\s*\)",
                     header)
    assert re.search(r"int\s+asp_sa_chains_advance\s*\(\s*asp_sa_chains \*c,\s*double const \*betas,\s*"
                     r"uint32_t num_sweeps,\s*uint32_t order,\s*int64_t \*out_trace\s*\)", header)
    body = re.search(r"typedef struct asp_sa_chains_snapshot \{(.*?)\} asp_sa_chains_snapshot;", header, flags=re.S)
    assert body, "include/asp.h does not declare asp_sa_chains_snapshot"
    assert re.findall(r"(\w+)\s*;", body.group(1)) == ["sweeps_done", "x_current", "x_best", "tracked_current",
                                                        "tracked_best", "accepted"]


def test_library_exports_the_symbols_and_lib_declares_them():
    from annealing_sign_problem_amd import _lib

    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()  # resolves every symbol of SIGNATURES or raises
    raw = ctypes.CDLL(_lib.library_path())
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        restype, argtypes = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == list(argtypes)
    assert _lib.SIGNATURES["asp_sa_chains_destroy"][0] is None
    assert all(_lib.SIGNATURES[name][0] is ctypes.c_int for name in SYMBOLS if name != "asp_sa_chains_destroy")


def test_ctypes_snapshot_mirrors_the_header():
    from annealing_sign_problem_amd import _lib

    fields = _lib.SaChainsSnapshot._fields_
    assert [name for name, _ in fields] == ["sweeps_done", "x_current", "x_best", "tracked_current", "tracked_best",
                                            "accepted"]
    assert fields[0][1] is ctypes.c_uint32 and all(t is ctypes.c_void_p for _, t in fields[1:])
    # a 32-bit counter, padding, five pointers
    assert _lib.SaChainsSnapshot.x_current.offset == 8 and ctypes.sizeof(_lib.SaChainsSnapshot) == 48


def test_null_arguments_are_invalid_without_a_device_and_write_nothing():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()

    def invalid(rc, word):
        assert rc == INVALID and lib.asp_last_error_code() == INVALID
        assert word in _lib.last_error(), _lib.last_error()

    handle = ctypes.c_void_p(0x5A5A)  # must stay as it is: nothing is written on failure
    invalid(lib.asp_sa_chains_create(None, ctypes.c_uint64(1), ctypes.c_uint32(4), ctypes.c_uint32(0), None,
                                     ctypes.c_uint64(0), ctypes.byref(handle)), "plan")
    assert handle.value == 0x5A5A
    betas = np.ones(4)
    trace = np.full((1, 5), 77, dtype=np.int64)
    invalid(lib.asp_sa_chains_advance(None, _lib.ptr(betas), ctypes.c_uint32(4), ctypes.c_uint32(0), _lib.ptr(trace)),
            "handle")
    assert np.all(trace == 77)
    xs, es = np.full(3, 5, dtype=np.uint64), np.full(3, 5.0)
    invalid(lib.asp_sa_chains_result(None, _lib.ptr(xs), _lib.ptr(es)), "handle")
    assert np.all(xs == 5) and np.all(es == 5.0)
    snap = _lib.SaChainsSnapshot()
    snap.sweeps_done = 123
    invalid(lib.asp_sa_chains_export(None, ctypes.byref(snap)), "handle")
    invalid(lib.asp_sa_chains_import(None, ctypes.byref(snap)), "handle")
    assert snap.sweeps_done == 123
    lib.asp_sa_chains_destroy(None)  # like free(NULL)
    assert _lib.gpu_touched() == touched  # none of it asked for the GPU
    lib.asp_clear_error()


def test_python_surface():
    import annealing_sign_problem_amd as pkg
    from annealing_sign_problem_amd import annealer as sa

    assert pkg.Chains is sa.Chains and pkg.anneal_until is sa.anneal_until
    assert "Chains" in sa.__all__ and "anneal_until" in sa.__all__
    init = inspect.signature(sa.Chains.__init__).parameters
    assert list(init) == ["self", "hamiltonian", "seed", "repetitions", "x0", "replica_offset"]
    assert init["seed"].default is None and init["repetitions"].default == 1 and init["x0"].default is None
    assert init["replica_offset"].default == 0
    advance = inspect.signature(sa.Chains.advance).parameters
    assert list(advance) == ["self", "betas", "sweep_order", "trace"]
    assert advance["sweep_order"].default is None and advance["trace"].default is False
    assert inspect.signature(sa.Chains.result).parameters["only_best"].default is False
    for member in ("state", "load_state", "close", "sweeps_done"):
        assert hasattr(sa.Chains, member)
    until = inspect.signature(sa.anneal_until).parameters
    for name in ("number_sweeps", "check_every", "patience", "repetitions", "sweep_order", "x0", "seed"):
        assert name in until
    assert until["patience"].default is None


def _no_library(monkeypatch):
    from annealing_sign_problem_amd import _lib

    def no_library(*args, **kwargs):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)


@pytest.mark.parametrize("shape", [(1,), (3,), (2, 2), (5, 1), (4, 2, 2), (4, 3)])
def test_chains_rejects_wrong_x0_shapes_before_the_library_is_loaded(monkeypatch, shape):
    from annealing_sign_problem_amd import annealer as sa

    _no_library(monkeypatch)
    ham = sa.Hamiltonian(scipy.sparse.identity(100, format="csr"), np.zeros(100))  # 2 words
    with pytest.raises(ValueError, match="x0"):
        sa.Chains(ham, seed=1, repetitions=4, x0=np.zeros(shape, dtype=np.uint64))


def test_chains_and_anneal_until_check_their_other_arguments_first(monkeypatch):
    from annealing_sign_problem_amd import annealer as sa

    _no_library(monkeypatch)
    ham = sa.Hamiltonian(scipy.sparse.identity(4, format="csr"), np.zeros(4))
    with pytest.raises(ValueError, match="repetitions"):
        sa.Chains(ham, seed=1, repetitions=0)
    with pytest.raises(TypeError):
        sa.Chains(object())
    with pytest.raises(ValueError, match="sweep_order"):
        sa.anneal_until(ham, seed=1, number_sweeps=8, check_every=4, sweep_order="bogus")
    with pytest.raises(ValueError, match="check_every"):
        sa.anneal_until(ham, seed=1, number_sweeps=8, check_every=0)
    with pytest.raises(ValueError, match="patience"):
        sa.anneal_until(ham, seed=1, number_sweeps=8, check_every=4, patience=0)
