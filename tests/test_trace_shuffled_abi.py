"""The shuffled-order trace entry point without a GPU: the built library exports it, _lib declares
its signature, and the Python surface has the agreed defaults and validates `sweep_order` before
anything touches the library."""
import ctypes
import inspect

import numpy as np
import pytest
import scipy.sparse


def test_library_exports_the_shuffled_trace_entry_point():
    from annealing_sign_problem_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())
    assert raw.asp_sa_anneal_shuffled_trace is not None


def test_lib_declares_the_signature():
    from annealing_sign_problem_amd import _lib

    restype, argtypes = _lib.SIGNATURES["asp_sa_anneal_shuffled_trace"]
    # asp_sa_anneal_shuffled's arguments and the trace pointer behind them, as asp_sa_anneal_trace
    plain_restype, plain_argtypes = _lib.SIGNATURES["asp_sa_anneal_shuffled"]
    assert restype is plain_restype is ctypes.c_int
    assert list(argtypes) == list(plain_argtypes) + [ctypes.c_void_p]
    assert list(argtypes) == list(_lib.SIGNATURES["asp_sa_anneal_trace"][1])
    fn = _lib.load().asp_sa_anneal_shuffled_trace
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes)


def test_defaults_of_the_python_surface():
    from annealing_sign_problem_amd import annealer as sa

    assert inspect.signature(sa.anneal_with_traces).parameters["sweep_order"].default == "colour"
    traces = inspect.signature(sa.anneal_traces).parameters
    assert traces["sweep_order"].default is None
    assert traces["repetitions"].default == 1 and traces["number_sweeps"].default == 5120
    assert list(traces)[:8] == ["hamiltonian", "x0", "seed", "number_sweeps", "beta0", "beta1", "repetitions",
                                "sweep_order"]
    assert inspect.signature(sa.anneal_trace_raw).parameters["shuffled"].default is False
    assert "anneal_traces" in sa.__all__
    assert "sweep_order=None" in sa.anneal_with_traces.__doc__ and "anneal()" in sa.anneal_with_traces.__doc__


@pytest.mark.parametrize("name", ["anneal_with_traces", "anneal_traces"])
def test_a_bad_sweep_order_raises_before_the_library_is_loaded(monkeypatch, name):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    def no_library(*args, **kwargs):
        raise AssertionError("the library was loaded before 'sweep_order' was checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    ham = sa.Hamiltonian(scipy.sparse.identity(4, format="csr"), np.zeros(4))
    with pytest.raises(ValueError, match="sweep_order"):
        getattr(sa, name)(ham, seed=1, number_sweeps=4, sweep_order="bogus")
    # ... and an order that `anneal` would take from the environment is checked as well
    monkeypatch.setenv("ASP_SWEEP_ORDER", "bogus")
    with pytest.raises(ValueError, match="sweep_order"):
        getattr(sa, name)(ham, seed=1, number_sweeps=4, sweep_order=None)
