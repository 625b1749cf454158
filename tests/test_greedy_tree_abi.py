"""The C ABI of the device tree of the greedy solver (include/asp.h) without a device: the
symbols, the header against the bindings, the validation that runs before any device work and before any
output is written, and the Python keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_greedy_tree", "asp_sa_greedy_tree_batch", "asp_sa_set_greedy_tree", "asp_sa_greedy_tree_last_ms",
           "asp_sa_greedy_tree_last_split_ms")
SENTINEL = np.uint64(0xABCDABCDABCDABCD)


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and getattr(raw, name) is not None, name
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+asp_sa_greedy_tree\s*\(\s*asp_sa_plan\s*\*\s*p\s*,\s*uint64_t\s*\*\s*out_x\s*\)\s*;", header)
    assert re.search(r"\bint\s+asp_sa_greedy_tree_batch\s*\(\s*asp_sa_plan\s*\*\s*const\s*\*\s*plans\s*,\s*uint32_t\s+count\s*,"
                     r"\s*uint64_t\s*\*\s*const\s*\*\s*out_x\s*\)\s*;", header)
    assert re.search(r"\bint\s+asp_sa_set_greedy_tree\s*\(\s*asp_sa_plan\s*\*\s*p\s*,\s*int\s+where\s*\)\s*;", header)
    assert re.search(r"\bfloat\s+asp_sa_greedy_tree_last_ms\s*\(\s*void\s*\)\s*;", header)
    p, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert _lib.SIGNATURES["asp_sa_greedy_tree"] == (ctypes.c_int, [p, p])
    assert _lib.SIGNATURES["asp_sa_greedy_tree_batch"] == (ctypes.c_int, [p, u32, p])
    assert _lib.SIGNATURES["asp_sa_set_greedy_tree"] == (ctypes.c_int, [p, ctypes.c_int])
    assert _lib.SIGNATURES["asp_sa_greedy_tree_last_ms"] == (ctypes.c_float, [])
    # the greedy item keeps "flags: 0 or invalid"; the tree is a setting of the plan
    assert "ASP-GREEDY-1" in _header() and "0; anything else is ASP_ERR_INVALID" in _header()


def test_validation_runs_before_any_device_work_and_before_any_output():
    """Null plans, null outputs and the same plan twice are ASP_ERR_INVALID (a batch names the item); the
    checks look at the pointers only, so plans that do not exist will do."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    x = np.full(4, SENTINEL, dtype=np.uint64)
    y = np.full(4, SENTINEL, dtype=np.uint64)
    fake_a, fake_b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)  # (never dereferenced: a check fails first)
    assert lib.asp_sa_greedy_tree(None, _lib.ptr(x)) == INVALID and "null plan" in _lib.last_error()
    assert lib.asp_sa_greedy_tree(fake_a, None) == INVALID and "null output" in _lib.last_error()
    assert lib.asp_sa_set_greedy_tree(None, ctypes.c_int(1)) == INVALID and "null plan" in _lib.last_error()

    def batch(plans, outs):
        n = len(plans)
        c_plans, c_outs = (ctypes.c_void_p * n)(*plans), (ctypes.c_void_p * n)(*outs)
        rc = lib.asp_sa_greedy_tree_batch(c_plans, ctypes.c_uint32(n), c_outs)
        return rc, _lib.last_error()

    rc, message = batch([fake_a, None], [x.ctypes.data, y.ctypes.data])
    assert rc == INVALID and "item 1" in message and "null plan" in message
    rc, message = batch([fake_a, fake_b], [x.ctypes.data, None])
    assert rc == INVALID and "item 1" in message and "null output" in message
    rc, message = batch([fake_a, fake_b, fake_a], [x.ctypes.data, y.ctypes.data, x.ctypes.data])
    assert rc == INVALID and "items 0 and 2" in message
    assert lib.asp_sa_greedy_tree_batch(None, ctypes.c_uint32(2), None) == INVALID
    c_plans = (ctypes.c_void_p * 1)(fake_a)
    assert lib.asp_sa_greedy_tree_batch(c_plans, ctypes.c_uint32(1), None) == INVALID
    assert np.all(x == SENTINEL) and np.all(y == SENTINEL)
    assert lib.asp_sa_greedy_tree_last_ms() == 0.0
    assert _lib.gpu_touched() == touched


def test_an_empty_batch_needs_no_device():
    from annealing_sign_problem_amd import _lib, greedy

    lib = _lib.load()
    touched = _lib.gpu_touched()
    assert lib.asp_sa_greedy_tree_batch(None, ctypes.c_uint32(0), None) == 0
    assert lib.asp_last_error_code() == 0
    assert greedy.greedy_tree_batch([], where="device") == [] and greedy.greedy_tree_batch([], where="host") == []
    assert _lib.gpu_touched() == touched


def test_python_surface(monkeypatch):
    from annealing_sign_problem_amd import annealer as sa, common, greedy, sampled_components

    for function in (greedy.greedy_solve, greedy.greedy_solve_batch, sa.greedy_solve, sa.greedy_solve_batch,
                     common.solve_ising_model, common.solve_ising_models):
        parameters = inspect.signature(function).parameters
        assert list(parameters)[-1] == "tree" and parameters["tree"].default is None, function
    assert inspect.signature(greedy.greedy_tree).parameters["where"].default == "device"
    assert inspect.signature(greedy.greedy_tree_batch).parameters["where"].default == "device"
    monkeypatch.delenv("ASP_GREEDY_TREE", raising=False)
    assert greedy.tree_where(None) == 0 and greedy.tree_where("host") == 0 and greedy.tree_where("device") == 1
    monkeypatch.setenv("ASP_GREEDY_TREE", "device")
    assert greedy.tree_where(None) == 1 and greedy.tree_where("host") == 0
    with pytest.raises(ValueError):
        greedy.tree_where("gpu")
    with pytest.raises(ValueError):
        greedy.greedy_solve_batch([], tree=["host"])
    monkeypatch.delenv("ASP_GREEDY_TREE")
    args = sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "1",
                                                  "--greedy-tree", "device"])
    assert args.greedy_tree == "device"
    args = sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "1"])
    assert args.greedy_tree is None
    with pytest.raises(SystemExit):
        sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "1",
                                               "--greedy-tree", "lds"])


def test_the_host_tree_of_the_python_surface_is_the_host_entry_point():
    import greedy_tree_cases as cases
    from annealing_sign_problem_amd import annealer as sa, greedy

    J, h = cases.case("components_field_order")
    assert np.array_equal(greedy.greedy_tree(sa.Hamiltonian(J, h), where="host"), cases.tree(J, h))
