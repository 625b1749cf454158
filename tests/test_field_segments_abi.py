"""The C ABI of the segmented boundary field (asp_operator_field_segments, include/asp.h) without
a device: the symbol, the header against the bindings, every validation branch — all of which run before any device
work and before any output is written, with the segment in the message —, the call that needs no device, and the
Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SENTINEL = 12345.5
FAKE = ctypes.c_void_p(0x1000)  # an operator that does not exist: never dereferenced, a check fails first


def _u64(values):
    return np.array(values, dtype=np.uint64)


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def _call(op, offsets, keys, psi, env_offsets, env_keys, env_psi, field, unresolved, segments=None, scale=2.0):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    if segments is None:
        segments = 0 if offsets is None else offsets.size - 1
    return lib.asp_operator_field_segments(op, segments, _lib.ptr(offsets), _lib.ptr(keys), _lib.ptr(psi),
                                           _lib.ptr(env_offsets), _lib.ptr(env_keys), _lib.ptr(env_psi), scale,
                                           _lib.ptr(field), _lib.ptr(unresolved))


def test_library_exports_and_header_declares_the_symbol():
    from annealing_sign_problem_amd import _lib, build

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    assert "asp_operator_field_segments" in _lib.SIGNATURES and hasattr(lib, "asp_operator_field_segments")
    assert raw.asp_operator_field_segments is not None
    text = _header()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int asp_operator_field_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets, "
            "uint64_t const *keys, double const *psi, uint64_t const *env_offsets, uint64_t const *env_keys, "
            "double const *env_psi, double scale, double *field , uint64_t *unresolved );") in header
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_operator_field_segments"] == (
        ctypes.c_int, [p, u64, p, p, p, p, p, p, ctypes.c_double, p, p])
    assert "ASP-FIELD-SEG-1" in text
    assert "operator_field_segments.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "operator_field_segments.hip"))


def test_every_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    offsets = _u64([0, 3, 3, 5])
    keys = _u64([3, 5, 6, 5, 9])
    psi = np.array([0.6, -0.8, 0.0, 0.6, 0.8])
    env_offsets = _u64([0, 2, 4, 4])
    env_keys = _u64([9, 10, 3, 12])
    env_psi = np.array([0.1, -0.2, 0.3, 0.4])
    field = np.full(5, SENTINEL)
    unresolved = np.full(3, 77, dtype=np.uint64)
    ok = [FAKE, offsets, keys, psi, env_offsets, env_keys, env_psi, field, unresolved]

    def refused(message, changes, **keywords):
        args = list(ok)
        for at, value in changes.items():
            args[at] = value
        assert _call(*args, **keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert np.all(field == SENTINEL) and np.all(unresolved == 77)

    refused("null operator", {0: None})
    refused("null offsets with 3 segments", {1: None}, segments=3)
    refused("null environment offsets with 3 segments", {4: None}, segments=3)
    refused("offsets[0] is not 0", {1: _u64([1, 3, 3, 5])})
    refused("environment offsets[0] is not 0", {4: _u64([1, 2, 4, 4])})
    refused("offsets decrease at index 2", {1: _u64([0, 3, 2, 5])})
    refused("environment offsets decrease at index 3", {4: _u64([0, 2, 4, 3])})
    for at in (2, 3, 7):  # keys, psi, field
        refused("null keys, psi or field with 5 table entries", {at: None})
    for at in (5, 6):  # env_keys, env_psi
        refused("null environment arrays with 4 environment entries", {at: None})
    refused("the keys of segment 0 are not sorted and unique at index 2", {2: _u64([3, 6, 5, 5, 9])})
    refused("the keys of segment 2 are not sorted and unique at index 1", {2: _u64([3, 5, 6, 9, 5])})
    refused("the keys of segment 2 are not sorted and unique at index 1", {2: _u64([3, 5, 6, 9, 9])})
    refused("the environment keys of segment 0 are not sorted and unique at index 1", {5: _u64([10, 9, 3, 12])})
    refused("the environment keys of segment 1 are not sorted and unique at index 1", {5: _u64([9, 10, 12, 12])})
    # (a state that repeats in ANOTHER segment, or is a cluster key here and an environment key there, is legal:
    # entries 1 and 3 of keys hold state 5, keys and env_keys both hold 3 and 9 — tests/test_gpu_field_segments.py)
    assert _lib.gpu_touched() == touched


def test_tables_beyond_the_index_range_are_refused():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    code = int(re.search(r"ASP_ERR_TOO_LARGE\s*=\s*(-?\d+)", _header()).group(1))
    one, amplitude = _u64([3]), np.array([1.0])
    field = np.full(1, SENTINEL)
    unresolved = np.full(1, 77, dtype=np.uint64)
    # T or E = 2^32 - 1 (only the offsets say so: nothing of that length is read before the size check)
    for big_offsets, big_env in ((_u64([0, 2 ** 32 - 1]), _u64([0, 1])), (_u64([0, 1]), _u64([0, 2 ** 32 - 1]))):
        assert _call(FAKE, big_offsets, one, amplitude, big_env, one, amplitude, field, unresolved) == code
        assert "2^32" in _lib.last_error() and field[0] == SENTINEL and unresolved[0] == 77
    assert _lib.gpu_touched() == touched


def test_an_empty_table_needs_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    env_keys, env_psi = _u64([9, 10]), np.array([0.1, -0.2])
    unresolved = np.full(3, 77, dtype=np.uint64)
    assert _call(FAKE, _u64([0, 0, 0, 0]), None, None, _u64([0, 2, 2, 2]), env_keys, env_psi, None, unresolved) == 0
    assert lib.asp_last_error_code() == 0 and unresolved.tolist() == [0, 0, 0]
    assert _call(FAKE, _u64([0, 0]), None, None, _u64([0, 0]), None, None, None, None) == 0
    assert _call(FAKE, None, None, None, None, None, None, None, None) == 0  # no segments at all
    assert _call(None, None, None, None, None, None, None, None, None) == INVALID
    assert _lib.gpu_touched() == touched


class _Device:
    """DeviceOperator.field_segments up to the library call."""

    def __init__(self):
        from annealing_sign_problem_amd import _lib

        self._lib_module = _lib
        self._handle = None  # (the library refuses a null operator, should a shape check let a call through)
        self._lib = _lib.load()


def test_shape_errors_of_field_segments():
    from annealing_sign_problem_amd import _lib, operators

    touched = _lib.gpu_touched()
    parameters = inspect.signature(operators.DeviceOperator.field_segments).parameters
    assert list(parameters) == ["self", "keys", "psi", "offsets", "env_keys", "env_psi", "env_offsets", "scale"]
    assert parameters["scale"].default == 2.0
    call = operators.DeviceOperator.field_segments
    device = _Device()
    keys, psi = _u64([3, 5, 6]), np.array([0.6, -0.8, 0.0])
    env_keys, env_psi = _u64([9, 10]), np.array([0.1, -0.2])
    with pytest.raises(ValueError, match="psi and keys differ"):
        call(device, keys, psi[:2], [0, 3], env_keys, env_psi, [0, 2])
    with pytest.raises(ValueError, match="offsets should run from 0 to the number of keys"):
        call(device, keys, psi, [0, 2], env_keys, env_psi, [0, 2])
    with pytest.raises(ValueError, match="offsets should run from 0 to the number of keys"):
        call(device, keys, psi, [], env_keys, env_psi, [0, 2])
    with pytest.raises(ValueError, match="env_psi and env_keys differ"):
        call(device, keys, psi, [0, 3], env_keys, env_psi[:1], [0, 2])
    with pytest.raises(ValueError, match="env_offsets should run"):
        call(device, keys, psi, [0, 3], env_keys, env_psi, [0, 1])
    with pytest.raises(ValueError, match="env_offsets should run"):
        call(device, keys, psi, [0, 1, 3], env_keys, env_psi, [0, 2])  # one entry per entry of offsets
    # the shapes pass: the call reaches the library (which refuses the null handle of this stand-in)
    with pytest.raises(_lib.AspError, match="null operator"):
        call(device, keys, psi, [0, 1, 3], env_keys, env_psi, [0, 2, 2])
    with pytest.raises(_lib.AspError, match="null operator"):
        call(device, keys, psi, [0, 1, 3], None, None, None)  # every environment empty
    assert _lib.gpu_touched() == touched


def test_signatures_of_the_callers_are_unchanged():
    from annealing_sign_problem_amd import common

    parameters = inspect.signature(common.make_ising_models).parameters
    assert list(parameters) == ["clusters", "quantum_hamiltonian", "log_psis", "log_psi_fn", "external_field"]
    assert parameters["log_psis"].default is None and parameters["log_psi_fn"].default is None
    assert parameters["external_field"].default is False
    parameters = inspect.signature(common.reweight_ising_models).parameters
    assert list(parameters) == ["model", "log_psis", "log_psi_fns", "external_field", "outs"]
    assert parameters["external_field"].default is False and parameters["outs"].default is None
    assert list(inspect.signature(common._boundary_field).parameters) == [
        "hamiltonian", "spins", "psi", "log_psi_fn", "cluster_norm"]
    assert list(inspect.signature(common._boundary_fields).parameters) == ["hamiltonian", "clusters", "log_psi_fns"]
    assert common._boundary_fields(None, [], None) == []
