"""The C ABI of the boundary field (asp_operator_field, include/asp.h) without a device: the
symbol, the header against the bindings, the validation that runs before any device work and before any output is
written, and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SENTINEL = 12345.5


def _call(lib, op, keys, psi, env_keys, env_psi, field, scale=2.0, unresolved=None, k=None, e=None):
    from annealing_sign_problem_amd import _lib

    k = (0 if keys is None else keys.size) if k is None else k
    e = (0 if env_keys is None else env_keys.size) if e is None else e
    return lib.asp_operator_field(op, k, _lib.ptr(keys), _lib.ptr(psi), e, _lib.ptr(env_keys), _lib.ptr(env_psi),
                                  scale, _lib.ptr(field), unresolved)


def test_library_exports_and_header_declares_the_symbol():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    assert "asp_operator_field" in _lib.SIGNATURES and hasattr(lib, "asp_operator_field")
    assert raw.asp_operator_field is not None
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        text = f.read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int asp_operator_field(asp_operator const *op, uint64_t num_spins, uint64_t const *keys, "
            "double const *psi, uint64_t num_env, uint64_t const *env_keys, double const *env_psi, double scale, "
            "double *field, uint64_t *unresolved );") in header
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_operator_field"] == (
        ctypes.c_int, [p, u64, p, p, u64, p, p, ctypes.c_double, p, ctypes.POINTER(u64)])
    assert "ASP-FIELD-1" in text


def test_validation_runs_before_any_device_work_and_before_any_output():
    """The checks look at the pointers and the keys only, so an operator that does not exist will do."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: a check fails first)
    keys = np.array([3, 5, 6], dtype=np.uint64)
    psi = np.array([0.6, -0.8, 0.0])
    env_keys = np.array([9, 10], dtype=np.uint64)
    env_psi = np.array([0.1, -0.2])
    field = np.full(3, SENTINEL)
    count = ctypes.c_uint64(77)
    ok = (keys, psi, env_keys, env_psi, field)
    assert _call(lib, None, *ok, unresolved=ctypes.byref(count)) == INVALID and "null operator" in _lib.last_error()
    for at in range(3):  # keys, psi, field
        args = list(ok)
        args[4 if at == 2 else at] = None
        assert _call(lib, fake, *args, k=3, unresolved=ctypes.byref(count)) == INVALID
        assert "null keys, psi or field" in _lib.last_error()
    for at in (2, 3):  # env_keys, env_psi
        args = list(ok)
        args[at] = None
        assert _call(lib, fake, *args, e=2, unresolved=ctypes.byref(count)) == INVALID
        assert "null environment" in _lib.last_error()
    assert _call(lib, fake, keys[::-1].copy(), psi, env_keys, env_psi, field) == INVALID
    assert "keys are not sorted" in _lib.last_error()
    assert _call(lib, fake, keys, psi, np.array([9, 9], dtype=np.uint64), env_psi, field) == INVALID
    assert "environment keys are not sorted" in _lib.last_error()
    assert np.all(field == SENTINEL) and count.value == 77
    assert _lib.gpu_touched() == touched


def test_an_empty_cluster_needs_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    fake = ctypes.c_void_p(0x1000)
    count = ctypes.c_uint64(77)
    env_keys = np.array([9, 10], dtype=np.uint64)
    assert _call(lib, fake, None, None, env_keys, np.array([0.1, -0.2]), None, unresolved=ctypes.byref(count)) == 0
    assert count.value == 0 and lib.asp_last_error_code() == 0
    assert _call(lib, fake, None, None, None, None, None) == 0
    assert _call(lib, None, None, None, None, None, None) == INVALID
    assert _lib.gpu_touched() == touched


class _Foreign:
    """An operator object that is not this package's: only its own batched_apply."""

    class basis:
        number_spins = 4

    def batched_apply(self, spins):
        raise AssertionError("not reached")


def test_python_surface():
    from annealing_sign_problem_amd import _lib, common, operators, sampled_components

    touched = _lib.gpu_touched()
    parameters = inspect.signature(operators.DeviceOperator.field).parameters
    assert list(parameters) == ["self", "keys", "psi", "env_keys", "env_psi", "scale"]
    assert parameters["scale"].default == 2.0
    assert inspect.signature(common.make_ising_model).parameters["external_field"].default is False
    extension = inspect.signature(common.make_hamiltonian_extension).parameters
    assert list(extension) == ["model", "log_psi_fn", "external_field"] and extension["external_field"].default is False
    for function in (sampled_components.process_cluster, sampled_components.stage_clusters,
                     sampled_components.process_clusters_batched):
        assert inspect.signature(function).parameters["external_field"].default is False, function
    spins = np.array([3, 5, 6], dtype=np.uint64)
    with pytest.raises(NotImplementedError, match="foreign"):
        common.make_ising_model(spins, _Foreign(), log_psi_fn=lambda s: np.zeros(len(s)), external_field=True)
    with pytest.raises(ValueError):
        common.make_ising_model(spins, _Foreign(), log_psi=np.zeros(3), external_field=True)
    assert _lib.gpu_touched() == touched
    base = ["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "1"]
    assert sampled_components.parse_command_line(base).external_field is False
    assert sampled_components.parse_command_line(base + ["--external-field"]).external_field is True
    assert sampled_components.external_field_of(sampled_components.parse_command_line(base)) == {}


def test_the_header_gains_a_line_only_with_the_flag(tmp_path):
    from annealing_sign_problem_amd import sampled_components

    lines = {}
    for flag in ([], ["--external-field"]):
        out = tmp_path / ("with.csv" if flag else "without.csv")
        args = sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--output", str(out),
                                                      "--order", "1"] + flag)
        sampled_components._write_header(args)
        lines[bool(flag)] = out.read_text().splitlines()
    assert [x for x in lines[True] if x not in lines[False]] == ["# external_field = True"]
    assert [x for x in lines[True] if x != "# external_field = True"] == lines[False]
    assert lines[False][-1] == lines[True][-1] == "# " + sampled_components.OptimizationResult.csv_header()
