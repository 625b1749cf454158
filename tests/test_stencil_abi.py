"""The coupling stencil (include/asp.h: asp_ising_stencil_*, asp_sa_plan_reweight_stencil_batch; DESIGN.md
§4.14.1): what can be checked without a device — the symbols, the header against the bindings, the struct
layouts, the refusals and no-ops that run before any device work, and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3

# name -> (return type, the header's parameter list)
DECLARATIONS = {
    "asp_ising_stencil_create": ("int", "asp_operator const *op, uint64_t num_spins, uint64_t const *keys, "
                                        "int64_t const *indptr, int32_t const *indices, asp_ising_stencil **out"),
    "asp_ising_stencil_destroy": ("void", "asp_ising_stencil *st"),
    "asp_ising_stencil_info": ("int", "asp_ising_stencil const *st, asp_ising_stencil_counts *out"),
    "asp_ising_stencil_values": ("int", "asp_ising_stencil *st, uint32_t count, double const *psi, double *data, "
                                        "int32_t *status"),
    "asp_sa_plan_reweight_stencil_batch": ("int", "asp_ising_stencil *st, asp_sa_stencil_item *items, uint32_t count"),
    "asp_sa_plan_reweight_stencil_last_ms": ("float", "void"),
}


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def _pattern(text):
    return r"\s*".join(re.escape(token) for token in re.findall(r"\w+|[^\w\s]", text))


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name, (returns, parameters) in DECLARATIONS.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + returns + r"\s+" + name + r"\s*\(\s*" + _pattern(parameters) + r"\s*\)\s*;", header), name
    p, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    assert _lib.SIGNATURES["asp_ising_stencil_create"] == (ctypes.c_int, [p, u64, p, p, p, ctypes.POINTER(p)])
    assert _lib.SIGNATURES["asp_ising_stencil_destroy"] == (None, [p])
    assert _lib.SIGNATURES["asp_ising_stencil_info"] == (ctypes.c_int, [p, ctypes.POINTER(_lib.IsingStencilCounts)])
    assert _lib.SIGNATURES["asp_ising_stencil_values"] == (ctypes.c_int, [p, u32, p, p, p])
    assert _lib.SIGNATURES["asp_sa_plan_reweight_stencil_batch"] == (
        ctypes.c_int, [p, ctypes.POINTER(_lib.SaStencilItem), u32])
    assert _lib.SIGNATURES["asp_sa_plan_reweight_stencil_last_ms"] == (ctypes.c_float, [])
    assert "ASP-STENCIL-1" in header and "__dmul_rn" in header  # the law stands in the comment


C_TYPES = {"uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "asp_sa_plan *": ctypes.c_void_p,
           "double const *": ctypes.c_void_p, "double *": ctypes.c_void_p}


@pytest.mark.parametrize("struct, mirror", [("asp_ising_stencil_counts", "IsingStencilCounts"),
                                            ("asp_sa_stencil_item", "SaStencilItem")])
def test_struct_layouts_match_the_header(struct, mirror):
    from annealing_sign_problem_amd import _lib

    body = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for declaration in filter(None, (d.strip() for d in body.split(";"))):
        kind, name = re.match(r"(.*?)(\w+)$", declaration).groups()
        kind = " ".join(kind.split())
        members.append((name, C_TYPES[kind]))
    assert [(name, kind) for name, kind in getattr(_lib, mirror)._fields_] == members
    # natural alignment, as the compiler lays the C struct out
    offset = 0
    for name, kind in members:
        size = ctypes.sizeof(kind)
        offset = (offset + size - 1) // size * size
        assert getattr(getattr(_lib, mirror), name).offset == offset, name
        offset += size
    assert ctypes.sizeof(getattr(_lib, mirror)) == (offset + 7) // 8 * 8


def test_refusals_and_no_ops_need_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = lib.asp_device_touched()
    psi, data, status = np.ones(2), np.zeros(2), np.zeros(1, dtype=np.int32)
    keys = np.array([1, 2], dtype=np.uint64)
    indptr, indices = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    out = ctypes.c_void_p()
    # creation: null arguments
    assert lib.asp_ising_stencil_create(None, 2, _lib.ptr(keys), _lib.ptr(indptr), _lib.ptr(indices),
                                        ctypes.byref(out)) == INVALID
    assert b"null operator" in lib.asp_last_error() and not out.value
    assert lib.asp_ising_stencil_create(None, 2, _lib.ptr(keys), _lib.ptr(indptr), _lib.ptr(indices), None) == INVALID
    # a null stencil
    assert lib.asp_ising_stencil_values(None, 1, _lib.ptr(psi), _lib.ptr(data), _lib.ptr(status)) == INVALID
    assert b"null stencil" in lib.asp_last_error()
    assert lib.asp_ising_stencil_info(None, ctypes.byref(_lib.IsingStencilCounts())) == INVALID
    items = (_lib.SaStencilItem * 1)()
    assert lib.asp_sa_plan_reweight_stencil_batch(None, items, 1) == INVALID
    assert b"null stencil" in lib.asp_last_error()
    lib.asp_ising_stencil_destroy(None)
    assert lib.asp_sa_plan_reweight_stencil_last_ms() == 0.0
    # a stencil of no states needs no device either; with it: null items, a null plan, count == 0
    empty = np.zeros(1, dtype=np.int64)
    operator = ctypes.c_void_p(1)  # (never dereferenced for K == 0)
    assert lib.asp_ising_stencil_create(operator, 0, None, _lib.ptr(empty), None, ctypes.byref(out)) == 0
    try:
        counts = _lib.IsingStencilCounts()
        assert lib.asp_ising_stencil_info(out, ctypes.byref(counts)) == 0
        assert (counts.num_spins, counts.stored, counts.connections, counts.silent_pairs) == (0, 0, 0, 0)
        assert lib.asp_sa_plan_reweight_stencil_batch(out, None, 1) == INVALID
        assert b"null items" in lib.asp_last_error()
        items[0].plan = None
        assert lib.asp_sa_plan_reweight_stencil_batch(out, items, 1) == INVALID
        assert b"item 0: null plan" in lib.asp_last_error()
        assert lib.asp_sa_plan_reweight_stencil_batch(out, None, 0) == 0
        assert lib.asp_sa_plan_reweight_stencil_batch(out, items, 0) == 0
        assert lib.asp_ising_stencil_values(out, 0, None, None, None) == 0
        status[0] = 7
        assert lib.asp_ising_stencil_values(out, 1, None, None, _lib.ptr(status)) == 0 and status[0] == 0
    finally:
        lib.asp_ising_stencil_destroy(out)
    # unsorted keys and a non-canonical pattern are refused before the operator is looked at
    for bad_keys, bad_indptr, bad_indices, message in (
            (keys[::-1].copy(), indptr, indices, b"not sorted"),
            (keys, np.array([0, 2, 1], dtype=np.int64), indices, b"not canonical"),
            (keys, np.array([1, 1, 2], dtype=np.int64), indices, b"not canonical"),
            (keys, np.array([0, 2, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), b"not canonical"),
            (keys, indptr, np.array([0, 2], dtype=np.int32), b"not canonical")):
        assert lib.asp_ising_stencil_create(operator, 2, _lib.ptr(bad_keys), _lib.ptr(bad_indptr), _lib.ptr(bad_indices),
                                            ctypes.byref(out)) == INVALID
        assert message in lib.asp_last_error() and not out.value
    assert lib.asp_device_touched() == touched


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, influence_of_noise, operators

    assert "reweight_hamiltonians" in sa.__all__ and "reweight_ising_models" in common.__all__
    assert list(inspect.signature(sa.reweight_hamiltonians).parameters) == ["hamiltonians", "stencil", "psis", "fields"]
    assert inspect.signature(sa.reweight_hamiltonians).parameters["fields"].default is None
    parameters = inspect.signature(common.reweight_ising_models).parameters
    assert list(parameters) == ["model", "log_psis", "log_psi_fns", "external_field", "outs"]
    assert [parameters[n].default for n in list(parameters)[1:]] == [None, None, False, None]
    assert list(inspect.signature(operators.DeviceOperator.ising_stencil).parameters) == ["self", "keys", "indptr", "indices"]
    for name in ("info", "values", "close", "__enter__", "__exit__"):
        assert hasattr(operators.IsingStencil, name), name
    assert list(inspect.signature(operators.IsingStencil.values).parameters) == ["self", "psis"]
    parameters = inspect.signature(influence_of_noise.influence_of_noise).parameters
    assert list(parameters) == ["hamiltonian", "ground_state", "noise_levels", "repetitions", "batch", "reuse", "seed",
                                "from_amplitudes"]
    assert parameters["from_amplitudes"].default is False and parameters["reuse"].default is True


def test_the_from_amplitudes_flag_parses(tmp_path, capsys):
    from annealing_sign_problem_amd import influence_of_noise

    # with an output file that exists the run ends after parsing, before anything is loaded
    output = tmp_path / "rows.csv"
    output.write_text("")
    for flags in (["--from-amplitudes"], []):
        assert influence_of_noise.main(["--model", "nothing", "--seed", "1", "--output", str(output)] + flags) == 1
        assert "exists already" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        influence_of_noise.main(["--model", "nothing", "--seed", "1", "--output", str(output), "--from-amplitude=3"])
    capsys.readouterr()


def test_reweight_ising_models_validates_before_a_device_is_touched():
    from annealing_sign_problem_amd import _lib, common

    touched = _lib.load().asp_device_touched()
    model = common.IsingModel(np.array([1, 2], dtype=np.uint64), object(), None, np.zeros(1, dtype=np.uint64))
    with pytest.raises(ValueError, match="one element per draw"):
        common.reweight_ising_models(model, log_psis=[np.zeros(2)], log_psi_fns=[None, None])
    with pytest.raises(ValueError, match="one element per draw"):
        common.reweight_ising_models(model, log_psis=[np.zeros(2)], outs=[None, None])
    with pytest.raises(ValueError, match="at least one of log_psi or log_psi_fn"):
        common.reweight_ising_models(model, log_psis=[np.zeros(2), None], log_psi_fns=[None, None])
    with pytest.raises(ValueError, match="log_psi_fn should be specified when external_field=True"):
        common.reweight_ising_models(model, log_psis=[np.zeros(2)], external_field=True)
    with pytest.raises(ValueError, match="twice"):
        common.reweight_ising_models(model, log_psis=[np.zeros(2)] * 2, outs=[model, model])
    assert common.reweight_ising_models(model) == []
    assert _lib.load().asp_device_touched() == touched
