"""asp_sa_plan_create_segments, asp_sa_plan_segments_last_ms, asp_sa_plan_read_array (include/asp.h;
DESIGN.md §4.15): what can be checked without a device — the symbols, the header against the bindings,
every argument error (returned before any device work, with out_plans all NULL), the num_segments == 0
no-op and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -3, -4
SYMBOLS = ("asp_sa_plan_create_segments", "asp_sa_plan_segments_last_ms", "asp_sa_plan_read_array")


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_plan_create_segments\s*\(\s*uint64_t\s+num_segments\s*,\s*uint64_t\s+const\s*\*\s*offsets\s*,"
                     r"\s*int64_t\s+const\s*\*\s*indptr\s*,\s*int32_t\s+const\s*\*\s*indices\s*,\s*double\s+const\s*\*\s*data\s*,"
                     r"\s*double\s+const\s*\*\s*field\s*,\s*asp_sa_plan\s*\*\*\s*out_plans\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_plan_segments_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_plan_read_array\s*\(\s*asp_sa_plan\s+const\s*\*\s*p\s*,\s*int\s+which\s*,\s*void\s*\*\s*dst\s*,"
                     r"\s*uint64_t\s+capacity_bytes\s*,\s*uint64_t\s*\*\s*bytes\s*\)\s*;", header)
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_sa_plan_create_segments"] == (ctypes.c_int, [u64, p, p, p, p, p, p])
    assert _lib.SIGNATURES["asp_sa_plan_segments_last_ms"] == (ctypes.c_float, [])
    assert _lib.SIGNATURES["asp_sa_plan_read_array"] == (ctypes.c_int, [p, ctypes.c_int, p, u64, ctypes.POINTER(u64)])
    # the ids of the header are the ids of the bindings
    for name, (which, _) in sa.PLAN_ARRAYS.items():
        assert re.search(r"ASP_SA_ARRAY_%s\s*=\s*%d\b" % (name.upper(), which), header), name
    assert sorted(sa.PLAN_ARRAYS) == sorted(pc.ARRAYS)


def _call(lib, count, offsets, indptr, indices, data, field, plans):
    from annealing_sign_problem_amd import _lib

    return lib.asp_sa_plan_create_segments(ctypes.c_uint64(count), _lib.ptr(offsets), _lib.ptr(indptr), _lib.ptr(indices),
                                           _lib.ptr(data), _lib.ptr(field), plans)


def test_argument_errors_come_before_any_device_work():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = lib.asp_device_touched()
    offsets, indptr, indices, data, field = pc.concatenate(pc.rounds()["round_of_3"])
    u64 = lambda *values: np.array(values, dtype=np.uint64)  # noqa: E731

    def refused(code, text, *arguments):
        plans = (ctypes.c_void_p * 3)(1, 1, 1)
        assert _call(lib, 3, *arguments, plans) == code, text
        assert text in lib.asp_last_error().decode(), lib.asp_last_error()
        assert [p for p in plans] == [None, None, None]  # all NULL

    assert _call(lib, 3, offsets, indptr, indices, data, field, None) == INVALID
    assert b"null out_plans" in lib.asp_last_error()
    refused(INVALID, "null offsets", None, indptr, indices, data, field)
    refused(INVALID, "null indptr/field", offsets, None, indices, data, field)
    refused(INVALID, "null indptr/field", offsets, indptr, indices, data, None)
    refused(INVALID, "null indices/data", offsets, indptr, None, data, field)
    refused(INVALID, "null indices/data", offsets, indptr, indices, None, field)
    shifted = offsets.copy()
    shifted[0] = 1
    refused(INVALID, "offsets[0] must be 0", shifted, indptr, indices, data, field)
    decreasing = offsets.copy()
    decreasing[2] = decreasing[1] - 1
    refused(INVALID, "offsets decrease", decreasing, indptr, indices, data, field)
    first = indptr.copy()
    first[0] = 1
    refused(INVALID, "indptr[0] must be 0", offsets, first, indices, data, field)
    bent = indptr.copy()
    bent[5] = bent[6] + 1
    refused(INVALID, "indptr is not monotone", offsets, bent, indices, data, field)
    # T >= 2^32 - 1 and nnz >= 2^32 - 1: known from offsets / indptr alone, nothing else is read
    refused(TOO_LARGE, "2^32 - 2", u64(0, 1, 2, 2 ** 32 - 1), None, None, None, None)
    refused(TOO_LARGE, "stored couplings", u64(0, 1, 1, 1), np.array([0, 2 ** 32 - 1], dtype=np.int64), None, None, np.zeros(1))
    assert lib.asp_device_touched() == touched  # refused before any device work


def test_no_segments_is_a_no_op_without_a_device():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    touched = lib.asp_device_touched()
    assert _call(lib, 0, None, None, None, None, None, None) == 0
    assert lib.asp_sa_plan_segments_last_ms() == 0.0
    sa.plan_hamiltonians([])
    size = ctypes.c_uint64(7)
    assert lib.asp_sa_plan_read_array(None, 0, None, ctypes.c_uint64(0), ctypes.byref(size)) == INVALID
    assert size.value == 0 and b"null plan" in lib.asp_last_error()
    assert lib.asp_device_touched() == touched


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, sampled_components

    assert list(inspect.signature(sa.plan_hamiltonians).parameters) == ["hamiltonians"]
    assert list(inspect.signature(sa.plan_hamiltonians_last_ms).parameters) == []
    parameters = inspect.signature(common.solve_ising_models).parameters
    assert parameters["plan_batch"].default is False
    for function in (sampled_components.stage_clusters, sampled_components.process_clusters_batched):
        assert inspect.signature(function).parameters["plan_batch"].default is False
    base = ["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "1", "--no-annealing", "--batch", "16"]
    assert sampled_components.parse_command_line(base + ["--greedy-batch"]).plan_batch is False
    args = sampled_components.parse_command_line(base + ["--greedy-batch", "--plan-batch"])
    assert args.plan_batch is True and sampled_components.plan_batch_of(args) == {"plan_batch": True}
    assert sampled_components.plan_batch_of(sampled_components.parse_command_line(base + ["--greedy-batch"])) == {}
    with pytest.raises(SystemExit):
        sampled_components.parse_command_line(base + ["--plan-batch"])  # needs --greedy-batch
