"""The C ABI of the segmented cluster growth (asp_operator_grow_segments; include/asp.h) without a
device: the symbol, the header against the binding, every validation branch that needs no operator — all of which run
before any device work and before any output is written —, the call that needs no device, and the Python surface.
(A seed with a bit at or above the operator's sites needs the operator: tests/test_gpu_grow.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
FAKE = ctypes.c_void_p(0x1000)  # an operator that does not exist: never dereferenced, a check fails first


def _u64(values):
    return np.array(values, dtype=np.uint64)


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_symbol():
    from annealing_sign_problem_amd import _lib, build

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    text = _header()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    name = "asp_operator_grow_segments"
    assert name in _lib.SIGNATURES and hasattr(lib, name) and getattr(raw, name) is not None
    assert ("int asp_operator_grow_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *seeds, "
            "uint64_t const *sizes, uint32_t const *ids, double keep_probability, uint64_t rng_seed, uint64_t capacity, "
            "uint64_t *out, uint64_t *out_offsets, uint64_t *count, uint32_t *passes );") in header
    assert _lib.SIGNATURES[name] == (ctypes.c_int, [p, u64, p, p, p, ctypes.c_double, u64, u64, p, p,
                                                    ctypes.POINTER(u64), p])
    assert "ASP-GROW-1" in text
    assert "cluster_grow.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "cluster_grow.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "segment_kernels.hpp"))


class _Grow:
    """Three segments of sizes 4, 1 and 7."""

    def __init__(self, capacity=12):
        self.seeds = _u64([0x5555, 0x0F0F, 0x3333])
        self.sizes = _u64([4, 1, 7])
        self.ids = np.array([0, 1, 2], dtype=np.uint32)
        self.capacity = capacity
        self.out = np.full(max(capacity, 1), 4242, dtype=np.uint64)
        self.out_offsets = np.full(4, 77, dtype=np.uint64)
        self.passes = np.full(3, 55, dtype=np.uint32)
        self.count = ctypes.c_uint64(991)

    def untouched(self):
        return bool(np.all(self.out == 4242) and np.all(self.out_offsets == 77) and np.all(self.passes == 55)
                    and self.count.value == 991)

    def call(self, op, p=0.5, segments=None, count=True, out_offsets=True, out=True, **replaced):
        from annealing_sign_problem_amd import _lib

        a = dict(seeds=self.seeds, sizes=self.sizes, ids=self.ids)
        a.update(replaced)
        segments = 3 if segments is None else segments
        return _lib.load().asp_operator_grow_segments(
            op, segments, _lib.ptr(a["seeds"]), _lib.ptr(a["sizes"]), _lib.ptr(a["ids"]), p, 12345, self.capacity,
            _lib.ptr(self.out) if out else None, _lib.ptr(self.out_offsets) if out_offsets else None,
            ctypes.byref(self.count) if count else None, _lib.ptr(self.passes))


def test_every_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    g = _Grow()

    def refused(message, op=FAKE, **keywords):
        assert g.call(op, **keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert g.untouched()

    refused("null operator", op=None)
    refused("null count pointer", count=False)
    refused("null count pointer", out_offsets=False)
    refused("null seeds, sizes or ids with 3 segments", seeds=None)
    refused("null seeds, sizes or ids with 3 segments", sizes=None)
    refused("null seeds, sizes or ids with 3 segments", ids=None)
    for p in (-0.25, 1.0000000000000002, float("nan"), float("inf"), -float("inf")):
        refused("is not in [0, 1]", p=p)
    refused("size of segment 1 is 0", sizes=_u64([4, 0, 7]))
    refused("size of segment 0 is 0", sizes=_u64([0, 0, 7]))
    refused("null output with 3 segments", out=False)
    short = _Grow(capacity=11)
    assert short.call(FAKE) == INVALID and "capacity 11 is below the sum of the sizes, 12" in _lib.last_error()
    assert short.untouched()
    assert _lib.gpu_touched() == touched


def test_sizes_beyond_the_index_range_are_refused():
    from annealing_sign_problem_amd import _lib

    code = int(re.search(r"ASP_ERR_TOO_LARGE\s*=\s*(-?\d+)", _header()).group(1))
    touched = _lib.gpu_touched()
    g = _Grow(capacity=1)
    g.capacity = 2 ** 40    # (never written: the sizes are refused first)
    for sizes in ([4, 2 ** 32 - 1, 7], [2 ** 31, 2 ** 31, 7]):
        assert g.call(FAKE, sizes=_u64(sizes)) == code
        assert "2^32" in _lib.last_error() and g.untouched()
    assert _lib.gpu_touched() == touched


def test_no_segments_need_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    for arrays in (dict(seeds=None, sizes=None, ids=None), {}):
        g = _Grow(capacity=0)
        assert g.call(FAKE, segments=0, out=False, **arrays) == 0 and lib.asp_last_error_code() == 0
        assert g.count.value == 0 and g.out_offsets.tolist() == [0, 77, 77, 77]
        assert np.all(g.out == 4242) and np.all(g.passes == 55)
    assert _lib.gpu_touched() == touched


# -- the Python surface ----------------------------------------------------------------------------------------
class _Foreign:
    """An operator object of another package: it has a batched_apply and no device action."""

    class basis:
        number_spins = 16
        states = _u64([0x5555, 0x0F0F])

    def batched_apply(self, spins):
        raise AssertionError("not reached")


def test_python_surface_and_command_line():
    from annealing_sign_problem_amd import operators, sampled_components as sc

    assert list(inspect.signature(operators.DeviceOperator.grow_segments).parameters) == [
        "self", "seeds", "sizes", "keep_probability", "seed", "ids"]
    assert inspect.signature(operators.DeviceOperator.grow_segments).parameters["ids"].default is None
    parameters = inspect.signature(sc.grow_clusters).parameters
    assert list(parameters) == ["hamiltonian", "seeds", "sizes", "keep_probability", "seed", "first_id",
                                "max_connections_per_call"]
    assert parameters["first_id"].default == 0 and parameters["max_connections_per_call"].default == 2 ** 32 - 1
    for function in (sc.iter_clusters, sc.generate_clusters):
        assert inspect.signature(function).parameters["grow"].default == "host"
    base = ["--model", "heisenberg_kagome_16", "--output", "x.csv", "--order", "0"]
    assert sc.parse_command_line(base).grow == "host"
    assert sc.parse_command_line(base + ["--grow", "device"]).grow == "device"
    assert sc.grow_of(sc.parse_command_line(base)) == {}
    assert sc.grow_of(sc.parse_command_line(base + ["--grow", "device", "--batch", "64"])) == {"grow": "device",
                                                                                              "batch": 64}
    with pytest.raises(SystemExit):
        sc.parse_command_line(base + ["--grow", "elsewhere"])


def test_a_foreign_operator_is_refused_and_not_grown_on_the_host():
    from annealing_sign_problem_amd import sampled_components as sc

    with pytest.raises(TypeError, match="no device action"):
        sc.grow_clusters(_Foreign(), _u64([0x5555]), _u64([5]), 0.5, 1)
    np.random.seed(3)
    with pytest.raises(TypeError, match="no device action"):
        list(sc.iter_clusters(_Foreign(), np.array([0.6, 0.8]), 2, 0.1, 3, 5, 0.5, grow="device"))
    with pytest.raises(ValueError):
        list(sc.iter_clusters(_Foreign(), np.array([0.6, 0.8]), 2, 0.1, 3, 5, 0.5, grow="elsewhere"))
