"""The C ABI of the segmented cutoff and extension (asp_sparsify_component_segments, asp_operator_extend_segments;
include/asp.h) without a device: the symbols, the header against the bindings, every
validation branch — all of which run before any device work and before any output is written —, the calls that need
no device, the Python surface and the --level-batch plumbing."""
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


def _too_large():
    return int(re.search(r"ASP_ERR_TOO_LARGE\s*=\s*(-?\d+)", _header()).group(1))


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib, build

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    text = _header()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    for name in ("asp_sparsify_component_segments", "asp_operator_extend_segments"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and getattr(raw, name) is not None
    assert ("int asp_sparsify_component_segments(uint64_t num_segments, uint64_t const *offsets, int64_t const *indptr, "
            "int32_t const *indices, double const *data, uint8_t const *is_frozen, double reltol, "
            "uint64_t const *anchors, uint8_t *keep, uint64_t *kept_offsets, uint64_t capacity, int64_t *out_indptr, "
            "int32_t *out_indices, double *out_data, uint64_t *out_nnz);") in header
    assert ("int asp_operator_extend_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets, "
            "uint64_t const *keys, uint64_t capacity, uint64_t *out, uint64_t *out_offsets, uint64_t *count);") in header
    assert _lib.SIGNATURES["asp_sparsify_component_segments"] == (
        ctypes.c_int, [u64, p, p, p, p, p, ctypes.c_double, p, p, p, u64, p, p, p, ctypes.POINTER(u64)])
    assert _lib.SIGNATURES["asp_operator_extend_segments"] == (ctypes.c_int, [p, u64, p, p, u64, p, p, ctypes.POINTER(u64)])
    assert "ASP-SPARSIFY-SEG-1" in text and "ASP-EXTEND-SEG-1" in text
    assert "level_segments.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "level_segments.hip"))


# -- asp_sparsify_component_segments ---------------------------------------------------------------------------
class _Sparsify:
    """Two segments of 2 and 3 spins: [[., 1], [1, .]] and a path 0 - 1 - 2."""

    def __init__(self, capacity=8):
        self.offsets = _u64([0, 2, 5])
        self.indptr = np.array([0, 1, 2, 3, 5, 6], dtype=np.int64)
        self.indices = np.array([1, 0, 1, 0, 2, 1], dtype=np.int32)
        self.data = np.array([1.0, 1.0, 0.5, 0.5, 2.0, 2.0])
        self.frozen = np.array([1, 0, 0, 1, 0], dtype=np.uint8)
        self.anchors = _u64([0, 1])
        self.capacity = capacity
        self.keep = np.full(5, 9, dtype=np.uint8)
        self.kept_offsets = np.full(3, 77, dtype=np.uint64)
        self.out_indptr = np.full(6, -77, dtype=np.int64)
        self.out_indices = np.full(capacity, -5, dtype=np.int32)
        self.out_data = np.full(capacity, 12345.5)
        self.nnz = ctypes.c_uint64(991)

    def untouched(self):
        return bool(np.all(self.keep == 9) and np.all(self.kept_offsets == 77) and np.all(self.out_indptr == -77)
                    and np.all(self.out_indices == -5) and np.all(self.out_data == 12345.5) and self.nnz.value == 991)

    def call(self, segments=None, nnz=True, kept=True, **replaced):
        from annealing_sign_problem_amd import _lib

        a = dict(offsets=self.offsets, indptr=self.indptr, indices=self.indices, data=self.data, frozen=self.frozen,
                 anchors=self.anchors, keep=self.keep)
        a.update(replaced)
        segments = (0 if a["offsets"] is None else a["offsets"].size - 1) if segments is None else segments
        return _lib.load().asp_sparsify_component_segments(
            segments, _lib.ptr(a["offsets"]), _lib.ptr(a["indptr"]), _lib.ptr(a["indices"]), _lib.ptr(a["data"]),
            _lib.ptr(a["frozen"]), 1e-3, _lib.ptr(a["anchors"]), _lib.ptr(a["keep"]),
            _lib.ptr(self.kept_offsets) if kept else None, self.capacity, _lib.ptr(self.out_indptr),
            _lib.ptr(self.out_indices), _lib.ptr(self.out_data), ctypes.byref(self.nnz) if nnz else None)


def test_every_sparsify_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    s = _Sparsify()

    def refused(message, **keywords):
        assert s.call(**keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert s.untouched()

    refused("null count pointer", nnz=False)
    refused("null count pointer", kept=False)
    refused("null offsets with 2 segments", offsets=None, segments=2)
    refused("null anchors with 2 segments", anchors=None)
    refused("offsets[0] is not 0", offsets=_u64([1, 2, 5]))
    refused("offsets decrease at index 2", offsets=_u64([0, 6, 5]))
    refused("null input array", indptr=None)
    refused("null input array", frozen=None)
    refused("null input array", keep=None)
    refused("indptr[0] must be 0", indptr=np.array([1, 1, 2, 3, 5, 6], dtype=np.int64))
    refused("indptr is not monotone", indptr=np.array([0, 1, 2, 5, 3, 6], dtype=np.int64))
    refused("null indices/data", indices=None)
    refused("null indices/data", data=None)
    # a column that is in range for the TABLE but not for its segment; a negative one
    refused("column index out of range in row 1 of segment 0", indices=np.array([1, 2, 1, 0, 2, 1], dtype=np.int32))
    refused("column index out of range in row 2 of segment 1", indices=np.array([1, 0, 1, 0, 2, 3], dtype=np.int32))
    refused("column index out of range in row 0 of segment 0", indices=np.array([-1, 0, 1, 0, 2, 1], dtype=np.int32))
    refused("row 1 of segment 1 is not sorted and duplicate-free", indices=np.array([1, 0, 1, 2, 0, 1], dtype=np.int32))
    refused("row 1 of segment 1 is not sorted and duplicate-free", indices=np.array([1, 0, 1, 2, 2, 1], dtype=np.int32))
    refused("anchor spin of segment 0 out of range", anchors=_u64([2, 1]))
    refused("anchor spin of segment 1 out of range", anchors=_u64([0, 3]))
    assert _lib.gpu_touched() == touched


def test_tables_beyond_the_index_range_are_refused():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    code = _too_large()
    s = _Sparsify()
    # T = 2^32 - 1 (only the offsets say so: nothing of that length is read before the size check)
    assert s.call(offsets=_u64([0, 2 ** 32 - 1]), anchors=_u64([0])) == code
    assert "2^32" in _lib.last_error() and s.untouched()
    e = _Extend(1)
    assert e.call(FAKE, _u64([0, 2 ** 32 - 1]), _u64([3])) == code
    assert "2^32" in _lib.last_error() and e.untouched()
    assert _lib.gpu_touched() == touched


def test_an_empty_sparsify_table_needs_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    for offsets in (None, _u64([0]), _u64([0, 0, 0])):
        s = _Sparsify()
        segments = 0 if offsets is None else offsets.size - 1
        assert s.call(offsets=offsets, indptr=None, indices=None, data=None, frozen=None, keep=None,
                      anchors=_u64([5, 5]) if segments else None) == 0 and lib.asp_last_error_code() == 0
        assert s.nnz.value == 0 and s.out_indptr[0] == 0 and np.all(s.out_indptr[1:] == -77)
        assert s.kept_offsets.tolist() == [0] * (segments + 1) + [77] * (2 - segments)   # (the anchors were not read)
        assert np.all(s.keep == 9) and np.all(s.out_indices == -5) and np.all(s.out_data == 12345.5)
    # a mask-only call of nothing
    nnz, kept = ctypes.c_uint64(7), _u64([7])
    assert lib.asp_sparsify_component_segments(0, None, None, None, None, None, 0.5, None, None, _lib.ptr(kept), 0, None,
                                               None, None, ctypes.byref(nnz)) == 0
    assert nnz.value == 0 and kept.tolist() == [0]
    assert _lib.gpu_touched() == touched


# -- asp_operator_extend_segments ------------------------------------------------------------------------------
class _Extend:
    def __init__(self, segments, capacity=8):
        self.capacity = capacity
        self.out = np.full(capacity, 4242, dtype=np.uint64)
        self.out_offsets = np.full(segments + 1, 77, dtype=np.uint64)
        self.count = ctypes.c_uint64(991)

    def untouched(self):
        return bool(np.all(self.out == 4242) and np.all(self.out_offsets == 77) and self.count.value == 991)

    def call(self, op, offsets, keys, segments=None, count=True, out_offsets=True):
        from annealing_sign_problem_amd import _lib

        segments = (0 if offsets is None else offsets.size - 1) if segments is None else segments
        return _lib.load().asp_operator_extend_segments(
            op, segments, _lib.ptr(offsets), _lib.ptr(keys), self.capacity, _lib.ptr(self.out),
            _lib.ptr(self.out_offsets) if out_offsets else None, ctypes.byref(self.count) if count else None)


def test_every_extend_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    offsets, keys = _u64([0, 3, 3, 5]), _u64([6, 3, 3, 5, 9])
    e = _Extend(3)

    def refused(message, *args, **keywords):
        assert e.call(*args, **keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert e.untouched()

    refused("null operator", None, offsets, keys)
    refused("null count pointer", FAKE, offsets, keys, count=False)
    refused("null count pointer", FAKE, offsets, keys, out_offsets=False)
    refused("null offsets with 3 segments", FAKE, None, keys, segments=3)
    refused("offsets[0] is not 0", FAKE, _u64([1, 3, 3, 5]), keys)
    refused("offsets decrease at index 2", FAKE, _u64([0, 3, 2, 5]), keys)
    refused("offsets decrease at index 3", FAKE, _u64([0, 3, 3, 2]), keys)
    refused("null keys with 5 table entries", FAKE, offsets, None)
    # (a key with a bit above the operator's sites needs the operator: tests/test_gpu_level_batch.py)
    assert _lib.gpu_touched() == touched


def test_an_empty_extend_table_needs_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    for offsets in (None, _u64([0]), _u64([0, 0, 0])):
        segments = 0 if offsets is None else offsets.size - 1
        e = _Extend(2)
        assert e.call(FAKE, offsets, None) == 0 and lib.asp_last_error_code() == 0
        assert e.count.value == 0 and e.out_offsets.tolist() == [0] * (segments + 1) + [77] * (2 - segments)
        assert np.all(e.out == 4242)
    assert _Extend(0).call(None, None, None) == INVALID
    assert _lib.gpu_touched() == touched


# -- the Python surface ----------------------------------------------------------------------------------------
class _Foreign:
    """An operator object that is not this package's: only its own batched_apply."""

    class basis:
        number_spins = 4

    def batched_apply(self, spins):
        raise AssertionError("not reached")


def test_python_surface(monkeypatch):
    from annealing_sign_problem_amd import _lib, common, operators, sampled_components

    touched = _lib.gpu_touched()
    assert list(inspect.signature(operators.DeviceOperator.extend_segments).parameters) == ["self", "keys", "offsets"]
    assert list(inspect.signature(common.extension_spins_segments).parameters) == ["hamiltonian", "spins_list"]
    assert list(inspect.signature(common.sparsify_component_segments).parameters) == [
        "offsets", "indptr", "indices", "data", "is_frozen", "reltol", "anchors"]
    assert list(inspect.signature(common.sparsify_models_using_global_cutoff).parameters) == [
        "models", "reltol", "frozen_spins_list"]
    parameters = inspect.signature(common.extend_and_sparsify_models).parameters
    assert list(parameters) == ["models", "log_psi_fn", "reltol", "frozen_spins_list", "external_field"]
    assert parameters["external_field"].default is False
    for name in ("extension_spins_segments", "sparsify_component_segments", "sparsify_models_using_global_cutoff",
                 "extend_and_sparsify_models"):
        assert name in common.__all__
    for function in (sampled_components.stage_clusters, sampled_components.process_clusters_batched):
        assert inspect.signature(function).parameters["level_batch"].default is False
    # a foreign operator object takes the loop of extension_spins
    seen = []

    def one(hamiltonian, spins):
        seen.append((hamiltonian, list(spins)))
        return "extension %d" % len(seen)

    monkeypatch.setattr(common, "extension_spins", one)
    foreign = _Foreign()
    assert common.extension_spins_segments(foreign, [[3, 5], [6]]) == ["extension 1", "extension 2"]
    assert seen == [(foreign, [3, 5]), (foreign, [6])]
    assert common.extension_spins_segments(foreign, []) == []
    assert common.sparsify_models_using_global_cutoff([], 1e-3, []) == []
    assert common.extend_and_sparsify_models([], None, 1e-3, []) == []
    with pytest.raises(ValueError, match="one array per model"):
        common.sparsify_models_using_global_cutoff([], 1e-3, [[1]])
    # the empty table goes through the library without a device
    keep, kept_offsets, ip, col, val = common.sparsify_component_segments([0, 0], [0], [], [], [], 1e-3, [0])
    assert keep.size == 0 and kept_offsets.tolist() == [0, 0] and ip.tolist() == [0] and col.size == 0 and val.size == 0
    assert _lib.gpu_touched() == touched


BASE = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1"]


def test_the_flag_travels_as_a_keyword_that_is_absent_without_it(monkeypatch):
    """--level-batch -> level_batch_of(args) -> process_clusters_batched -> stage_clusters(level_batch=True); without
    the flag no new keyword is passed anywhere."""
    from annealing_sign_problem_amd import sampled_components

    args = sampled_components.parse_command_line(BASE)
    assert args.level_batch is False and sampled_components.level_batch_of(args) == {}
    args = sampled_components.parse_command_line(BASE + ["--build-batch", "--level-batch"])
    assert args.level_batch is True and sampled_components.level_batch_of(args) == {"level_batch": True}
    assert sampled_components.level_batch_of(object()) == {}
    seen = []

    def stage(clusters, hamiltonian, ground_state, noisy_ground_state, noisy_log_coeff_fn, order, global_cutoff,
              jobs=1, **keywords):
        seen.append(keywords)
        return []

    monkeypatch.setattr(sampled_components, "stage_clusters", stage)
    for extra, want in (([], {}), (["--build-batch"], {"build_batch": True}),
                        (["--build-batch", "--level-batch"], {"build_batch": True, "level_batch": True}),
                        (["--build-batch", "--level-batch", "--greedy-batch", "--external-field"],
                         {"build_batch": True, "level_batch": True, "greedy_batch": True, "external_field": True})):
        args = sampled_components.parse_command_line(BASE + extra)
        out = sampled_components.process_clusters_batched(
            [[1], [2]], None, None, None, None, 1, 1e-4, False, jobs=1, sweep_order=args.sweep_order,
            **({"greedy_batch": True} if args.greedy_batch else {}), **sampled_components.early_stop_of(args),
            **sampled_components.external_field_of(args), **sampled_components.build_batch_of(args),
            **sampled_components.level_batch_of(args))
        assert out == [[], []] and seen.pop() == want and not seen


def test_the_flag_needs_build_batch(capsys):
    from annealing_sign_problem_amd import sampled_components

    with pytest.raises(SystemExit) as error:
        sampled_components.parse_command_line(BASE + ["--level-batch"])
    assert error.value.code == 2
    assert "--level-batch needs --build-batch" in " ".join(capsys.readouterr().err.split())
    sampled_components.parse_command_line(BASE + ["--level-batch", "--build-batch"])


@pytest.mark.parametrize("greedy_batch", [False, True])
def test_stage_clusters_stages_a_level_in_one_call(monkeypatch, greedy_batch):
    """With build_batch and level_batch the models of order i > 0 of ALL clusters come from ONE
    extend_and_sparsify_models call; none of the per-cluster builders runs; the staged list keeps its order."""
    from annealing_sign_problem_amd import common, sampled_components

    class Model:
        basis_index = None

        def __init__(self, name):
            self.name, self.spins, self.size = name, name, 3

    calls = []

    def many(clusters, hamiltonian, log_psis=None, log_psi_fn=None, **keywords):
        calls.append(("models", [list(c) for c in clusters], log_psi_fn, keywords))
        return [Model("m%d" % c[0]) for c in clusters]

    def level(models, log_psi_fn, reltol, frozen_spins_list, **keywords):
        calls.append(("level", [m.name for m in models], log_psi_fn, reltol, [list(f) for f in frozen_spins_list], keywords))
        return [Model(m.name + "+s") for m in models]

    def single(*a, **k):
        raise AssertionError("the per-cluster builders are not used")

    def solve(h, cluster, exact_signs, weights, annealing):
        assert not greedy_batch and annealing is False
        return sampled_components.OptimizationResult(h.size, h.name, exact_signs, 0.0, 0.0, 0.0)

    monkeypatch.setattr(common, "make_ising_models", many)
    monkeypatch.setattr(common, "extend_and_sparsify_models", level)
    for name in ("make_hamiltonian_extensions", "sparsify_using_global_cutoff", "make_ising_model",
                 "make_hamiltonian_extension", "extension_spins", "sparsify_component"):
        monkeypatch.setattr(common, name, single)
    monkeypatch.setattr(common, "solve_ising_models", lambda models, frozen, mode: [m.name for m in models])
    monkeypatch.setattr(common, "compute_accuracy_and_overlap", lambda x, signs, weights: (x, signs))
    monkeypatch.setattr(sampled_components, "exact_signs_and_weights",
                        lambda cluster, model, ground_state, basis: ("signs of " + model.name, None))
    monkeypatch.setattr(sampled_components, "amplitude_overlap", lambda spins, *a: "overlap " + spins)
    monkeypatch.setattr(sampled_components, "solve_and_test_model", solve)

    class Hamiltonian:
        basis = None

    clusters = [[1, 2], [3], [4, 5]]
    staged = sampled_components.stage_clusters(clusters, Hamiltonian, None, None, "fn", 2, 0.25, 1,
                                               **({"greedy_batch": True} if greedy_batch else {}),
                                               external_field=True, build_batch=True, level_batch=True)
    assert [(c, m.name) for c, m, _, _, _ in staged] == [
        (0, "m1"), (0, "m1+s"), (0, "m1+s+s"), (1, "m3"), (1, "m3+s"), (1, "m3+s+s"),
        (2, "m4"), (2, "m4+s"), (2, "m4+s+s")]
    assert [r.greedy_accuracy for _, _, _, _, r in staged] == [m.name for _, m, _, _, _ in staged]
    field = {"external_field": True}
    assert calls == [
        ("models", clusters, "fn", field),
        ("level", ["m1", "m3", "m4"], "fn", 0.25, clusters, field),
        ("level", ["m1+s", "m3+s", "m4+s"], "fn", 0.25, clusters, field)]
    # without external_field the keyword is absent
    del calls[:]
    sampled_components.stage_clusters(clusters, Hamiltonian, None, None, "fn", 1, 0.25, 1,
                                      **({"greedy_batch": True} if greedy_batch else {}), build_batch=True,
                                      level_batch=True)
    assert calls == [("models", clusters, "fn", {}), ("level", ["m1", "m3", "m4"], "fn", 0.25, clusters, {})]
    assert sampled_components.stage_clusters([], Hamiltonian, None, None, "fn", 2, 0.25, 1, build_batch=True,
                                             level_batch=True) == []
