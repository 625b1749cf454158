"""The C ABI of the segmented coupling build (asp_operator_ising_segments, include/asp.h) without a
device: the symbol, the header against the bindings, every validation branch — all of which run before any device
work and before any output is written —, the call that needs no device, the Python surface and the --build-batch
plumbing."""
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


class _Outputs:
    def __init__(self, rows, capacity=8):
        self.capacity = capacity
        self.indptr = np.full(rows + 1, -77, dtype=np.int64)
        self.col = np.full(capacity, -5, dtype=np.int32)
        self.val = np.full(capacity, 12345.5)
        self.nnz = ctypes.c_uint64(991)

    def untouched(self):
        return bool(np.all(self.indptr == -77) and np.all(self.col == -5) and np.all(self.val == 12345.5)
                    and self.nnz.value == 991)


def _call(op, offsets, keys, psi, out, segments=None, nnz=True):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    segments = (0 if offsets is None else offsets.size - 1) if segments is None else segments
    return lib.asp_operator_ising_segments(
        op, segments, _lib.ptr(offsets), _lib.ptr(keys), _lib.ptr(psi), out.capacity if out else 0,
        _lib.ptr(out.indptr) if out else None, _lib.ptr(out.col) if out else None, _lib.ptr(out.val) if out else None,
        ctypes.byref(out.nnz) if out and nnz else None)


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_symbol():
    from annealing_sign_problem_amd import _lib, build

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    assert "asp_operator_ising_segments" in _lib.SIGNATURES and hasattr(lib, "asp_operator_ising_segments")
    assert raw.asp_operator_ising_segments is not None
    text = _header()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int asp_operator_ising_segments(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets, "
            "uint64_t const *keys, double const *psi, uint64_t capacity, int64_t *indptr, int32_t *col, double *val, "
            "uint64_t *nnz);") in header
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_operator_ising_segments"] == (ctypes.c_int,
                                                              [p, u64, p, p, p, u64, p, p, p, ctypes.POINTER(u64)])
    assert "ASP-ISING-SEG-1" in text
    assert "operator_ising_segments.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "operator_ising_segments.hip"))


def test_every_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    offsets = _u64([0, 3, 3, 5])
    keys = _u64([3, 5, 6, 5, 9])
    psi = np.array([0.6, -0.8, 0.0, 0.6, 0.8])
    out = _Outputs(5)

    def refused(message, *args, **keywords):
        assert _call(*args, **keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert out.untouched()

    refused("null operator", None, offsets, keys, psi, out)
    refused("null nnz pointer", FAKE, offsets, keys, psi, out, nnz=False)
    refused("null offsets with 3 segments", FAKE, None, keys, psi, out, segments=3)
    refused("offsets[0] is not 0", FAKE, _u64([1, 3, 3, 5]), keys, psi, out)
    refused("offsets decrease at index 2", FAKE, _u64([0, 3, 2, 5]), keys, psi, out)
    refused("offsets decrease at index 3", FAKE, _u64([0, 3, 3, 2]), keys, psi, out)
    refused("null keys or psi with 5 table entries", FAKE, offsets, None, psi, out)
    refused("null keys or psi with 5 table entries", FAKE, offsets, keys, None, out)
    refused("the keys of segment 0 are not sorted and unique at index 2", FAKE, offsets, _u64([3, 6, 5, 5, 9]), psi, out)
    refused("the keys of segment 0 are not sorted and unique at index 1", FAKE, offsets, _u64([3, 3, 6, 5, 9]), psi, out)
    refused("the keys of segment 2 are not sorted and unique at index 1", FAKE, offsets, _u64([3, 5, 6, 9, 5]), psi, out)
    # (a key that repeats in ANOTHER segment is legal — entries 1 and 3 hold state 5: tests/test_gpu_ising_segments.py)
    assert _lib.gpu_touched() == touched


def test_a_table_beyond_the_index_range_is_refused():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    code = int(re.search(r"ASP_ERR_TOO_LARGE\s*=\s*(-?\d+)", _header()).group(1))
    out = _Outputs(1)
    # T = 2^31 - 1 (only the offsets say so: nothing of that length is read before the size check)
    assert _call(FAKE, _u64([0, 2 ** 31 - 1]), _u64([3]), np.array([1.0]), out) == code
    assert "2^31" in _lib.last_error() and out.untouched()
    assert _lib.gpu_touched() == touched


def test_an_empty_table_needs_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    for offsets in (None, _u64([0]), _u64([0, 0, 0])):
        out = _Outputs(0)
        assert _call(FAKE, offsets, None, None, out) == 0 and lib.asp_last_error_code() == 0
        assert out.nnz.value == 0 and out.indptr.tolist() == [0]
        assert np.all(out.col == -5) and np.all(out.val == 12345.5)
    # a sizing call of nothing
    nnz = ctypes.c_uint64(7)
    assert lib.asp_operator_ising_segments(FAKE, 0, None, None, None, 0, None, None, None, ctypes.byref(nnz)) == 0
    assert nnz.value == 0
    assert _call(None, None, None, None, _Outputs(0)) == INVALID
    assert _lib.gpu_touched() == touched


class _Foreign:
    """An operator object that is not this package's: only its own batched_apply."""

    class basis:
        number_spins = 4

    def batched_apply(self, spins):
        raise AssertionError("not reached")


def test_python_surface(monkeypatch):
    from annealing_sign_problem_amd import _lib, common, operators, sampled_components

    touched = _lib.gpu_touched()
    assert list(inspect.signature(operators.DeviceOperator.ising_csr_segments).parameters) == [
        "self", "keys", "psi", "offsets"]
    parameters = inspect.signature(common.make_ising_models).parameters
    assert list(parameters) == ["clusters", "quantum_hamiltonian", "log_psis", "log_psi_fn", "external_field"]
    assert parameters["log_psis"].default is None and parameters["log_psi_fn"].default is None
    assert parameters["external_field"].default is False
    parameters = inspect.signature(common.make_hamiltonian_extensions).parameters
    assert list(parameters) == ["models", "log_psi_fn", "external_field"] and parameters["external_field"].default is False
    assert "make_ising_models" in common.__all__ and "make_hamiltonian_extensions" in common.__all__
    for function in (sampled_components.stage_clusters, sampled_components.process_clusters_batched):
        assert inspect.signature(function).parameters["build_batch"].default is False
    # a foreign operator object takes the loop of make_ising_model, cluster by cluster, with the same arguments
    seen = []

    def one(spins, hamiltonian, log_psi=None, log_psi_fn=None, external_field=False):
        seen.append((list(spins), hamiltonian, log_psi, log_psi_fn, external_field))
        return "model %d" % len(seen)

    monkeypatch.setattr(common, "make_ising_model", one)
    foreign, fn = _Foreign(), (lambda spins: np.zeros(len(spins)))
    assert common.make_ising_models([[3, 5], [6]], foreign, log_psi_fn=fn) == ["model 1", "model 2"]
    assert seen == [([3, 5], foreign, None, fn, False), ([6], foreign, None, fn, False)]
    del seen[:]
    assert common.make_ising_models([[9]], foreign, log_psis=["l"], external_field=True) == ["model 1"]
    assert seen == [([9], foreign, "l", None, True)]
    assert common.make_ising_models([], foreign, log_psi_fn=fn) == []
    with pytest.raises(ValueError, match="one array per cluster"):
        common.make_ising_models([[3]], foreign, log_psis=[])
    assert common.make_hamiltonian_extensions([], fn) == []
    assert _lib.gpu_touched() == touched


BASE = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1"]


def test_the_flag_travels_as_a_keyword_that_is_absent_without_it(monkeypatch):
    """--build-batch -> build_batch_of(args) -> process_clusters_batched -> stage_clusters(build_batch=True); without
    the flag no new keyword is passed anywhere."""
    from annealing_sign_problem_amd import sampled_components

    args = sampled_components.parse_command_line(BASE)
    assert args.build_batch is False and sampled_components.build_batch_of(args) == {}
    args = sampled_components.parse_command_line(BASE + ["--build-batch"])
    assert args.build_batch is True and sampled_components.build_batch_of(args) == {"build_batch": True}
    assert sampled_components.build_batch_of(object()) == {}
    seen = []

    def stage(clusters, hamiltonian, ground_state, noisy_ground_state, noisy_log_coeff_fn, order, global_cutoff,
              jobs=1, **keywords):
        seen.append(keywords)
        return []

    monkeypatch.setattr(sampled_components, "stage_clusters", stage)
    for extra, want in (([], {}), (["--build-batch"], {"build_batch": True}),
                        (["--build-batch", "--greedy-batch", "--external-field"],
                         {"build_batch": True, "greedy_batch": True, "external_field": True})):
        args = sampled_components.parse_command_line(BASE + extra)
        out = sampled_components.process_clusters_batched(
            [[1], [2]], None, None, None, None, 1, 1e-4, False, jobs=1, sweep_order=args.sweep_order,
            **({"greedy_batch": True} if args.greedy_batch else {}), **sampled_components.early_stop_of(args),
            **sampled_components.external_field_of(args), **sampled_components.build_batch_of(args))
        assert out == [[], []] and seen.pop() == want and not seen


@pytest.mark.parametrize("extra", [["--batch", "1"], ["--no-annealing"]])
def test_the_flag_needs_rounds_of_clusters(extra, capsys):
    from annealing_sign_problem_amd import sampled_components

    with pytest.raises(SystemExit) as error:
        sampled_components.parse_command_line(BASE + ["--build-batch"] + extra)
    assert error.value.code == 2
    assert "--build-batch needs --batch > 1" in " ".join(capsys.readouterr().err.split())
    sampled_components.parse_command_line(BASE + ["--build-batch", "--no-annealing", "--greedy-batch"])


@pytest.mark.parametrize("greedy_batch", [False, True])
def test_stage_clusters_builds_level_by_level(monkeypatch, greedy_batch):
    """With build_batch the models of one order of ALL clusters come from one make_ising_models /
    make_hamiltonian_extensions call; the staged list keeps its order (cluster by cluster, orders ascending)."""
    from annealing_sign_problem_amd import common, sampled_components

    class Model:
        basis_index = None

        def __init__(self, name):
            self.name, self.spins, self.size = name, name, 3

    calls = []

    def many(clusters, hamiltonian, log_psis=None, log_psi_fn=None, **keywords):
        calls.append(("models", [list(c) for c in clusters], log_psi_fn, keywords))
        return [Model("m%d" % c[0]) for c in clusters]

    def extensions(models, log_psi_fn, **keywords):
        calls.append(("extensions", [m.name for m in models], log_psi_fn, keywords))
        return [Model(m.name + "+") for m in models]

    def sparsify(model, cutoff, cluster):
        calls.append(("sparsify", model.name, cutoff, list(cluster)))
        return Model(model.name + "s")

    def single(*a, **k):
        raise AssertionError("the per-cluster builders are not used")

    def solve(h, cluster, exact_signs, weights, annealing):
        assert not greedy_batch and annealing is False
        return sampled_components.OptimizationResult(h.size, h.name, exact_signs, 0.0, 0.0, 0.0)

    monkeypatch.setattr(common, "make_ising_models", many)
    monkeypatch.setattr(common, "make_hamiltonian_extensions", extensions)
    monkeypatch.setattr(common, "sparsify_using_global_cutoff", sparsify)
    monkeypatch.setattr(common, "make_ising_model", single)
    monkeypatch.setattr(common, "make_hamiltonian_extension", single)
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
                                               external_field=True, build_batch=True)
    assert [(c, m.name) for c, m, _, _, _ in staged] == [
        (0, "m1"), (0, "m1+s"), (0, "m1+s+s"), (1, "m3"), (1, "m3+s"), (1, "m3+s+s"),
        (2, "m4"), (2, "m4+s"), (2, "m4+s+s")]
    assert [s for _, _, s, _, _ in staged] == [x for n in (1, 3, 4) for x in ["signs of m%d" % n] * 3]
    assert [r.greedy_accuracy for _, _, _, _, r in staged] == [m.name for _, m, _, _, _ in staged]
    assert [r.amplitude_overlap for _, _, _, _, r in staged] == ["overlap " + m.name for _, m, _, _, _ in staged]
    field = {"external_field": True}
    assert calls == [
        ("models", clusters, "fn", field),
        ("extensions", ["m1", "m3", "m4"], "fn", field),
        ("sparsify", "m1+", 0.25, [1, 2]), ("sparsify", "m3+", 0.25, [3]), ("sparsify", "m4+", 0.25, [4, 5]),
        ("extensions", ["m1+s", "m3+s", "m4+s"], "fn", field),
        ("sparsify", "m1+s+", 0.25, [1, 2]), ("sparsify", "m3+s+", 0.25, [3]), ("sparsify", "m4+s+", 0.25, [4, 5])]
    assert sampled_components.stage_clusters([], Hamiltonian, None, None, "fn", 2, 0.25, 1, build_batch=True) == []
