"""Batched isoenergetic cluster moves (asp_sa_chains_cluster_move_batch, annealer.cluster_move_chains /
.parallel_tempering_cluster_batch, method="tempering-cluster" of common.solve_ising_models and
--anneal-method tempering-cluster; DESIGN.md §4.13 "Batched form"): what can be checked without a
device — the symbols, the header against the bindings, the validation that needs no handle, and the
argument checks of the Python layer.  The validation that needs a live handle (slots, the same handle
twice) is in tests/test_gpu_cluster_move_batch.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_chains_cluster_move_batch", "asp_sa_chains_cluster_move_batch_last_ms")
C_TYPES = {"asp_sa_chains *": ctypes.c_void_p, "uint32_t const *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
           "uint32_t *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def _header_fields(name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` as the header declares it."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for declaration in body.split(";"):
        declaration = " ".join(declaration.split())
        if not declaration:
            continue
        match = re.match(r"(.*?[\s\*])(\w+(?:\s*,\s*\w+)*)$", declaration)
        ctype = " ".join(match.group(1).split())
        for field in match.group(2).split(","):
            fields.append((field.strip(), C_TYPES[ctype]))
    return fields


def test_library_exports_and_header_declares_the_two_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_chains_cluster_move_batch\s*\(\s*asp_sa_chains_cluster_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_chains_cluster_move_batch_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert re.search(r"#define\s+ASP_CLUSTER_NO_PACKED\s+1u", header)
    assert _lib.SIGNATURES["asp_sa_chains_cluster_move_batch"] == (ctypes.c_int,
                                                                    [ctypes.POINTER(_lib.SaChainsClusterItem),
                                                                     ctypes.c_uint32])
    assert _lib.SIGNATURES["asp_sa_chains_cluster_move_batch_last_ms"] == (ctypes.c_float, [])
    # declared next to the single call
    assert header.index("int asp_sa_chains_cluster_move(") < header.index("int asp_sa_chains_cluster_move_batch(") \
        < header.index("asp_sa_batch_item")


def test_structure_layout_agrees_with_the_header():
    from annealing_sign_problem_amd import _lib

    structure = _lib.SaChainsClusterItem
    assert [(name, ctype) for name, ctype in structure._fields_] == _header_fields("asp_sa_chains_cluster_item")
    # natural alignment: three 32-bit words behind two pointers, one word of padding, three pointers
    assert ctypes.sizeof(structure) == 56
    assert [getattr(structure, name).offset for name, _ in structure._fields_] == [0, 8, 16, 20, 24, 32, 40, 48]


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common

    for name in ("cluster_move_chains", "parallel_tempering_cluster_batch"):
        assert name in sa.__all__ and callable(getattr(sa, name))
    parameters = inspect.signature(sa.cluster_move_chains).parameters
    assert list(parameters)[:3] == ["chains", "pairs", "draws"] and parameters["draws"].default == 0
    assert all(p.default == 0 for name, p in parameters.items() if name not in ("chains", "pairs"))
    assert sa.CLUSTER_NO_PACKED == 1
    single = inspect.signature(sa.parallel_tempering_cluster).parameters
    batch = inspect.signature(sa.parallel_tempering_cluster_batch).parameters
    assert list(batch) == ["hamiltonians"] + list(single)[1:]
    assert all(batch[k].default == single[k].default for k in list(single)[1:])
    assert inspect.signature(common.solve_ising_models).parameters["method"].default == "anneal"


def _item(lib_module, num_pairs=2, sentinel=77):
    """One item with outputs full of a sentinel: (items, (differing, sizes, deltas), keep-alive)."""
    pairs = np.array([0, 1, 2, 3], dtype=np.uint32)
    differing = np.full(num_pairs, sentinel, dtype=np.uint32)
    sizes = np.full(num_pairs, sentinel, dtype=np.uint32)
    deltas = np.full(num_pairs, -sentinel, dtype=np.int64)
    items = (lib_module.SaChainsClusterItem * 1)()
    items[0].pairs = pairs.ctypes.data
    items[0].num_pairs = num_pairs
    items[0].out_differing = differing.ctypes.data
    items[0].out_size = sizes.ctypes.data
    items[0].out_delta = deltas.ctypes.data
    return items, (differing, sizes, deltas), pairs


def test_count_zero_needs_no_device_and_null_items_are_invalid():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    assert lib.asp_sa_chains_cluster_move_batch(None, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_cluster_move_batch_last_ms() == 0.0
    items, _, _keep = _item(_lib)
    assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_cluster_move_batch(None, ctypes.c_uint32(2)) == INVALID
    assert "null items" in _lib.last_error()
    assert _lib.gpu_touched() == touched


def test_null_handles_and_flags_are_rejected_with_the_item_index_before_any_output_is_written():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    items, outputs, _keep = _item(_lib)
    assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null chains handle" in _lib.last_error()
    items[0].flags = 1  # ASP_CLUSTER_NO_PACKED is a known flag: the handle is what is wrong
    assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null chains handle" in _lib.last_error()
    for flags in (2, 4, 3, 0x80000000):
        items[0].flags = flags
        assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(1)) == INVALID
        assert "item 0" in _lib.last_error() and "flags" in _lib.last_error()
    differing, sizes, deltas = outputs
    assert np.all(differing == 77) and np.all(sizes == 77) and np.all(deltas == -77)
    assert lib.asp_sa_chains_cluster_move_batch_last_ms() == 0.0
    assert _lib.gpu_touched() == touched


def _closed_chains(repetitions=5):
    """A Chains object without a handle: the wrappers' checks run before the handle is looked at."""
    from annealing_sign_problem_amd import annealer as sa

    chains = sa.Chains.__new__(sa.Chains)
    chains._handle, chains.repetitions = None, repetitions
    return chains


def test_cluster_move_chains_validates_without_a_device():
    from annealing_sign_problem_amd import annealer as sa

    a, b = _closed_chains(), _closed_chains()
    good = [[[0, 1], [3, 2]], [[4, 0]]]
    with pytest.raises(TypeError):
        sa.cluster_move_chains([a, "not chains"], good)
    # wrong lengths
    with pytest.raises(ValueError):
        sa.cluster_move_chains([a, b], good[:1])
    with pytest.raises(ValueError):
        sa.cluster_move_chains([a, b], good, draws=[0])
    with pytest.raises(ValueError):
        sa.cluster_move_chains([a, b], good, draws=[0, 1, 2])
    # wrong shapes and entries: the checks of Chains.cluster_move, per handle
    for bad in ([0, 1], [[0, 1, 2]], [[0.0, 1.0]], [[0, 5]], [[-1, 2]], [[0, 1], [2, 0]], [[3, 3]]):
        with pytest.raises(ValueError, match="pairs"):
            sa.cluster_move_chains([a, b], [good[0], bad])
    # draws beyond 32 bits
    with pytest.raises(ValueError, match="draws"):
        sa.cluster_move_chains([a, b], good, draws=2 ** 32)
    with pytest.raises(ValueError, match="draws"):
        sa.cluster_move_chains([a, b], good, draws=[0, -1])
    with pytest.raises(ValueError, match="flags"):
        sa.cluster_move_chains([a, b], good, flags=2)
    # everything valid: the first thing that needs a device is the handle
    with pytest.raises(ValueError, match="closed"):
        sa.cluster_move_chains([a, b], good, draws=[3, 2 ** 32 - 1])
    with pytest.raises(ValueError, match="closed"):
        sa.cluster_move_chains([a, b], [[], np.zeros((0, 2), dtype=np.int64)], flags=sa.CLUSTER_NO_PACKED)
    assert sa.cluster_move_chains([], []) == []


def test_the_batched_driver_validates_without_a_device():
    from annealing_sign_problem_amd import annealer as sa

    with pytest.raises(ValueError):
        sa.parallel_tempering_cluster_batch([], sweep_order="random")
    with pytest.raises(ValueError):
        sa.parallel_tempering_cluster_batch([], number_rounds=0)
    with pytest.raises(ValueError):
        sa.parallel_tempering_cluster_batch([], sweeps_per_round=0)
    with pytest.raises(TypeError):
        sa.parallel_tempering_cluster_batch(["not a Hamiltonian"], sweep_order="colour")
    for odd in (7, 1, 0):
        with pytest.raises(ValueError, match="even"):
            sa.parallel_tempering_cluster_batch([], repetitions=odd, sweep_order="colour")
    for rungs in (5, -1):
        with pytest.raises(ValueError, match="cluster_rungs"):
            sa.parallel_tempering_cluster_batch([], repetitions=8, cluster_rungs=rungs, sweep_order="colour")
    ham = sa.Hamiltonian(scipy.sparse.identity(4, format="csr"), np.zeros(4))
    with pytest.raises(ValueError, match="own Hamiltonian"):
        sa.parallel_tempering_cluster_batch([ham, ham], repetitions=8, beta0=1.0, beta1=2.0, sweep_order="colour")
    assert sa.parallel_tempering_cluster_batch([], sweep_order="colour") == []


def test_solve_ising_models_rejects_what_the_method_cannot_do_without_a_device():
    from annealing_sign_problem_amd import common

    with pytest.raises(ValueError, match="method") as error:
        common.solve_ising_models([], method="quench")
    assert "tempering-cluster" in str(error.value)
    with pytest.raises(ValueError, match="patience"):
        common.solve_ising_models([], method="tempering-cluster", patience=2)
    with pytest.raises(ValueError, match="number_sweeps"):
        common.solve_ising_models([], method="tempering-cluster", number_sweeps=9)
    with pytest.raises(ValueError, match="mode"):
        common.solve_ising_models([], method="tempering-cluster", mode="greedy")
    with pytest.raises(ValueError, match="even"):
        common.solve_ising_models([], method="tempering-cluster", repetitions=7, sweep_order="colour")
    assert common.solve_ising_models([], method="tempering-cluster", sweep_order="colour") == []


NEEDS_BATCH = "--anneal-method tempering-cluster needs --annealing and --batch > 1"
NO_PATIENCE = "--anneal-method tempering-cluster cannot be combined with --anneal-patience"
BASE = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1"]


@pytest.mark.parametrize("extra,message", [
    (["--anneal-method", "tempering-cluster", "--no-annealing"], NEEDS_BATCH),
    (["--anneal-method", "tempering-cluster", "--batch", "1"], NEEDS_BATCH),
    (["--anneal-method", "tempering-cluster", "--anneal-patience", "2"], NO_PATIENCE)])
def test_sampled_components_refuses_the_choice_where_it_refuses_tempering(extra, message, capsys):
    from annealing_sign_problem_amd import sampled_components

    with pytest.raises(SystemExit) as error:
        sampled_components.parse_command_line(BASE + extra)
    assert error.value.code == 2
    assert message in " ".join(capsys.readouterr().err.split())  # (argparse wraps long messages)
    # ... exactly where it refuses the plain tempering
    with pytest.raises(SystemExit):
        sampled_components.parse_command_line(BASE + ["tempering" if x == "tempering-cluster" else x for x in extra])


def test_the_choice_reaches_solve_ising_models_through_the_staged_annealing(monkeypatch):
    from annealing_sign_problem_amd import common, sampled_components

    args = sampled_components.parse_command_line(BASE)
    assert args.anneal_method == "anneal" and sampled_components.early_stop_of(args) == {}
    args = sampled_components.parse_command_line(BASE + ["--sweep-order", "colour", "--anneal-method", "tempering-cluster"])
    assert sampled_components.early_stop_of(args) == {"early_stop": {"method": "tempering-cluster"}}

    class Model:
        size = 3

        class ising_hamiltonian:
            release = staticmethod(lambda: None)

    seen = []

    def solve(models, frozen, **kw):
        seen.append((len(models), [list(f) for f in frozen], kw))
        return ["x%d" % k for k in range(len(models))]

    monkeypatch.setattr(common, "solve_ising_models", solve)
    monkeypatch.setattr(common, "compute_accuracy_and_overlap", lambda x, signs, weights: (x, signs))
    results = [sampled_components.OptimizationResult(3, 0.0, 0.0, 0.0, 0.0, 0.0) for _ in range(3)]
    staged = [(0, Model, "s0", None, results[0]), (1, Model, "s1", None, results[1]), (1, Model, "s2", None, results[2])]
    monkeypatch.setattr(sampled_components, "stage_clusters", lambda *a, **k: staged)
    out = sampled_components.process_clusters_batched([[1, 2], [3]], None, None, None, None, 1, 1e-4, True,
                                                      sweep_order=args.sweep_order,
                                                      **sampled_components.early_stop_of(args))
    count, frozen, kw = seen.pop()
    assert not seen and count == 3 and frozen == [[1, 2], [3], [3]]
    assert kw == dict(sweep_order="colour", method="tempering-cluster")
    assert out == [[results[0]], [results[1], results[2]]]
