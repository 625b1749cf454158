"""Batched parallel tempering (asp_sa_chains_advance_ladder_batch / _exchange_batch, annealer
.advance_ladder_chains / .exchange_chains / .parallel_tempering_batch, the `method` of
common.solve_ising_models and --anneal-method; DESIGN.md §4.12 "Batched forms"): what can be checked
without a device — the symbols, the header against the bindings, the validation that runs before any
device work, and the argument checks of the Python layer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_chains_advance_ladder_batch", "asp_sa_chains_exchange_batch", "asp_sa_chains_exchange_last_ms")
C_TYPES = {"asp_sa_chains *": ctypes.c_void_p, "double const *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
           "uint32_t *": ctypes.c_void_p, "double *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}


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


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_chains_advance_ladder_batch\s*\(\s*asp_sa_chains_ladder_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_chains_exchange_batch\s*\(\s*asp_sa_chains_exchange_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_chains_exchange_last_ms\s*\(\s*void\s*\)\s*;", header)
    u32 = ctypes.c_uint32
    assert _lib.SIGNATURES["asp_sa_chains_advance_ladder_batch"] == (ctypes.c_int,
                                                                      [ctypes.POINTER(_lib.SaChainsLadderItem), u32])
    assert _lib.SIGNATURES["asp_sa_chains_exchange_batch"] == (ctypes.c_int,
                                                                [ctypes.POINTER(_lib.SaChainsExchangeItem), u32])
    assert _lib.SIGNATURES["asp_sa_chains_exchange_last_ms"] == (ctypes.c_float, [])
    # declared next to the single-handle calls
    assert header.index("int asp_sa_chains_advance_ladder(") < header.index("int asp_sa_chains_advance_ladder_batch(") \
        < header.index("int asp_sa_chains_result(")
    assert header.index("int asp_sa_chains_exchange(") < header.index("int asp_sa_chains_exchange_batch(") \
        < header.index("asp_sa_batch_item")


@pytest.mark.parametrize("c_name,mirror", [("asp_sa_chains_ladder_item", "SaChainsLadderItem"),
                                           ("asp_sa_chains_exchange_item", "SaChainsExchangeItem")])
def test_structure_layouts_agree_with_the_header(c_name, mirror):
    from annealing_sign_problem_amd import _lib

    structure = getattr(_lib, mirror)
    assert [(name, ctype) for name, ctype in structure._fields_] == _header_fields(c_name)
    # natural alignment: three 32-bit words behind two pointers, one word of padding, three pointers
    assert ctypes.sizeof(structure) == 56
    offsets = [getattr(structure, name).offset for name, _ in structure._fields_]
    assert offsets == [0, 8, 16, 20, 24, 32, 40, 48]


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common

    for name in ("advance_ladder_chains", "exchange_chains", "parallel_tempering_batch"):
        assert name in sa.__all__ and callable(getattr(sa, name))
    assert list(inspect.signature(sa.advance_ladder_chains).parameters) == ["chains", "chain_betas", "number_sweeps",
                                                                            "sweep_order", "progress"]
    assert list(inspect.signature(sa.exchange_chains).parameters) == ["chains", "chain_betas", "parity", "draws"]
    assert inspect.signature(sa.exchange_chains).parameters["draws"].default == 0
    single = inspect.signature(sa.parallel_tempering).parameters
    batch = inspect.signature(sa.parallel_tempering_batch).parameters
    assert list(batch) == ["hamiltonians"] + list(single)[1:]
    assert all(batch[k].default == single[k].default for k in list(single)[1:])
    assert inspect.signature(common.solve_ising_models).parameters["method"].default == "anneal"


def test_count_zero_needs_no_device_and_null_items_are_invalid():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    assert lib.asp_sa_chains_advance_ladder_batch(None, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_exchange_batch(None, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_exchange_last_ms() == 0.0 and lib.asp_sa_chains_batch_last_ms() == 0.0
    assert lib.asp_sa_chains_advance_ladder_batch(None, ctypes.c_uint32(2)) == INVALID
    assert "null items" in _lib.last_error()
    assert lib.asp_sa_chains_exchange_batch(None, ctypes.c_uint32(2)) == INVALID
    assert "null items" in _lib.last_error()
    assert _lib.gpu_touched() == touched


def test_null_handles_and_flags_are_rejected_with_the_item_index_before_any_output_is_written():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    betas = np.ones(4)
    trace = np.full((4, 3), 77, dtype=np.int64)
    best = np.full(4, 77, dtype=np.int64)
    improved = ctypes.c_uint32(12345)
    ladder = (_lib.SaChainsLadderItem * 1)()
    ladder[0].chain_betas = betas.ctypes.data
    ladder[0].num_sweeps = 2
    ladder[0].out_trace = trace.ctypes.data
    ladder[0].out_tracked_best = best.ctypes.data
    ladder[0].out_improved = ctypes.addressof(improved)
    assert lib.asp_sa_chains_advance_ladder_batch(ladder, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null chains handle" in _lib.last_error()
    source = np.full(4, 77, dtype=np.uint32)
    energy = np.full(4, -77.0)
    accepted = ctypes.c_uint32(12345)
    exchange = (_lib.SaChainsExchangeItem * 1)()
    exchange[0].chain_betas = betas.ctypes.data
    exchange[0].out_source = source.ctypes.data
    exchange[0].out_energy = energy.ctypes.data
    exchange[0].out_accepted = ctypes.addressof(accepted)
    assert lib.asp_sa_chains_exchange_batch(exchange, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null chains handle" in _lib.last_error()
    exchange[0].flags = 4
    assert lib.asp_sa_chains_exchange_batch(exchange, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "flags" in _lib.last_error()
    assert np.all(trace == 77) and np.all(best == 77) and improved.value == 12345
    assert np.all(source == 77) and np.all(energy == -77.0) and accepted.value == 12345


def _closed_chains(repetitions=3):
    """A Chains object without a handle: the wrappers' checks run before the handle is looked at."""
    from annealing_sign_problem_amd import annealer as sa

    chains = sa.Chains.__new__(sa.Chains)
    chains._handle, chains.repetitions = None, repetitions
    return chains


def test_python_wrappers_validate_without_a_device():
    from annealing_sign_problem_amd import annealer as sa

    a, b = _closed_chains(), _closed_chains()
    good = [[1.0, 2.0, 3.0], [0.5, 0.0, 4.0]]
    # non-Chains entries
    with pytest.raises(TypeError):
        sa.advance_ladder_chains([a, "not chains"], good, 4, sweep_order="colour")
    with pytest.raises(TypeError):
        sa.exchange_chains([a, None], good, 0)
    # length mismatches
    with pytest.raises(ValueError):
        sa.advance_ladder_chains([a, b], good[:1], 4, sweep_order="colour")
    with pytest.raises(ValueError):
        sa.advance_ladder_chains([a, b], good, [4, 4, 4], sweep_order="colour")
    with pytest.raises(ValueError):
        sa.advance_ladder_chains([a, b], good, 4, sweep_order=["colour"])
    with pytest.raises(ValueError):
        sa.exchange_chains([a, b], good[:1], 0)
    with pytest.raises(ValueError):
        sa.exchange_chains([a, b], good, [0, 1, 0])
    with pytest.raises(ValueError):
        sa.exchange_chains([a, b], good, 0, draws=[0])
    # the checks of the single calls, per handle
    with pytest.raises(ValueError, match="chain_betas"):
        sa.advance_ladder_chains([a, b], [good[0], [1.0, 2.0]], 4, sweep_order="colour")
    with pytest.raises(ValueError, match="chain_betas"):
        sa.exchange_chains([a, b], [good[0], [1.0, np.inf, 2.0]], 0)
    with pytest.raises(ValueError, match="sweep_order"):
        sa.advance_ladder_chains([a, b], good, 4, sweep_order="random")
    with pytest.raises(ValueError, match="number_sweeps"):
        sa.advance_ladder_chains([a, b], good, [4, -1], sweep_order="colour")
    with pytest.raises(ValueError, match="parity"):
        sa.exchange_chains([a, b], good, [0, 2])
    # draws beyond 32 bits
    with pytest.raises(ValueError, match="draws"):
        sa.exchange_chains([a, b], good, 0, draws=2 ** 32)
    with pytest.raises(ValueError, match="draws"):
        sa.exchange_chains([a, b], good, 0, draws=[0, -1])
    # everything valid: the first thing that needs a device is the handle
    with pytest.raises(ValueError, match="closed"):
        sa.advance_ladder_chains([a, b], good, [4, 5], sweep_order=["colour", "shuffled"])
    with pytest.raises(ValueError, match="closed"):
        sa.exchange_chains([a, b], good, [0, 1], draws=[3, 2 ** 32 - 1])
    # the driver
    with pytest.raises(ValueError):
        sa.parallel_tempering_batch([], sweep_order="random")
    with pytest.raises(ValueError):
        sa.parallel_tempering_batch([], number_rounds=0)
    with pytest.raises(ValueError):
        sa.parallel_tempering_batch([], sweeps_per_round=0)
    with pytest.raises(TypeError):
        sa.parallel_tempering_batch(["not a Hamiltonian"], sweep_order="colour")
    with pytest.raises(ValueError):
        sa.parallel_tempering_batch([], repetitions=0, sweep_order="colour")
    assert sa.parallel_tempering_batch([], sweep_order="colour") == []


def test_solve_ising_models_rejects_bad_methods_without_a_device():
    from annealing_sign_problem_amd import common

    with pytest.raises(ValueError, match="method"):
        common.solve_ising_models([], method="quench")
    for method in ("population", "tempering"):
        with pytest.raises(ValueError, match="patience"):
            common.solve_ising_models([], method=method, patience=2)
        with pytest.raises(ValueError, match="number_sweeps"):
            common.solve_ising_models([], method=method, number_sweeps=9)
        with pytest.raises(ValueError, match="mode"):
            common.solve_ising_models([], method=method, mode="greedy")


NEEDS_BATCH = "needs --annealing and --batch > 1"
NO_PATIENCE = "cannot be combined with --anneal-patience"


@pytest.mark.parametrize("extra,message", [
    (["--anneal-method", "tempering", "--no-annealing"], "--anneal-method tempering " + NEEDS_BATCH),
    (["--anneal-method", "population", "--no-annealing"], "--anneal-method population " + NEEDS_BATCH),
    (["--anneal-method", "tempering", "--batch", "1"], "--anneal-method tempering " + NEEDS_BATCH),
    (["--anneal-method", "population", "--batch", "1"], "--anneal-method population " + NEEDS_BATCH),
    (["--anneal-method", "tempering", "--anneal-patience", "2"], "--anneal-method tempering " + NO_PATIENCE),
    (["--anneal-method", "population", "--anneal-patience", "2"], "--anneal-method population " + NO_PATIENCE),
    (["--anneal-method", "quench"], "invalid choice: 'quench'")])
def test_sampled_components_rejects_the_combinations_that_cannot_act(extra, message, capsys):
    from annealing_sign_problem_amd import sampled_components

    base = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1"]
    with pytest.raises(SystemExit) as error:
        sampled_components.parse_command_line(base + extra)
    assert error.value.code == 2
    assert message in " ".join(capsys.readouterr().err.split())  # (argparse wraps long messages)


def test_the_method_reaches_solve_ising_models_through_the_staged_annealing(monkeypatch):
    """--anneal-method travels as early_stop_of(args) -> process_clusters_batched / anneal_staged ->
    common.solve_ising_models(method=...): the whole route, with the solver and the scoring replaced."""
    from annealing_sign_problem_amd import common, sampled_components

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
    base = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1", "--sweep-order", "colour"]
    clusters = [[1, 2], [3]]
    for extra, want in ((["--anneal-method", "tempering"], {"method": "tempering"}),
                        (["--anneal-method", "population"], {"method": "population"}),
                        (["--anneal-patience", "3"], {"patience": 3, "check_every": None}),
                        ([], {})):
        args = sampled_components.parse_command_line(base + extra)
        results = [sampled_components.OptimizationResult(3, 0.0, 0.0, 0.0, 0.0, 0.0) for _ in range(3)]
        staged = [(0, Model, "s0", None, results[0]), (1, Model, "s1", None, results[1]), (1, Model, "s2", None, results[2])]
        monkeypatch.setattr(sampled_components, "stage_clusters", lambda *a, **k: staged)
        out = sampled_components.process_clusters_batched(clusters, None, None, None, None, 1, 1e-4, True,
                                                          sweep_order=args.sweep_order,
                                                          **sampled_components.early_stop_of(args))
        count, frozen, kw = seen.pop()
        assert not seen and count == 3 and frozen == [[1, 2], [3], [3]]
        assert kw == dict(sweep_order="colour", **want)
        assert out == [[results[0]], [results[1], results[2]]]
        assert [r.sa_accuracy for r in results] == ["x0", "x1", "x2"] and [r.sa_overlap for r in results] == ["s0", "s1", "s2"]


def test_sampled_components_passes_the_method_on_like_the_patience():
    from annealing_sign_problem_amd import sampled_components

    base = ["--model", "heisenberg_kagome_16", "--output", "unused.csv", "--order", "1"]
    args = sampled_components.parse_command_line(base)
    assert args.anneal_method == "anneal" and sampled_components.early_stop_of(args) == {}
    for method in ("population", "tempering"):
        args = sampled_components.parse_command_line(base + ["--anneal-method", method])
        assert sampled_components.early_stop_of(args) == {"early_stop": {"method": method}}
    args = sampled_components.parse_command_line(base + ["--anneal-patience", "3"])
    assert sampled_components.early_stop_of(args) == {"early_stop": {"patience": 3, "check_every": None}}
