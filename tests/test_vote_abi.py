"""Consensus signs (include/asp.h: asp_sign_vote_batch, asp_sa_chains_vote_batch, asp_sign_vote_last_ms; law
ASP-VOTE-1): what can be checked without a device — the symbols and the header against
the bindings, the layout of the two items, every refusal (raised before any device work, so before the
missing device is noticed, and before any output is written), the calls that need no device at all, the
Python surface and the command-line flag."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
TOO_LARGE = -4
SYMBOLS = ("asp_sign_vote_batch", "asp_sa_chains_vote_batch", "asp_sign_vote_last_ms")
C_TYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "asp_sa_chains *": ctypes.c_void_p,
           "uint64_t const *": ctypes.c_void_p, "double const *": ctypes.c_void_p, "uint32_t *": ctypes.c_void_p,
           "uint8_t *": ctypes.c_void_p, "double *": ctypes.c_void_p, "uint64_t *": ctypes.c_void_p}
MARK = 77


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
        match = re.match(r"(.*?[\s\*])(\w+)$", declaration)
        fields.append((match.group(2), C_TYPES[" ".join(match.group(1).split())]))
    return fields


class _Outputs:
    """The seven outputs of an item, prefilled with a marker."""

    def __init__(self, spins=130, count=3):
        words = (spins + 63) // 64
        self.distance = np.full(max(count, 1), MARK, dtype=np.uint32)
        self.flipped = np.full(max(count, 1), MARK, dtype=np.uint8)
        self.ones = np.full(max(spins, 1), MARK, dtype=np.uint32)
        self.plus = np.full(max(spins, 1), float(MARK))
        self.minus = np.full(max(spins, 1), float(MARK))
        self.consensus = np.full(max(words, 1), MARK, dtype=np.uint64)
        self.changed = np.full(1, MARK, dtype=np.uint32)

    def arrays(self):
        return (self.distance, self.flipped, self.ones, self.plus, self.minus, self.consensus, self.changed)

    def untouched(self) -> bool:
        return all(bool(np.all(a == MARK)) for a in self.arrays())

    def attach(self, item) -> None:
        (item.out_distance, item.out_flipped, item.out_ones, item.out_plus, item.out_minus, item.out_consensus,
         item.out_changed) = (a.ctypes.data for a in self.arrays())


def _item(item, outputs, spins=130, count=3, x=None, stride=3, weights=None, ref=None, anchor=0, align=1, rounds=1):
    item.num_spins, item.count, item.x_stride = spins, count, stride
    item.x = None if x is None else x.ctypes.data
    item.weights = None if weights is None else weights.ctypes.data
    item.ref = None if ref is None else ref.ctypes.data
    item.anchor, item.align, item.rounds = anchor, align, rounds
    outputs.attach(item)


def _vote(**arguments):
    """Return code of a batch of one item, the message, and whether the outputs kept their marker."""
    from annealing_sign_problem_amd import _lib

    outputs = _Outputs(min(arguments.get("spins", 130), 1000), min(arguments.get("count", 3), 1000))
    items = (_lib.SignVoteItem * 1)()
    _item(items[0], outputs, **arguments)
    rc = _lib.load().asp_sign_vote_batch(items, ctypes.c_uint32(1))
    return rc, _lib.last_error(), outputs.untouched()


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sign_vote_batch\s*\(\s*asp_sign_vote_item\s+const\s*\*\s*items\s*,\s*uint32_t\s+count"
                     r"\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_chains_vote_batch\s*\(\s*asp_sa_chains_vote_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sign_vote_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert _lib.SIGNATURES["asp_sign_vote_batch"] == (ctypes.c_int, [ctypes.POINTER(_lib.SignVoteItem),
                                                                     ctypes.c_uint32])
    assert _lib.SIGNATURES["asp_sa_chains_vote_batch"] == (ctypes.c_int, [ctypes.POINTER(_lib.SaChainsVoteItem),
                                                                          ctypes.c_uint32])
    assert _lib.SIGNATURES["asp_sign_vote_last_ms"] == (ctypes.c_float, [])
    assert lib.asp_sign_vote_last_ms.restype is ctypes.c_float
    assert "ASP-VOTE-1" in header


def test_structure_layouts_agree_with_the_header():
    from annealing_sign_problem_amd import _lib

    item = _lib.SignVoteItem
    assert [(name, ctype) for name, ctype in item._fields_] == _header_fields("asp_sign_vote_item")
    assert ctypes.sizeof(item) == 120
    assert [getattr(item, name).offset for name, _ in item._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 64, 72, 80,
                                                                        88, 96, 104, 112]
    item = _lib.SaChainsVoteItem
    assert [(name, ctype) for name, ctype in item._fields_] == _header_fields("asp_sa_chains_vote_item")
    assert ctypes.sizeof(item) == 104
    assert [getattr(item, name).offset for name, _ in item._fields_] == [0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72, 80,
                                                                        88, 96]


def test_refusals_come_before_any_device_work():
    x = np.zeros((3, 3), dtype=np.uint64)
    ref = np.zeros(3, dtype=np.uint64)
    weights = np.ones(3)
    # a null x with configurations and spins
    assert _vote(x=None)[::2] == (INVALID, True)
    # a stride between 1 and W - 1
    for stride in (1, 2):
        rc, message, untouched = _vote(x=x, stride=stride)
        assert (rc, untouched) == (INVALID, True) and "x_stride" in message
    # weights that are negative, NaN or infinite
    for bad in (-1.0, -5e-324, np.nan, np.inf, -np.inf):
        wrong = weights.copy()
        wrong[2] = bad
        rc, message, untouched = _vote(x=x, weights=wrong)
        assert (rc, untouched) == (INVALID, True) and "weight 2" in message
    # no ref and an anchor that is no configuration; with a ref the anchor is not read
    for anchor in (3, 2**32 - 1):
        rc, message, untouched = _vote(x=x, anchor=anchor)
        assert (rc, untouched) == (INVALID, True) and "anchor" in message
    # rounds outside 1 .. 16
    for rounds in (0, 17, 2**32 - 1):
        rc, message, untouched = _vote(x=x, ref=ref, rounds=rounds)
        assert (rc, untouched) == (INVALID, True) and "rounds" in message
    # 2^31 spins or more; more than 2^20 configurations
    assert _vote(x=x, spins=2**31, stride=2**25)[::2] == (TOO_LARGE, True)
    assert _vote(x=x, count=2**20 + 1)[::2] == (TOO_LARGE, True)


def test_batch_refusals_name_the_item_and_null_arguments():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    x = np.zeros((3, 3), dtype=np.uint64)
    wrong = np.array([1.0, -2.0, 1.0])
    outputs = [_Outputs() for _ in range(3)]
    items = (_lib.SignVoteItem * 3)()
    for item, out in zip(items, outputs):
        _item(item, out, x=x)
    items[2].weights = wrong.ctypes.data
    assert lib.asp_sign_vote_batch(items, ctypes.c_uint32(3)) == INVALID
    assert "item 2" in _lib.last_error() and "weight 1" in _lib.last_error()
    items[2].weights = None
    items[1].rounds = 0
    assert lib.asp_sign_vote_batch(items, ctypes.c_uint32(3)) == INVALID
    assert "item 1" in _lib.last_error()
    assert all(out.untouched() for out in outputs)  # (items 0 and 2 were valid: nothing ran for them either)
    assert lib.asp_sign_vote_batch(None, ctypes.c_uint32(3)) == INVALID
    assert lib.asp_sa_chains_vote_batch(None, ctypes.c_uint32(1)) == INVALID
    handles = (_lib.SaChainsVoteItem * 2)()  # null handles
    for item in handles:
        item.rounds = 1
    assert lib.asp_sa_chains_vote_batch(handles, ctypes.c_uint32(2)) == INVALID
    assert "item 0" in _lib.last_error() and "handle" in _lib.last_error()


def test_nothing_to_do_needs_no_device():
    from annealing_sign_problem_amd import _lib, scores

    lib = _lib.load()
    touched = _lib.gpu_touched()
    assert lib.asp_sign_vote_batch(None, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_vote_batch(None, ctypes.c_uint32(0)) == 0
    # items without configurations: nothing is written, whatever the anchor
    rc, _, untouched = _vote(x=None, count=0, stride=0)
    assert (rc, untouched) == (0, True)
    # no spins: zeros per configuration and changed = 0; the per-site outputs have no entries
    outputs = _Outputs(0, 3)
    items = (_lib.SignVoteItem * 1)()
    _item(items[0], outputs, spins=0, count=3, x=None, stride=0, anchor=2)
    assert lib.asp_sign_vote_batch(items, ctypes.c_uint32(1)) == 0
    assert not outputs.distance.any() and not outputs.flipped.any() and outputs.changed[0] == 0
    assert np.all(outputs.ones == MARK) and np.all(outputs.consensus == MARK)
    # the Python layer
    assert scores.consensus_batch([]) == []
    empty = scores.consensus(np.zeros((0, 3), dtype=np.uint64), 130)
    assert empty.x.shape == (3,) and empty.distance.shape == (0,) and empty.margin.shape == (130,)
    none = scores.consensus(np.zeros((4, 0), dtype=np.uint64), 0, anchor=3)
    assert none.x.shape == (0,) and none.flipped.shape == (4,) and none.changed == 0
    assert _lib.gpu_touched() == touched


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, sampled_components, scores

    for name in ("Consensus", "consensus", "consensus_batch", "vote_weights", "vote_last_ms"):
        assert name in scores.__all__ and getattr(scores, name) is not None
    assert "consensus_chains" in sa.__all__ and callable(sa.consensus_chains) and callable(sa.Chains.consensus)
    assert list(inspect.signature(scores.consensus).parameters) == ["xs", "number_spins", "weights", "ref", "anchor",
                                                                    "align", "rounds"]
    parameters = inspect.signature(scores.consensus).parameters
    assert (parameters["anchor"].default, parameters["align"].default, parameters["rounds"].default) == (0, True, 1)
    parameters = inspect.signature(sa.Chains.consensus).parameters
    assert list(parameters) == ["self", "weights", "which", "anchor", "align", "rounds"]
    assert (parameters["which"].default, parameters["anchor"].default, parameters["align"].default) == ("best", None,
                                                                                                        None)
    assert [f.name for f in __import__("dataclasses").fields(scores.Consensus)][:8] == [
        "x", "ones", "plus", "minus", "margin", "flipped", "distance", "changed"]
    for function in (common.solve_ising_model, common.solve_ising_models):
        assert inspect.signature(function).parameters["select"].default == "best"
    # weights of a vote
    energies = np.array([-3.0, -5.0, -4.0])
    assert np.array_equal(scores.vote_weights(energies), np.ones(3))
    assert np.array_equal(scores.vote_weights(energies, 0.5), np.exp(-0.5 * (energies + 5.0)))
    assert scores.vote_weights(energies, 0.5)[1] == 1.0
    # arguments that do not fit one another
    x = np.zeros((3, 3), dtype=np.uint64)
    with pytest.raises(ValueError):
        scores.consensus(x, 130, weights=np.ones(4))
    with pytest.raises(ValueError):
        scores.consensus(x[:, :2], 130)
    with pytest.raises(ValueError):
        scores.consensus(x, 130, ref=np.zeros(2, dtype=np.uint64))
    with pytest.raises(ValueError):
        scores.consensus(x[0], 130)
    with pytest.raises(ValueError):
        scores.consensus(x, -1)
    with pytest.raises(TypeError):
        sa.consensus_chains([object()])
    # the drivers' keyword: refused before anything is solved
    for arguments in (dict(mode="greedy"), dict(method="population"), dict(method="tempering"), dict(patience=3)):
        with pytest.raises(ValueError, match="consensus"):
            common.solve_ising_models([], select="consensus", **arguments)
    with pytest.raises(ValueError, match="select"):
        common.solve_ising_models([], select="median")
    with pytest.raises(ValueError, match="consensus"):
        common.solve_ising_model(None, mode="greedy", select="consensus")
    assert common.solve_ising_models([], select="consensus") == []


def test_command_line_flag():
    from annealing_sign_problem_amd import sampled_components

    base = ["--model", "heisenberg_kagome_16", "--order", "1", "--output", "x.csv"]
    args = sampled_components.parse_command_line(base)
    assert args.anneal_select == "best" and sampled_components.early_stop_of(args) == {}
    args = sampled_components.parse_command_line(base + ["--anneal-select", "consensus"])
    assert sampled_components.early_stop_of(args) == {"early_stop": {"select": "consensus"}}
    for extra in (["--anneal-patience", "3"], ["--anneal-method", "tempering"], ["--no-annealing"], ["--batch", "1"],
                  ["--anneal-select", "median"]):
        with pytest.raises(SystemExit):
            sampled_components.parse_command_line(base + ["--anneal-select", "consensus"] + extra)
    assert sampled_components.OptimizationResult.csv_header() == \
        "size,greedy_accuracy,greedy_overlap,sa_accuracy,sa_overlap,amplitude_overlap"
