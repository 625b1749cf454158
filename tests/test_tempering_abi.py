"""Parallel tempering on resumable chains (include/asp.h section 4, DESIGN.md §4.10 "Ladder law" and
§4.12, law ASP-PT-1): what can be checked without a device — the symbols, the header against the
bindings, the validation that runs before any device work, and the properties of the law as
tests/tempering_law.py restates it (the checker of tests/test_gpu_tempering.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import tempering_law as law

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_chains_advance_ladder", "asp_sa_chains_exchange")


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_two_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_chains_advance_ladder\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*double\s+const\s*\*\s*chain_betas\s*,"
                     r"\s*uint32_t\s+num_sweeps\s*,\s*uint32_t\s+order\s*,\s*int64_t\s*\*\s*out_trace\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_chains_exchange\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*double\s+const\s*\*\s*chain_betas\s*,"
                     r"\s*uint32_t\s+parity\s*,\s*uint32_t\s+draw\s*,\s*uint32_t\s*\*\s*out_source\s*,"
                     r"\s*double\s*\*\s*out_energy\s*,\s*uint32_t\s*\*\s*out_accepted\s*\)\s*;", header)
    p, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert _lib.SIGNATURES["asp_sa_chains_advance_ladder"] == (ctypes.c_int, [p, p, u32, u32, p])
    assert _lib.SIGNATURES["asp_sa_chains_exchange"] == (ctypes.c_int, [p, p, u32, u32, p, p, p])
    # the law is in the header's comment: the counter word of the draw and the ladder law's "alone"
    assert "0xFFFFFFFC" in header and "ASP-PT-1" in header and "Ladder law" in header


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa

    assert "parallel_tempering" in sa.__all__ and callable(sa.parallel_tempering)
    assert list(inspect.signature(sa.Chains.advance_ladder).parameters) == ["self", "chain_betas", "number_sweeps",
                                                                            "sweep_order", "trace"]
    assert list(inspect.signature(sa.Chains.exchange).parameters) == ["self", "chain_betas", "parity", "draw"]
    assert inspect.signature(sa.Chains.exchange).parameters["draw"].default == 0
    parameters = inspect.signature(sa.parallel_tempering).parameters
    assert list(parameters) == ["hamiltonian", "seed", "number_rounds", "sweeps_per_round", "beta0", "beta1",
                                "repetitions", "only_best", "sweep_order", "exchange"]
    defaults = {k: p.default for k, p in parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(seed=None, number_rounds=512, sweeps_per_round=10, beta0=None, beta1=None, repetitions=64,
                            only_best=True, sweep_order=None, exchange=True)


def test_python_validation_needs_no_device():
    from annealing_sign_problem_amd import annealer as sa

    with pytest.raises(ValueError):
        sa.parallel_tempering(None, sweep_order="random")
    with pytest.raises(ValueError):
        sa.parallel_tempering(None, number_rounds=0)
    with pytest.raises(ValueError):
        sa.parallel_tempering(None, sweeps_per_round=0)
    with pytest.raises(TypeError):
        sa.parallel_tempering("not a Hamiltonian")
    # (the checks of the methods run before the handle is looked at: an object without one will do)
    chains = sa.Chains.__new__(sa.Chains)
    chains._handle, chains.repetitions = None, 3
    for bad in ([1.0, 2.0], [1.0, -1.0, 2.0], [1.0, np.nan, 2.0], [1.0, np.inf, 2.0]):
        with pytest.raises(ValueError, match="chain_betas"):
            chains.advance_ladder(bad, 4, sweep_order="colour")
        with pytest.raises(ValueError, match="chain_betas"):
            chains.exchange(bad, 0)
    with pytest.raises(ValueError, match="sweep_order"):
        chains.advance_ladder([1.0, 2.0, 3.0], 4, sweep_order="random")
    with pytest.raises(ValueError, match="number_sweeps"):
        chains.advance_ladder([1.0, 2.0, 3.0], -1, sweep_order="colour")
    with pytest.raises(ValueError, match="parity"):
        chains.exchange([1.0, 2.0, 3.0], 2)
    with pytest.raises(ValueError, match="draw"):
        chains.exchange([1.0, 2.0, 3.0], 0, draw=2 ** 32)
    with pytest.raises(ValueError, match="closed"):
        chains.exchange([1.0, 2.0, 3.0], 0)


def test_null_handles_are_rejected_before_any_output_is_written():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    betas = np.ones(4)
    trace = np.full((4, 3), 77, dtype=np.int64)
    assert lib.asp_sa_chains_advance_ladder(None, _lib.ptr(betas), ctypes.c_uint32(2), ctypes.c_uint32(0),
                                            _lib.ptr(trace)) == INVALID
    assert "null chains handle" in _lib.last_error()
    source = np.full(4, 77, dtype=np.uint32)
    energy = np.full(4, -77.0)
    accepted = ctypes.c_uint32(12345)
    assert lib.asp_sa_chains_exchange(None, _lib.ptr(betas), ctypes.c_uint32(0), ctypes.c_uint32(0), _lib.ptr(source),
                                      _lib.ptr(energy), ctypes.byref(accepted)) == INVALID
    assert "null chains handle" in _lib.last_error()
    assert np.all(trace == 77) and np.all(source == 77) and np.all(energy == -77.0) and accepted.value == 12345


# ---- the restated law ------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2, 3, 4, 7, 64, 257])
def test_the_map_is_an_involution_of_adjacent_transpositions_of_the_right_parity(R):
    rng = np.random.default_rng(R)
    for parity in (0, 1):
        ks = law.pairs(R, parity)
        assert all(k % 2 == parity and k + 1 < R for k in ks)
        assert ks == [k for k in range(R) if k % 2 == parity and k + 1 < R]
        for trial in range(4):
            energies = rng.normal(size=R)
            betas = np.sort(rng.random(R)) * 8.0
            source, accepted = law.exchange(energies, betas, parity, 11, trial, 0)
            assert source.dtype == np.uint32 and source.shape == (R,)
            assert sorted(source) == list(range(R))  # a permutation ...
            assert all(source[source[j]] == j for j in range(R))  # ... that is its own inverse
            moved = [j for j in range(R) if source[j] != j]
            assert len(moved) == 2 * accepted
            for j in moved:  # disjoint adjacent transpositions that start at a k of the parity
                k = min(j, int(source[j]))
                assert abs(int(source[j]) - j) == 1 and k in ks


def test_r1_and_r2_with_parity_1_give_the_identity():
    assert law.pairs(1, 0) == [] and law.pairs(1, 1) == [] and law.pairs(2, 1) == [] and law.pairs(2, 0) == [0]
    for R, parity in ((1, 0), (1, 1), (2, 1)):
        source, accepted = law.exchange([3.0, -1.0][:R], [0.5, 0.1][:R], parity, 5, 0, 0)
        assert list(source) == list(range(R)) and accepted == 0


def test_equal_betas_or_equal_energies_always_swap():
    rng = np.random.default_rng(3)
    R = 9
    for parity in (0, 1):
        every = len(law.pairs(R, parity))
        for draw in range(3):
            source, accepted = law.exchange(rng.normal(size=R), np.full(R, 0.7), parity, 1, 0, draw)
            assert accepted == every  # x = 0
            source, accepted = law.exchange(np.full(R, -2.5), np.sort(rng.random(R)), parity, 1, 0, draw)
            assert accepted == every
        # ... whatever the word: the largest one, u closest to 1
        words = {k: 2 ** 32 - 1 for k in law.pairs(R, parity)}
        assert law.select(list(rng.normal(size=R)), [0.7] * R, parity, words)[1] == every
    assert law.cost(0.7, 0.7, 1.0, 2.0) == 0.0 and law.accepts(2 ** 32 - 1, 0.0)


def test_detailed_balance_of_the_two_directions():
    """For a pair of slots at (beta, beta + dbeta) the configurations with energies (E, E + dE) and the
    swapped ones (E + dE, E) have costs x and -x: one direction's threshold is 1, the other's
    expneg(|x|), so the ratio of the two swap probabilities is the ratio of the Boltzmann weights."""
    import oracle

    for dbeta in (0.0, 1e-3, 0.25, 1.0, 7.5, 40.0):
        for de in (0.0, 1e-6, 0.1, 1.0, 3.0, 22.0, 23.0, 1e3):
            forward = law.cost(0.5, 0.5 + dbeta, 2.0, 2.0 + de)   # the colder slot holds the higher energy
            backward = law.cost(0.5, 0.5 + dbeta, 2.0 + de, 2.0)
            assert forward == -backward and forward <= 0.0
            assert law.threshold(forward) == 1.0
            magnitude = abs(backward)
            assert law.threshold(backward) == (1.0 if magnitude == 0.0 else
                                               (oracle.expneg(magnitude) if magnitude < 23.0 else 0.0))
            # a colder slot with the higher energy always swaps, whatever the word
            assert law.accepts(2 ** 32 - 1, forward)
            if magnitude >= 23.0:
                assert not law.accepts(0, backward)
    # the word decides against the threshold: u = (v + 0.5) 2^-32 < expneg(x)
    p = oracle.expneg(1.0)
    edge = int(p * 2.0 ** 32)
    assert law.accepts(edge - 1, 1.0) and not law.accepts(edge + 1, 1.0)
    assert not law.accepts(0, float("nan"))


def test_the_draw_has_its_own_counter_word_and_every_argument_matters():
    import population_law

    words = {law.draw_word(5, 0, 0, 0), law.draw_word(5, 2, 0, 0), law.draw_word(5, 0, 16, 0), law.draw_word(5, 0, 0, 7),
             law.draw_word(6, 0, 0, 0), law.draw_word(5 + 2 ** 32, 0, 0, 0)}
    assert len(words) == 6
    assert law.DRAW_WORD >= 2 ** 30 and law.DRAW_WORD not in (0xFFFFFFFE, 0xFFFFFFFF, population_law.DRAW_WORD)
