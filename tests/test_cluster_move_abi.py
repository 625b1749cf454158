"""Isoenergetic cluster moves on resumable chains (include/asp.h section 4, DESIGN.md §4.13, law
ASP-ICM-1): what can be checked without a device — the symbols, the header against the bindings, the
validation that runs before any device work, and the properties of the law as tests/cluster_move_law.py
restates it (the checker of tests/test_gpu_cluster_move.py), among them its exact stationarity."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse

import cluster_move_law as law

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_chains_cluster_move", "asp_sa_chains_cluster_move_last_ms", "asp_sa_chains_set_cluster_planes")


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_three_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_chains_cluster_move\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*uint32_t\s+const\s*\*\s*pairs\s*,"
                     r"\s*uint32_t\s+num_pairs\s*,\s*uint32_t\s+draw\s*,\s*uint32_t\s*\*\s*out_differing\s*,"
                     r"\s*uint32_t\s*\*\s*out_size\s*,\s*int64_t\s*\*\s*out_delta\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_chains_cluster_move_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_chains_set_cluster_planes\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*int\s+where\s*\)\s*;", header)
    p, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert _lib.SIGNATURES["asp_sa_chains_cluster_move"] == (ctypes.c_int, [p, p, u32, u32, p, p, p])
    assert _lib.SIGNATURES["asp_sa_chains_cluster_move_last_ms"] == (ctypes.c_float, [])
    assert _lib.SIGNATURES["asp_sa_chains_set_cluster_planes"] == (ctypes.c_int, [p, ctypes.c_int])
    # the law is in the header's comment: its name and the counter word of the draw
    assert "0xFFFFFFFB" in header and "ASP-ICM-1" in header


def test_python_surface():
    from annealing_sign_problem_amd import annealer as sa

    assert list(inspect.signature(sa.Chains.cluster_move).parameters) == ["self", "pairs", "draw"]
    assert inspect.signature(sa.Chains.cluster_move).parameters["draw"].default == 0
    assert "parallel_tempering_cluster" in sa.__all__ and callable(sa.parallel_tempering_cluster)
    parameters = inspect.signature(sa.parallel_tempering_cluster).parameters
    plain = inspect.signature(sa.parallel_tempering).parameters
    # the plain driver's parameters with their defaults, then the one this driver adds
    assert list(parameters) == list(plain) + ["cluster_rungs"]
    for name in plain:
        assert parameters[name].default == plain[name].default, name
    assert parameters["cluster_rungs"].default is None


def test_python_validation_needs_no_device():
    from annealing_sign_problem_amd import annealer as sa

    with pytest.raises(ValueError):
        sa.parallel_tempering_cluster(None, sweep_order="random")
    with pytest.raises(ValueError):
        sa.parallel_tempering_cluster(None, number_rounds=0)
    with pytest.raises(TypeError):
        sa.parallel_tempering_cluster("not a Hamiltonian")
    ham = sa.Hamiltonian(scipy.sparse.identity(4, format="csr"), np.zeros(4))
    with pytest.raises(ValueError, match="even"):
        sa.parallel_tempering_cluster(ham, repetitions=7)
    with pytest.raises(ValueError, match="cluster_rungs"):
        sa.parallel_tempering_cluster(ham, repetitions=8, beta0=1.0, beta1=2.0, cluster_rungs=5)
    # (the checks of the method run before the handle is looked at: an object without one will do)
    chains = sa.Chains.__new__(sa.Chains)
    chains._handle, chains.repetitions = None, 5
    for bad in ([0, 1], [[0, 1, 2]], [[0.0, 1.0]], [[0, 5]], [[-1, 2]], [[0, 1], [2, 0]], [[3, 3]]):
        with pytest.raises(ValueError, match="pairs"):
            chains.cluster_move(bad)
    with pytest.raises(ValueError, match="draw"):
        chains.cluster_move([[0, 1]], draw=2 ** 32)
    with pytest.raises(ValueError, match="closed"):
        chains.cluster_move([[3, 0], [1, 4]])
    with pytest.raises(ValueError, match="closed"):
        chains.cluster_move([])


def test_a_null_handle_is_rejected_before_any_output_is_written():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.load().asp_device_touched()
    pairs = np.array([0, 1], dtype=np.uint32)
    differing = np.full(1, 77, dtype=np.uint32)
    sizes = np.full(1, 77, dtype=np.uint32)
    deltas = np.full(1, -77, dtype=np.int64)
    assert lib.asp_sa_chains_cluster_move(None, _lib.ptr(pairs), ctypes.c_uint32(1), ctypes.c_uint32(0),
                                          _lib.ptr(differing), _lib.ptr(sizes), _lib.ptr(deltas)) == INVALID
    assert "null chains handle" in _lib.last_error()
    assert lib.asp_sa_chains_set_cluster_planes(None, ctypes.c_int(2)) == INVALID
    assert "null chains handle" in _lib.last_error()
    assert differing[0] == 77 and sizes[0] == 77 and deltas[0] == -77
    assert lib.asp_sa_chains_cluster_move_last_ms() == 0.0
    assert _lib.load().asp_device_touched() == touched  # no device work


# ---- the restated law ------------------------------------------------------------------------------

def _frustrated():
    """Five spins: a frustrated triangle 0-1-2 with a tail 2-3-4 and a chord 1-3, asymmetric J with a
    diagonal, a field."""
    J = np.zeros((5, 5))
    J[0, 1], J[1, 0] = 0.7, 0.2
    J[1, 2] = 1.1
    J[2, 0], J[0, 2] = 0.4, 0.5
    J[2, 3] = -0.8
    J[3, 4], J[4, 3] = 0.3, 0.35
    J[3, 1] = -0.6
    J[1, 1], J[4, 4] = 0.25, -1.5
    h = np.array([0.3, -0.2, 0.15, 0.45, -0.1])
    return scipy.sparse.csr_matrix(J), h


def _state(xs, sweeps_done=0, tracked=None):
    xs = np.asarray(xs, dtype=np.uint64).reshape(len(xs), -1)
    R = xs.shape[0]
    tracked = np.zeros(R, dtype=np.int64) if tracked is None else np.asarray(tracked, dtype=np.int64)
    return dict(x_current=xs.copy(), x_best=xs.copy(), tracked_current=tracked.copy(), tracked_best=tracked.copy(),
                accepted=np.zeros(R, dtype=np.uint64), sweeps_done=np.uint32(sweeps_done))


def _random_problem(K, rng, degree=4):
    rows = rng.integers(0, K, size=degree * K)
    cols = rng.integers(0, K, size=degree * K)
    J = scipy.sparse.coo_matrix((rng.normal(size=degree * K), (rows, cols)), shape=(K, K)).tocsr()
    return J, rng.normal(size=K) * 0.3


@pytest.mark.parametrize("K", [1, 5, 63, 64, 65, 130])
def test_involution_conservation_and_the_difference_stays(K):
    rng = np.random.default_rng(K)
    J, h = _random_problem(K, rng)
    S = 30
    R = 6
    xs = np.stack([law.pack(rng.random(K) < 0.5) for _ in range(R)])
    xs[5] = xs[4]  # identical replicas
    state = _state(xs, sweeps_done=7, tracked=rng.integers(-1000, 1000, size=R))
    pairs = [(3, 0), (1, 2), (5, 4)]
    for draw in (0, 9):
        new, differing, sizes, deltas = law.move(J, h, S, state, 11, pairs, draw)
        for p, (a, b) in enumerate(pairs):
            d_before = law.bits(state["x_current"][a], K) ^ law.bits(state["x_current"][b], K)
            d_after = law.bits(new["x_current"][a], K) ^ law.bits(new["x_current"][b], K)
            assert np.array_equal(d_before, d_after) and differing[p] == d_before.sum()
            flipped = law.bits(state["x_current"][a], K) ^ law.bits(new["x_current"][a], K)
            assert flipped.sum() == sizes[p] and not np.any(flipped & ~d_before)
            assert (sizes[p] == 0) == (differing[p] == 0)
            # the tracked sum is conserved exactly, the energies to rounding
            assert (new["tracked_current"][a] + new["tracked_current"][b]
                    == state["tracked_current"][a] + state["tracked_current"][b])
            assert new["tracked_current"][a] - state["tracked_current"][a] == deltas[p]
            before = [law.energy(J, h, law.bits(state["x_current"][r], K)) for r in (a, b)]
            after = [law.energy(J, h, law.bits(new["x_current"][r], K)) for r in (a, b)]
            scale = max(1.0, abs(J).sum() + abs(h).sum())
            assert abs(sum(after) - sum(before)) <= 1e-12 * scale
            # E(a') - E(a) = Q 2^-S up to |C| roundings of 2^-S (and the rounding of the energies)
            assert abs((after[0] - before[0]) - float(deltas[p]) * 2.0 ** -S) <= sizes[p] * 2.0 ** -S + 1e-12 * scale
        assert differing[2] == 0 and deltas[2] == 0
        # the same call again restores x_current and tracked_current bit for bit
        again, differing2, sizes2, deltas2 = law.move(J, h, S, new, 11, pairs, draw)
        assert np.array_equal(again["x_current"], state["x_current"])
        assert np.array_equal(again["tracked_current"], state["tracked_current"])
        assert np.array_equal(differing2, differing) and np.array_equal(sizes2, sizes)
        assert np.array_equal(deltas2, -deltas)
        for name in ("accepted", "sweeps_done"):
            assert np.array_equal(new[name], state[name])


def test_best_follows_a_strict_improvement_only():
    J, h = _frustrated()
    K, S = 5, 30
    xs = np.stack([law.pack([1, 1, 0, 1, 0]), law.pack([1, 0, 1, 1, 0])])
    first, _, _, deltas = law.move(J, h, S, _state(xs), 1, [(0, 1)], 0)
    Q = int(deltas[0])
    assert Q != 0
    low, high = (0, 1) if Q < 0 else (1, 0)
    assert first["tracked_best"][low] == -abs(Q) and first["tracked_best"][high] == 0
    assert np.array_equal(first["x_best"][low], first["x_current"][low])
    assert np.array_equal(first["x_best"][high], xs[high])
    # a tie with the best energy replaces nothing
    tied = _state(xs)
    tied["tracked_best"][low] = -abs(Q)
    tied["x_best"][low] = law.pack([0, 0, 0, 0, 0])
    second, _, _, _ = law.move(J, h, S, tied, 1, [(0, 1)], 0)
    assert second["tracked_current"][low] == -abs(Q) == second["tracked_best"][low]
    assert np.array_equal(second["x_best"][low], law.pack([0, 0, 0, 0, 0]))


def test_the_seed_is_uniform_over_the_differing_sites():
    for n in (1, 2, 3, 5, 64, 1000, 2 ** 31 + 5):
        assert law.seed_index(0, n) == 0 and law.seed_index(2 ** 32 - 1, n) == n - 1
        for U in {0, 1, n // 2, n - 1}:
            if U < n:
                v = -((-U * 2 ** 32) // n)  # the smallest word that gives U
                assert law.seed_index(v, n) == U and (v == 0 or law.seed_index(v - 1, n) == U - 1)


def test_the_draw_has_its_own_counter_word_and_every_argument_matters():
    import population_law
    import tempering_law

    words = {law.draw_word(5, 0, 0, 0), law.draw_word(5, 2, 0, 0), law.draw_word(5, 0, 16, 0), law.draw_word(5, 0, 0, 7),
             law.draw_word(6, 0, 0, 0), law.draw_word(5 + 2 ** 32, 0, 0, 0)}
    assert len(words) == 6
    assert law.DRAW_WORD >= 2 ** 30
    assert law.DRAW_WORD not in (0xFFFFFFFE, 0xFFFFFFFF, population_law.DRAW_WORD, tempering_law.DRAW_WORD)


def test_exact_stationarity_of_the_product_boltzmann_distribution():
    """All 4^5 joint states of two replicas of the frustrated five-spin model: the mixture of the move
    over the n equally likely seeds (one word for every U) maps the product Boltzmann distribution at
    one beta onto itself."""
    J, h = _frustrated()
    K, S, beta = 5, 40, 0.9
    A = law.couplings(J)
    configurations = [np.array(c, dtype=bool) for c in itertools.product([False, True], repeat=K)]
    packed = [law.pack(c) for c in configurations]
    index = {int(x[0]): k for k, x in enumerate(packed)}
    energies = np.array([law.energy(J, h, c) for c in configurations])
    weights = np.exp(-beta * (energies - energies.min()))
    weights /= weights.sum()
    joint = np.outer(weights, weights)
    image = np.zeros_like(joint)
    moved = 0
    for ka, kb in itertools.product(range(len(packed)), repeat=2):
        n = int((configurations[ka] ^ configurations[kb]).sum())
        if n == 0:
            image[ka, kb] += joint[ka, kb]
            continue
        for U in range(n):
            v = -((-U * 2 ** 32) // n)
            assert law.seed_index(v, n) == U
            xa, xb, n_out, size, Q = law.pair_move(A, h, S, K, packed[ka], packed[kb], v)
            assert n_out == n and 1 <= size <= n
            image[index[int(xa[0])], index[int(xb[0])]] += joint[ka, kb] / n
            moved += 1
    assert moved == sum(n * 2 ** K * len(list(itertools.combinations(range(K), n))) for n in range(1, K + 1))
    assert np.max(np.abs(image - joint)) <= 1e-12
    assert abs(image.sum() - 1.0) <= 1e-12
