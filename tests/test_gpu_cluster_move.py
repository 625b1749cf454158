"""GPU: isoenergetic cluster moves on resumable chains (asp_sa_chains_cluster_move, DESIGN.md §4.13, law
ASP-ICM-1) against the law as tests/cluster_move_law.py restates it — all five state arrays through
Chains.state() and the three outputs, exact — on the shapes where the kernel can go wrong: the tail
word, a path (one site per search round), a hub (a row the wavefront shares), a component that must
not cross an equal site, isolated seeds, identical and opposite replicas, many pairs in one launch, the
bit planes in LDS and in HBM; then the driver against the closed calls.

What comes out when sweeps, exchange and cluster moves are composed is tested in
tests/test_gpu_ensemble_law.py against the exact joint law of tests/ensemble_exact_law.py, which is
independent of the restated law used here."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse

import cluster_move_law as law

pytestmark = pytest.mark.gpu

INVALID = -3
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parallel_tempering_planted500.npz")


def _same_state(a, b):
    for name in STATE:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name])), name
    assert int(a["sweeps_done"]) == int(b["sweeps_done"])


def _random_problem(K, seed, degree=4):
    """Asymmetric J with a diagonal, a field."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, K, size=degree * K)
    cols = rng.integers(0, K, size=degree * K)
    J = scipy.sparse.coo_matrix((rng.normal(size=degree * K), (rows, cols)), shape=(K, K)).tocsr()
    return J, rng.normal(size=K) * 0.3


def _random_x0(K, seed, rows):
    rng = np.random.default_rng(seed)
    return np.stack([law.pack(rng.random(K) < 0.5) for _ in range(rows)])


def _move(J, h, ham, chains, pairs, draw=0):
    """One device move checked against the law: (state before, state after, outputs)."""
    before = chains.state()
    expected, differing, sizes, deltas = law.move(J, h, ham.info().energy_scale_exp, before, chains.seed, pairs, draw)
    got = chains.cluster_move(pairs, draw)
    after = chains.state()
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.int64
    assert np.array_equal(got[0], differing) and np.array_equal(got[1], sizes) and np.array_equal(got[2], deltas)
    _same_state(after, expected)
    return before, after, got


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_tail_word_two_draws_two_sweep_counts_and_the_move_twice(K):
    from annealing_sign_problem_amd import annealer as sa

    J, h = _random_problem(K, K)
    ham = sa.Hamiltonian(J, h)
    R = 5
    pairs = [(3, 0), (1, 4)]
    with sa.Chains(ham, seed=17, repetitions=R, x0=_random_x0(K, K + 1, R)) as chains:
        for sweeps in (0, 3):
            if sweeps:
                chains.advance(np.full(sweeps, 0.4), sweep_order="colour")
            for draw in (0, 7):
                before, after, got = _move(J, h, ham, chains, pairs, draw)
                # slot 2 is in no pair: untouched in all five arrays
                for name in STATE:
                    assert np.array_equal(before[name][2], after[name][2]), name
                # the tracked sum of a pair is conserved exactly, the energies to the project's 1e-12
                for a, b in pairs:
                    assert (after["tracked_current"][a] + after["tracked_current"][b]
                            == before["tracked_current"][a] + before["tracked_current"][b])
                    e0 = ham.energies(before["x_current"][[a, b]])
                    e1 = ham.energies(after["x_current"][[a, b]])
                    scale = max(1.0, float(abs(J).sum() + np.abs(h).sum()))
                    assert abs(e1.sum() - e0.sum()) <= 1e-12 * scale
                # the same call again restores x_current and tracked_current bit for bit
                _, again, got2 = _move(J, h, ham, chains, pairs, draw)
                assert np.array_equal(again["x_current"], before["x_current"])
                assert np.array_equal(again["tracked_current"], before["tracked_current"])
                assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])
                assert np.array_equal(got2[2], -got[2])
                chains.cluster_move(pairs, draw)  # (and on from the moved state)
        # the host mirror follows tracked_current: entry 0 of the next trace
        trace = chains.advance(np.full(2, 0.4), sweep_order="colour", trace=True)
        assert np.array_equal(trace[:, 0], after["tracked_current"])


def _opposite_pair(ham, J, h, K, seed=3, **kw):
    """Two chains, b = ~a; one move against the law."""
    from annealing_sign_problem_amd import annealer as sa

    up = np.random.default_rng(seed).random(K) < 0.5
    x0 = np.stack([law.pack(up), law.pack(~up)])
    with sa.Chains(ham, seed=seed, repetitions=2, x0=x0) as chains:
        return _move(J, h, ham, chains, [(0, 1)], **kw)


def test_a_path_of_300_sites_that_all_differ():
    """300 search rounds with a frontier one site wide (two, from a seed in the middle)."""
    from annealing_sign_problem_amd import annealer as sa

    K = 300
    rng = np.random.default_rng(1)
    J = scipy.sparse.diags(rng.normal(size=K - 1), 1, shape=(K, K), format="csr")
    h = rng.normal(size=K) * 0.2
    _, _, got = _opposite_pair(sa.Hamiltonian(J, h), J, h, K)
    assert got[0][0] == K and got[1][0] == K


def test_a_star_whose_hub_has_degree_300():
    from annealing_sign_problem_amd import annealer as sa

    K = 301
    rng = np.random.default_rng(2)
    J = scipy.sparse.coo_matrix((rng.normal(size=K - 1), (np.full(K - 1, 17), np.delete(np.arange(K), 17))),
                                shape=(K, K)).tocsr()
    h = rng.normal(size=K) * 0.2
    ham = sa.Hamiltonian(J, h)
    _, _, got = _opposite_pair(ham, J, h, K)
    assert got[0][0] == K and got[1][0] == K
    # half of the leaves equal: the hub's row sum runs over them, the component over the others
    up = rng.random(K) < 0.5
    other = ~up
    other[18:160] = up[18:160]
    with sa.Chains(ham, seed=4, repetitions=2, x0=np.stack([law.pack(up), law.pack(other)])) as chains:
        for draw in range(3):
            _move(J, h, ham, chains, [(1, 0)], draw)


def test_the_search_does_not_cross_an_equal_site():
    """Two dense blobs joined only through site 40, on which the replicas agree."""
    from annealing_sign_problem_amd import annealer as sa

    K = 81
    rng = np.random.default_rng(5)
    dense = np.zeros((K, K))
    dense[:40, :40] = np.triu(rng.normal(size=(40, 40)), 1)
    dense[41:, 41:] = np.triu(rng.normal(size=(40, 40)), 1)
    dense[40, 3], dense[40, 60], dense[7, 40] = 0.9, -0.7, 0.4
    J = scipy.sparse.csr_matrix(dense)
    h = rng.normal(size=K) * 0.2
    ham = sa.Hamiltonian(J, h)
    up = rng.random(K) < 0.5
    other = ~up
    other[40] = up[40]
    with sa.Chains(ham, seed=6, repetitions=2, x0=np.stack([law.pack(up), law.pack(other)])) as chains:
        sizes = set()
        for draw in range(6):
            before, after, got = _move(J, h, ham, chains, [(0, 1)], draw)
            assert got[0][0] == 80 and got[1][0] == 40
            flipped = law.bits(before["x_current"][0], K) ^ law.bits(after["x_current"][0], K)
            sizes.add(bool(flipped[0]))
            assert flipped[:40].all() != flipped[41:].all() and not flipped[40]
        assert sizes == {True, False}  # (a condition on the draws: both blobs were the seed's)


def test_isolated_seeds_identical_replicas_and_the_best_configuration():
    from annealing_sign_problem_amd import annealer as sa

    K = 70
    J, h = _random_problem(K, 8)
    J = scipy.sparse.lil_matrix(J)
    for i in (5, 64, 69):  # isolated spins (a diagonal entry is no coupling)
        J[i, :] = 0.0
        J[:, i] = 0.0
    J[5, 5] = 0.75
    J = scipy.sparse.csr_matrix(J)
    J.eliminate_zeros()
    ham = sa.Hamiltonian(J, h)
    S = ham.info().energy_scale_exp
    up = np.random.default_rng(9).random(K) < 0.5
    other = up.copy()
    other[[5, 64, 69]] ^= True
    x0 = np.stack([law.pack(up), law.pack(other), law.pack(up), law.pack(up)])
    with sa.Chains(ham, seed=10, repetitions=4, x0=x0) as chains:
        start = chains.state()
        seen = set()
        for draw in range(8):
            chains.load_state(start)
            before, after, got = _move(J, h, ham, chains, [(0, 1), (3, 2)], draw)
            # pair 0: |C| = 1 and Q from the field alone; pair 1: identical replicas, nothing changes
            assert got[0][0] == 3 and got[1][0] == 1
            i = int(np.flatnonzero(law.bits(before["x_current"][0], K) ^ law.bits(after["x_current"][0], K))[0])
            seen.add(i)
            assert got[2][0] == int(np.rint((-2.0 if up[i] else 2.0) * h[i] * 2.0 ** S))
            assert got[0][1] == 0 and got[1][1] == 0 and got[2][1] == 0
            for name in STATE:
                assert np.array_equal(before[name][2:], after[name][2:]), name
            # the chain whose energy fell has a new best configuration, the other keeps the start
            Q = int(got[2][0])
            if Q != 0:
                low, high = (0, 1) if Q < 0 else (1, 0)
                assert after["tracked_best"][low] == -abs(Q) and np.array_equal(after["x_best"][low], after["x_current"][low])
                assert after["tracked_best"][high] == 0 and np.array_equal(after["x_best"][high], start["x_best"][high])
                # a tie with the best energy replaces nothing
                tied = {name: np.array(value, copy=True) for name, value in start.items()}
                tied["tracked_best"][low] = -abs(Q)
                tied["x_best"][low] = law.pack(np.zeros(K, dtype=bool))
                chains.load_state(tied)
                _, after_tie, _ = _move(J, h, ham, chains, [(0, 1), (3, 2)], draw)
                assert after_tie["tracked_current"][low] == -abs(Q) == after_tie["tracked_best"][low]
                assert np.array_equal(after_tie["x_best"][low], tied["x_best"][low])
        assert len(seen) >= 2  # (a condition on the draws)


def test_257_chains_with_128_pairs_in_one_launch():
    from annealing_sign_problem_amd import annealer as sa

    K, R = 70, 257
    J, h = _random_problem(K, 12)
    ham = sa.Hamiltonian(J, h)
    order = np.random.default_rng(13).permutation(R)
    pairs = order[:256].reshape(128, 2)
    with sa.Chains(ham, seed=14, repetitions=R) as chains:
        chains.advance(np.full(2, 0.3), sweep_order="shuffled")
        before, after, got = _move(J, h, ham, chains, pairs)
        assert np.count_nonzero(got[1]) > 100
        left = int(order[256])
        for name in STATE:
            assert np.array_equal(before[name][left], after[name][left]), name


def test_a_planted_cluster_after_cold_sweeps():
    """planted_cluster(3000), 20 cold sweeps from random starts: a realistic set of differing sites."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(3000, seed=5)
    h = np.random.default_rng(5).normal(size=3000) * 0.01
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    with sa.Chains(ham, seed=15, repetitions=4) as chains:
        chains.advance(np.full(20, info.beta1_auto))
        before, after, got = _move(J, h, ham, chains, [(0, 1), (3, 2)])
        assert np.all(got[0] > 0) and np.all(got[1] > 0)
        e0 = ham.energies(before["x_current"])
        e1 = ham.energies(after["x_current"])
        for a, b in ((0, 1), (3, 2)):
            assert abs((e1[a] + e1[b]) - (e0[a] + e0[b])) <= 1e-12 * max(1.0, abs(e0[a]) + abs(e0[b]))


def test_20000_spins_with_the_planes_in_hbm_and_in_lds():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    K = 20000
    J, h = _random_problem(K, 16, degree=2)
    ham = sa.Hamiltonian(J, h)
    lib = _lib.load()
    pairs = [(1, 2), (3, 0)]
    with sa.Chains(ham, seed=18, repetitions=4, x0=_random_x0(K, 17, 4)) as chains:
        start = chains.state()
        expected, differing, sizes, deltas = law.move(J, h, ham.info().energy_scale_exp, start, chains.seed, pairs, 0)
        assert np.all(sizes > 1000)  # (a condition on the inputs: large components)
        for where in (2, 1, 0):
            chains.load_state(start)
            _lib.check(lib.asp_sa_chains_set_cluster_planes(chains._live(), ctypes.c_int(where)))
            got = chains.cluster_move(pairs)
            assert lib.asp_sa_chains_cluster_move_last_ms() > 0.0
            assert np.array_equal(got[0], differing) and np.array_equal(got[1], sizes) and np.array_equal(got[2], deltas)
            _same_state(chains.state(), expected)


def test_invalid_arguments_return_before_any_launch():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    K, R = 65, 4
    J, h = _random_problem(K, 19)
    ham = sa.Hamiltonian(J, h)
    u32 = ctypes.c_uint32
    with sa.Chains(ham, seed=1, repetitions=R) as chains:
        before = chains.state()
        handle = chains._live()
        differing = np.full(2, 77, dtype=np.uint32)
        sizes = np.full(2, 77, dtype=np.uint32)
        deltas = np.full(2, -77, dtype=np.int64)

        def move(pairs, count):
            pairs = None if pairs is None else np.array(pairs, dtype=np.uint32)
            return lib.asp_sa_chains_cluster_move(handle, _lib.ptr(pairs), u32(count), u32(0), _lib.ptr(differing),
                                                  _lib.ptr(sizes), _lib.ptr(deltas))

        assert move(None, 2) == INVALID and "null pairs" in _lib.last_error()
        assert move([0, 1, 2, 4], 2) == INVALID and "pairs[3]" in _lib.last_error()
        assert move([0, 1, 2, 0], 2) == INVALID
        assert "pairs[0]" in _lib.last_error() and "pairs[3]" in _lib.last_error()
        assert move([1, 1], 1) == INVALID and "pairs[0]" in _lib.last_error() and "pairs[1]" in _lib.last_error()
        assert np.all(differing == 77) and np.all(sizes == 77) and np.all(deltas == -77)
        _same_state(chains.state(), before)
        # no pairs: nothing runs; NULL outputs are allowed: the move still runs
        assert move(None, 0) == 0 and move([0, 1], 0) == 0
        _same_state(chains.state(), before)
        expected = law.move(J, h, ham.info().energy_scale_exp, before, 1, [(2, 1)], 0)[0]
        pairs = np.array([2, 1], dtype=np.uint32)
        assert lib.asp_sa_chains_cluster_move(handle, _lib.ptr(pairs), u32(1), u32(0), None, None, None) == 0
        _same_state(chains.state(), expected)
        got = chains.cluster_move(np.zeros((0, 2), dtype=np.int64))
        assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].shape == (0,)


# ---- the drivers ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_parallel_tempering_cluster_is_the_loop_over_the_closed_calls(order):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    rounds, per, R, seed = 5, 4, 8, 5
    J, _, _ = synthetic.planted_cluster(300, seed=70)
    h = np.random.default_rng(70).normal(size=300) * 0.01
    make = lambda: sa.Hamiltonian(J, h)
    info = make().info()
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, R // 2)
    hairpin = np.concatenate([ladder, ladder[::-1]])
    kw = dict(seed=seed, number_rounds=rounds, sweeps_per_round=per, repetitions=R, sweep_order=order)
    for rungs in (None, 2):
        xs, es = sa.parallel_tempering_cluster(make(), only_best=False, cluster_rungs=rungs, **kw)
        count = R // 2 if rungs is None else rungs
        pairs = [(k, R - 1 - k) for k in range(R // 2 - count, R // 2)]
        flipped = 0
        with sa.Chains(make(), seed=seed, repetitions=R) as chains:
            for j in range(rounds):
                chains.advance_ladder(hairpin, per, sweep_order=order)
                flipped += int(chains.cluster_move(pairs, 0)[1].sum())
                if j + 1 < rounds:
                    chains.exchange(hairpin, j & 1, 0)
            hxs, hes = chains.result()
        assert flipped > 0  # (a condition on the inputs: the moves did something)
        assert np.array_equal(xs, hxs) and es.tobytes() == hes.tobytes()
    ham = make()
    assert es.tobytes() == ham.energies(xs).tobytes()
    x, e = sa.parallel_tempering_cluster(make(), cluster_rungs=2, **kw)
    best = int(np.argmin(es))
    assert np.array_equal(x, xs[best]) and np.float64(e).tobytes() == es[best].tobytes()


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_parallel_tempering_without_cluster_moves_is_the_recorded_result(order):
    """The plain driver on planted_cluster(500) against what it returned before cluster moves existed
    (tests/golden/parallel_tempering_planted500.npz)."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(500, seed=21)
    h = np.random.default_rng(21).normal(size=500) * 0.01
    xs, es = sa.parallel_tempering(sa.Hamiltonian(J, h), seed=3, number_rounds=6, sweeps_per_round=5, repetitions=8,
                                   only_best=False, sweep_order=order)
    recorded = np.load(GOLDEN, allow_pickle=False)
    assert np.array_equal(xs, recorded["xs_" + order]) and es.tobytes() == recorded["es_" + order].tobytes()
