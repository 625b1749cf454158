"""Scores and distances of the configurations RESIDENT in a chains handle (asp_sa_chains_scores /
_distances, annealer.Chains.scores / .distances, anneal_until(target=...); specification ASP-SCORE-1,
DESIGN.md §3.11) on a planted cluster of 300 spins with 64 chains: equal, bit for bit, to the scores of
the exported configurations — after advance, resample, exchange and load_state —, the handle untouched by
them, and the early stop on the accuracy."""
import ctypes

import numpy as np
import pytest

import score_cases

pytestmark = pytest.mark.gpu

SPINS, CHAINS = 300, 64


@pytest.fixture(scope="module")
def problem():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, h, planted = synthetic.planted_cluster(SPINS, seed=23)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    rng = np.random.default_rng(4)
    weights = np.exp(rng.normal(0.0, 3.0, size=SPINS)) ** 2
    subset = np.sort(rng.choice(SPINS, size=170, replace=False)).astype(np.int32)
    return {"ham": ham, "exact": sa.signs_to_bits(planted), "planted": planted, "weights": weights, "subset": subset,
            "betas": sa.make_schedule(info.beta0_auto, info.beta1_auto, 40)}


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(score_cases.bits_of(got[1]), score_cases.bits_of(want[1]))
    assert score_cases.bits_of(got[2]) == score_cases.bits_of(want[2])


def _check_against_exports(chains, p):
    """Chains.scores / .distances of both configuration sets against sign_scores / sign_distances of what
    the handle exports, with and without weights and through the sorted subset."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import scores

    best, _ = chains.result(only_best=False)
    current = chains.state()["x_current"]
    assert np.array_equal(best, chains.state()["x_best"])
    subset_exact = sa.signs_to_bits(p["planted"][p["subset"]])
    for which, xs in (("best", best), ("current", current)):
        _same(chains.scores(p["exact"], p["weights"], which=which),
              scores.sign_scores(xs, p["exact"], p["weights"], number_spins=SPINS))
        _same(chains.scores(p["exact"], which=which), scores.sign_scores(xs, p["exact"], number_spins=SPINS))
        _same(chains.scores(subset_exact, p["weights"][p["subset"]], select=p["subset"], which=which),
              scores.sign_scores(xs, subset_exact, p["weights"][p["subset"]], select=p["subset"], number_spins=SPINS))
        distances = chains.distances(which=which)
        assert np.array_equal(distances, scores.sign_distances(xs, SPINS))
        assert np.array_equal(distances, score_cases.distances_law(xs, SPINS))
    # ... and the law itself, so that it is not the kernel against itself
    case = {"spins": SPINS, "scored": SPINS, "xs": best, "exact": p["exact"], "weights": p["weights"], "select": None}
    _same(chains.scores(p["exact"], p["weights"]), score_cases.scores_law(case))


def test_scores_of_resident_chains_after_every_kind_of_step(problem):
    from annealing_sign_problem_amd import annealer as sa

    p = problem
    with sa.Chains(p["ham"], seed=11, repetitions=CHAINS) as chains:
        _check_against_exports(chains, p)  # the starts
        chains.advance(p["betas"][:20], sweep_order="shuffled")
        _check_against_exports(chains, p)
        chains.resample(0.3)  # (the handle's two buffer sets have changed places)
        _check_against_exports(chains, p)
        chains.advance(p["betas"][20:30], sweep_order="colour")
        ladder = np.geomspace(0.5, 5.0, CHAINS)
        chains.exchange(ladder, parity=0)
        _check_against_exports(chains, p)
        saved = chains.state()
        chains.advance(p["betas"][30:], sweep_order="shuffled")
        chains.load_state(saved)
        _check_against_exports(chains, p)
        accuracy, overlap = chains.accuracy_and_overlap(p["exact"], p["weights"])
        assert accuracy.shape == overlap.shape == (CHAINS,) and np.all(accuracy >= 0.5) and np.all(overlap <= 1.0)


def test_scoring_calls_leave_the_chains_untouched(problem):
    from annealing_sign_problem_amd import annealer as sa

    p = problem

    def run(scoring: bool):
        with sa.Chains(p["ham"], seed=5, repetitions=CHAINS) as chains:
            for first in range(0, 40, 10):
                chains.advance(p["betas"][first:first + 10], sweep_order="shuffled")
                if scoring:
                    chains.scores(p["exact"], p["weights"], which="best")
                    chains.scores(p["exact"], which="current")
                    chains.distances("best")
                    chains.distances("current")
                if first == 10:
                    chains.resample(0.2)
            state = chains.state()
            xs, es = chains.result()
        return state, xs, es

    plain, scored = run(False), run(True)
    assert set(plain[0]) == set(scored[0])
    for name in plain[0]:
        assert np.array_equal(plain[0][name], scored[0][name]), name
    assert np.array_equal(plain[1], scored[1]) and plain[2].tobytes() == scored[2].tobytes()


def test_refusals_that_need_a_handle(problem):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    p = problem
    lib = _lib.load()
    with sa.Chains(p["ham"], seed=1, repetitions=3) as chains:
        before = chains.state()
        out = np.full((3, 3), 77, dtype=np.uint32)
        matches = np.full(3, 77, dtype=np.uint64)
        assert lib.asp_sa_chains_distances(chains._live(), ctypes.c_uint32(2), _lib.ptr(out)) == -3
        assert lib.asp_sa_chains_scores(chains._live(), ctypes.c_uint32(2), ctypes.c_uint64(SPINS), None,
                                        _lib.ptr(p["exact"]), None, _lib.ptr(matches), None, None) == -3
        wrong = p["subset"].copy()
        wrong[-1] = SPINS
        assert lib.asp_sa_chains_scores(chains._live(), ctypes.c_uint32(0), ctypes.c_uint64(wrong.shape[0]),
                                        _lib.ptr(wrong), _lib.ptr(p["exact"]), None, _lib.ptr(matches), None,
                                        None) == -3
        assert np.all(out == 77) and np.all(matches == 77)
        with pytest.raises(ValueError):
            chains.scores(p["exact"], which="first")
        after = chains.state()
        assert all(np.array_equal(before[name], after[name]) for name in before)


def test_anneal_until_stops_on_the_accuracy(problem):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import scores

    p = problem
    wanted, sweeps, every = 0.9, 2000, 100
    arguments = dict(seed=9, number_sweeps=sweeps, repetitions=8, check_every=every, only_best=False,
                     sweep_order="shuffled")
    _, _, plain = sa.anneal_until(p["ham"], **arguments)
    xs, es, done = sa.anneal_until(p["ham"], target=(p["exact"], p["weights"], wanted), **arguments)
    assert plain == sweeps and done <= plain and done % every == 0
    assert done < sweeps  # (a planted cluster: 90 % of the signs long before the ladder ends)
    accuracy, _ = scores.accuracy_and_overlap(xs, p["exact"], p["weights"], SPINS)
    assert np.max(accuracy) >= wanted
    # the same segments by hand: the result is theirs, and one segment earlier no chain had met the target
    info = p["ham"].info()
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, sweeps)
    with sa.Chains(p["ham"], seed=9, repetitions=8) as chains:
        for first in range(0, done, every):
            if first > 0:
                assert np.max(chains.accuracy_and_overlap(p["exact"], p["weights"])[0]) < wanted
            chains.advance(ladder[first:first + every], sweep_order="shuffled")
        hxs, hes = chains.result()
    assert np.array_equal(hxs, xs) and hes.tobytes() == es.tobytes()
    # the batch driver: one problem with a target, its clone without
    other = p["ham"].clone()
    try:
        both = sa.anneal_batch_until([p["ham"], other], seed=9, number_sweeps=sweeps, repetitions=8, check_every=every,
                                     only_best=False, sweep_order="shuffled",
                                     target=[(p["exact"], p["weights"], wanted), None])
    finally:
        other.release()
    assert both[0][2] == done and both[1][2] == sweeps
    assert np.array_equal(both[0][0], xs) and both[0][1].tobytes() == es.tobytes()
