"""The numpy law of the sign scores (tests/score_cases.py, specification ASP-SCORE-1)
against the host route it restates, on every named case and without a GPU: the accuracy derived from
`matches` IS common.compute_accuracy_and_overlap's, the overlap derived from the tree is within
(K0 + 64) * 2^-53 of it, the tree's sum is within the same bound (times the total) of math.fsum, and the
distances equal a brute-force loop."""
import math

import numpy as np
import pytest

import score_cases

NAMES = sorted(score_cases.cases())
DISTANCE_NAMES = sorted(score_cases.distance_cases())


def _bound(scored: int) -> float:
    return (scored + 64) * 2.0 ** -53


def test_the_axes_are_covered():
    cases = score_cases.cases()
    assert {c["scored"] for c in cases.values()} >= set(score_cases.SCORED)
    assert {c["xs"].shape[0] for c in cases.values()} >= set(score_cases.COUNTS)
    assert any(c["xs"].shape[1] > score_cases.words_of(c["spins"]) for c in cases.values())
    assert any(c["select"] is not None and c["scored"] < c["spins"] for c in cases.values())
    assert any(c["select"] is not None and c["scored"] > c["spins"] for c in cases.values())
    assert any(c["weights"] is not None and np.any(c["weights"] == 0) and np.any(c["weights"] > 0)
               and np.any((c["weights"] > 0) & (c["weights"] < 2.3e-308)) for c in cases.values())
    assert any(c["weights"] is not None and not np.any(c["weights"]) for c in cases.values())
    distance = score_cases.distance_cases()
    assert {xs.shape[0] for xs, _ in distance.values()} >= set(score_cases.DISTANCE_COUNTS)
    assert {score_cases.words_of(k) for _, k in distance.values()} >= set(score_cases.DISTANCE_WORDS)
    # 7 passes + 1: the binary counter of pass partials carries twice (passes 1 -> 2 and 3 -> 4)
    assert (7 * score_cases.PASS + 1) in score_cases.SCORED


def test_tree_sum_is_the_pairwise_tree():
    assert score_cases.tree_sum([]) == 0.0 and not np.signbit(score_cases.tree_sum([]))
    assert score_cases.tree_sum([3.0]) == 3.0
    # (a + b) + (c + 0), not ((a + b) + c): the two differ for these values
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    assert score_cases.tree_sum([a, b, c]) == (a + b) + (c + 0.0)
    values = np.random.default_rng(1).normal(size=11)
    v = list(values) + [0.0] * 5
    want = (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) + \
           (((v[8] + v[9]) + (v[10] + v[11])) + ((v[12] + v[13]) + (v[14] + v[15])))
    assert score_cases.tree_sum(values) == want


@pytest.mark.parametrize("name", NAMES)
def test_law_against_the_host_function(name):
    from annealing_sign_problem_amd import common
    from annealing_sign_problem_amd.scores import accuracy_and_overlap_of

    case = score_cases.cases()[name]
    matches, signed, total = score_cases.laws()[name]
    scored = case["scored"]
    accuracy, overlap = accuracy_and_overlap_of(matches, signed, total, scored)
    predicted = score_cases.pack(score_cases.gathered(case))  # the scored bits, in scoring order
    weights = case["weights"]
    terms_w = np.ones(scored) if weights is None else weights
    exact_bits = score_cases.unpack(case["exact"], scored)
    assert abs(total - math.fsum(terms_w)) <= _bound(scored) * math.fsum(terms_w)
    for c in range(predicted.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore"):
            host_accuracy, host_overlap = common.compute_accuracy_and_overlap(
                predicted[c], case["exact"], weights, number_spins=scored)
        assert np.float64(accuracy[c]).view(np.uint64) == np.float64(host_accuracy).view(np.uint64)
        if total == 0.0:
            assert np.isnan(overlap[c]) and np.isnan(host_overlap)
        else:
            assert abs(overlap[c] - host_overlap) <= _bound(scored), (overlap[c], host_overlap)
        same = score_cases.gathered(case)[c] == exact_bits
        exact_sum = math.fsum(np.where(same, terms_w, -terms_w))
        assert abs(signed[c] - exact_sum) <= _bound(scored) * total
    if not name.endswith("repeats") and predicted.shape[0] > 1:  # the planted contents
        assert matches[0] == scored and matches[1] == 0 and accuracy[0] == accuracy[1] == 1.0


@pytest.mark.parametrize("name", DISTANCE_NAMES)
def test_distance_law_against_a_loop(name):
    xs, spins = score_cases.distance_cases()[name]
    law = score_cases.distances_law(xs, spins)
    words = score_cases.words_of(spins)
    mask = [(1 << 64) - 1] * words
    if spins % 64:
        mask[-1] = (1 << (spins % 64)) - 1
    rows = [[int(w) & m for w, m in zip(row[:words], mask)] for row in xs]
    count = len(rows)
    # (every pair of the small cases, a band of the large ones: the loop is Python)
    for a in range(count):
        for b in (range(count) if count <= 65 else (a, (a + 1) % count, (a + 64) % count, count - 1 - a)):
            assert law[a, b] == sum(bin(p ^ q).count("1") for p, q in zip(rows[a], rows[b])), (a, b)
    assert np.array_equal(law, law.T) and not np.any(np.diag(law))
    if count > 2:
        assert law[0, 1] == spins and law[0, 2] == 0
