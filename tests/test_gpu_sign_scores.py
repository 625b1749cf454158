"""Sign scores on the GPU (csrc/sign_scores.hip, annealing_sign_problem_amd/scores.py, specification
ASP-SCORE-1 in DESIGN.md §3.11): every named case of tests/score_cases.py against the numpy law bit for
bit — matches, the signed tree, the total, the distances —, the batch call on all cases at once in two
item orders, the derived accuracy and overlap against the host function, and two threads side by side."""
import threading

import numpy as np
import pytest

import score_cases

pytestmark = pytest.mark.gpu

NAMES = sorted(score_cases.cases())
DISTANCE_NAMES = sorted(score_cases.distance_cases())


def _arguments(case):
    return case["xs"], case["exact"], case["weights"], case["select"], case["spins"]


def _assert_is_law(got, law, name):
    matches, signed, total = got
    want_matches, want_signed, want_total = law
    assert matches.dtype == np.uint64 and np.array_equal(matches, want_matches), name
    assert np.array_equal(score_cases.bits_of(signed), score_cases.bits_of(want_signed)), name
    assert score_cases.bits_of(total) == score_cases.bits_of(want_total), name


@pytest.mark.parametrize("name", NAMES)
def test_scores_are_the_law_bit_for_bit(name):
    from annealing_sign_problem_amd import scores

    case = score_cases.cases()[name]
    _assert_is_law(scores.sign_scores(*_arguments(case)), score_cases.laws()[name], name)
    assert scores.last_ms() > 0.0


def test_batch_in_two_orders_is_the_single_calls():
    from annealing_sign_problem_amd import scores

    cases, laws = score_cases.cases(), score_cases.laws()
    for order in (NAMES, NAMES[::-1][3:] + NAMES[::-1][:3]):
        got = scores.sign_scores_batch([_arguments(cases[name]) for name in order])
        for name, result in zip(order, got):
            _assert_is_law(result, laws[name], name)
    # dict items, and an item without configurations in the middle of a batch
    some = [dict(xs=cases[n]["xs"], exact=cases[n]["exact"], weights=cases[n]["weights"], select=cases[n]["select"],
                 number_spins=cases[n]["spins"]) for n in NAMES[:3]]
    some[1] = dict(some[1], xs=some[1]["xs"][:0])
    got = scores.sign_scores_batch(some)
    _assert_is_law(got[0], laws[NAMES[0]], NAMES[0])
    _assert_is_law(got[2], laws[NAMES[2]], NAMES[2])
    assert got[1][0].shape == (0,)


def test_outputs_may_be_null_and_no_scored_positions():
    import ctypes

    from annealing_sign_problem_amd import _lib, scores

    case = score_cases.cases()["w_lognormal_s_subset"]
    xs, exact, weights, select, spins = _arguments(case)
    signed = np.zeros(xs.shape[0])
    _lib.check(_lib.load().asp_sign_scores(
        ctypes.c_uint64(spins), ctypes.c_uint32(xs.shape[0]), _lib.ptr(xs), ctypes.c_uint64(xs.shape[1]),
        ctypes.c_uint64(case["scored"]), _lib.ptr(select), _lib.ptr(exact), _lib.ptr(weights), None,
        _lib.ptr(signed), None))
    assert np.array_equal(score_cases.bits_of(signed), score_cases.bits_of(score_cases.laws()[case["name"]][1]))
    # K0 = 0: through an empty select, and through K = 0
    for arguments in ((xs, exact, np.zeros(0), np.zeros(0, dtype=np.int32), spins),
                      (np.zeros((2, 0), dtype=np.uint64), np.zeros(0, dtype=np.uint64), None, None, 0)):
        matches, signed, total = scores.sign_scores(*arguments)
        assert not matches.any() and not signed.any() and total == 0.0
        assert not np.signbit(signed).any() and not np.signbit(total)


@pytest.mark.parametrize("name", NAMES[::4])
def test_accuracy_and_overlap_against_the_host_function(name):
    from annealing_sign_problem_amd import common, scores

    case = score_cases.cases()[name]
    scored = case["scored"]
    accuracy, overlap = scores.accuracy_and_overlap(case["xs"], case["exact"], case["weights"], case["spins"],
                                                    case["select"])
    predicted = score_cases.pack(score_cases.gathered(case))
    for c in range(min(predicted.shape[0], 8)):
        with np.errstate(invalid="ignore", divide="ignore"):
            host_accuracy, host_overlap = common.compute_accuracy_and_overlap(predicted[c], case["exact"],
                                                                              case["weights"], number_spins=scored)
        assert np.float64(accuracy[c]).view(np.uint64) == np.float64(host_accuracy).view(np.uint64)
        if np.isnan(host_overlap):
            assert np.isnan(overlap[c])
        else:
            assert abs(overlap[c] - host_overlap) <= (scored + 64) * 2.0 ** -53


def test_plural_host_function_is_one_batch_call():
    from annealing_sign_problem_amd import common

    names = [n for n in NAMES if score_cases.cases()[n]["select"] is None and score_cases.cases()[n]["weights"] is not None
             and np.any(score_cases.cases()[n]["weights"])]
    cases = [score_cases.cases()[n] for n in names]
    predicted = [c["xs"][-1] for c in cases]  # (rows with a stride: the function takes the first W words)
    got = common.compute_accuracies_and_overlaps(predicted, [c["exact"] for c in cases], [c["weights"] for c in cases])
    assert len(got) == len(cases)
    for case, p, (accuracy, overlap) in zip(cases, predicted, got):
        host_accuracy, host_overlap = common.compute_accuracy_and_overlap(p, case["exact"], case["weights"])
        assert np.float64(accuracy).view(np.uint64) == np.float64(host_accuracy).view(np.uint64)
        assert abs(overlap - host_overlap) <= (case["scored"] + 64) * 2.0 ** -53


@pytest.mark.parametrize("name", DISTANCE_NAMES)
def test_distances_are_exact(name):
    from annealing_sign_problem_amd import scores

    xs, spins = score_cases.distance_cases()[name]
    got = scores.sign_distances(xs, spins)
    assert got.dtype == np.uint32 and got.shape == (xs.shape[0],) * 2
    assert np.array_equal(got, score_cases.distances_law(xs, spins))


def test_two_threads_side_by_side():
    from annealing_sign_problem_amd import scores

    cases, laws = score_cases.cases(), score_cases.laws()
    distance = score_cases.distance_cases()
    failures = []

    def work(names, distance_name):
        try:
            for _ in range(3):
                for name in names:
                    _assert_is_law(scores.sign_scores(*_arguments(cases[name])), laws[name], name)
                xs, spins = distance[distance_name]
                assert np.array_equal(scores.sign_distances(xs, spins), score_cases.distances_law(xs, spins))
        except BaseException as exc:  # (an assertion in a thread would be lost)
            failures.append(exc)

    threads = [threading.Thread(target=work, args=(NAMES[0::2][:12], "c130_w17_tail")),
               threading.Thread(target=work, args=(NAMES[1::2][:12], "c65_w3_stride"))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
