"""Consensus signs on the GPU (csrc/sign_vote.hip, annealing_sign_problem_amd/scores.py, law ASP-VOTE-1 in
DESIGN.md §3.12): every named case of tests/vote_cases.py against the numpy restatement bit for bit —
distances, flips, counts, the two sums, the consensus and the number of changed sites —, the batch call on
all cases at once and permuted with an empty item in the middle, and the outputs left out one at a time."""
import ctypes

import numpy as np
import pytest

import vote_cases

pytestmark = pytest.mark.gpu

NAMES = sorted(vote_cases.cases())


@pytest.mark.parametrize("name", NAMES)
def test_vote_is_the_law_bit_for_bit(name):
    from annealing_sign_problem_amd import scores

    case = vote_cases.cases()[name]
    got = scores.consensus(*vote_cases.arguments(case))
    assert vote_cases.same(got, vote_cases.laws()[name]), name
    assert got.ones.dtype == np.uint32 and got.distance.dtype == np.uint32 and got.x.dtype == np.uint64
    assert scores.vote_last_ms() > 0.0
    # the margin is the host's division of the two sums
    total = got.plus + got.minus
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got.margin, np.where(total != 0, (got.plus - got.minus) / total, 0.0))


def test_batch_and_permuted_batch_are_the_single_calls():
    from annealing_sign_problem_amd import scores

    cases, laws = vote_cases.cases(), vote_cases.laws()
    got = scores.consensus_batch([vote_cases.arguments(cases[name]) for name in NAMES])
    for name, result in zip(NAMES, got):
        assert vote_cases.same(result, laws[name]), name
    # another order, an item without configurations in the middle, dict items
    order = list(np.random.default_rng(3).permutation(NAMES))
    items = [dict(zip(("xs", "number_spins", "weights", "ref", "anchor", "align", "rounds"),
                      vote_cases.arguments(cases[name]))) for name in order]
    middle = len(items) // 2
    items.insert(middle, dict(xs=np.zeros((0, 5), dtype=np.uint64), number_spins=300))
    got = scores.consensus_batch(items)
    assert got[middle].distance.shape == (0,) and not got[middle].x.any()
    del got[middle]
    for name, result in zip(order, got):
        assert vote_cases.same(result, laws[name]), name


@pytest.mark.parametrize("name", ["rounds2_weighted", "stride_k257"])  # (with weights, and the integer path)
def test_outputs_may_be_null_one_at_a_time(name):
    from annealing_sign_problem_amd import _lib, scores

    case, law = vote_cases.cases()[name], vote_cases.laws()[name]
    fields = ("out_distance", "out_flipped", "out_ones", "out_plus", "out_minus", "out_consensus", "out_changed")
    law_of_field = dict(zip(fields, (law["distance"], law["flipped"].astype(np.uint8), law["ones"], law["plus"],
                                     law["minus"], law["x"], np.array([law["changed"]], dtype=np.uint32))))
    for missing in fields + (None,):
        vote = scores._as_vote(vote_cases.arguments(case))
        item = (_lib.SignVoteItem * 1)()
        vote.fill(item[0])
        if missing is not None:
            setattr(item[0], missing, None)
        _lib.check(_lib.load().asp_sign_vote_batch(item, ctypes.c_uint32(1)))
        arrays = dict(zip(fields, (vote.distance, vote.flipped, vote.ones, vote.plus, vote.minus, vote.x, vote.changed)))
        for field, array in arrays.items():
            if field == missing:
                assert not array.any(), (missing, field)  # (as it was allocated)
            else:
                assert array.tobytes() == law_of_field[field].tobytes(), (missing, field)
    # every per-site output missing at once: the consensus alone, as the drivers take it
    vote = scores._as_vote(vote_cases.arguments(case))
    item = (_lib.SignVoteItem * 1)()
    vote.fill(item[0])
    item[0].out_ones = item[0].out_plus = item[0].out_minus = None
    _lib.check(_lib.load().asp_sign_vote_batch(item, ctypes.c_uint32(1)))
    assert np.array_equal(vote.x, law["x"]) and int(vote.changed[0]) == law["changed"]
