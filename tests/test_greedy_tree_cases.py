"""The named cases of tests/greedy_tree_cases.py without a GPU: the plain-Python restatement of
ASP-GREEDY-1's steps 1-3 equals the host tree (asp_sa_greedy_tree_host) and the CPU oracle on every case,
every named wrong variant is told apart by a named case, and the sizes still cross the boundaries they
name."""
import numpy as np
import pytest

import greedy_tree_cases as cases
import oracle

SLOW_IN_PYTHON = ("sparse_50000",)  # (restated once, with the law only)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_equals_host_tree_and_oracle(name):
    J, h = cases.case(name)
    host = cases.reference(name)
    assert host.shape == ((J.shape[0] + 63) // 64,)
    assert np.array_equal(cases.tree(J, h), host)
    assert np.array_equal(oracle.greedy_solve(J, h, relax=False)[0], host)
    tail = J.shape[0] % 64
    if tail:
        assert int(host[-1]) >> tail == 0  # the bits beyond K


def test_the_sum_order_cases_give_the_words_the_law_names():
    for name, word in cases.EXPECTED_WORDS.items():
        J, h = cases.case(name)
        assert int(cases.reference(name)[0]) == word
        assert int(cases.tree(J, h, "row_reversed")[0]) == word ^ 0b10000
    J, h = cases.case("sum_order")
    assert int(cases.tree(J, h, "row_pairwise")[0]) != cases.EXPECTED_WORDS["sum_order"]


@pytest.mark.parametrize("variant", sorted(cases.VARIANTS))
def test_every_wrong_variant_is_told_apart(variant):
    name = cases.TOLD_APART[variant]
    J, h = cases.case(name)
    assert not np.array_equal(cases.tree(J, h, variant), cases.reference(name)), (variant, name)


def test_variants_and_cases_are_all_named():
    assert sorted(cases.TOLD_APART) == sorted(cases.VARIANTS) and len(cases.VARIANTS) == 10
    assert set(cases.TOLD_APART.values()) <= set(cases.CASES)
    with pytest.raises(AssertionError):
        cases.tree(*cases.case("k2"), variant="no such variant")


def test_sizes_cross_the_boundaries_they_name():
    spins = {name: cases.case(name)[0].shape[0] for name in cases.CASES}
    assert [spins[n] for n in ("k1", "k2", "k63", "k64", "k65", "k130")] == [1, 2, 63, 64, 65, 130]
    bonds = {name: cases.bond_count(cases.case(name)[0]) for name in cases.CASES if name != "sparse_50000"}
    assert [bonds[n] for n in ("bonds_63", "bonds_64", "bonds_65")] == [63, 64, 65]
    W = cases.FILTER_WINDOW
    assert [bonds["bonds_window" + s] for s in ("_minus_1", "", "_plus_1")] == [W - 1, W, W + 1]
    assert bonds["no_bonds"] == 0 and bonds["k1"] == 0
    for row in (63, 64, 65, 300):  # the hub's row, and the hub is the last to join (its bonds are the weakest)
        A = cases.couplings(cases.case("hub_%d" % row)[0])
        assert A.indptr[row + 1] - A.indptr[row] == row
        assert np.abs(A.data[A.indptr[row]:A.indptr[row + 1]]).max() < np.abs(A[:row, :row].data).min()
    # a whole filter window of skips: the strongest 33 bonds span the 34 spins, 528 skips follow
    assert bonds["window_of_skips"] == 34 * 33 // 2 + 1 and 33 + 2 * W <= bonds["window_of_skips"]
    # every |w| equal
    for name in ("ring_ties", "random_ties", "random_ties_300"):
        assert set(np.abs(cases.couplings(cases.case(name)[0]).data)) == {1.0}
    # the forest of the large case does not fit 160 KiB of LDS at 8 bytes per spin; the planted one does
    assert 8 * spins["sparse_50000"] > 160 * 1024 and spins["planted_3000"] == 3000
    assert 3.0 < 2 * cases.bond_count(cases.case("sparse_50000")[0]) / spins["sparse_50000"] < 5.0
    # the field of the order case changes the sign of a cluster's sum with the direction of the walk
    h = cases.case("components_field_order")[1]
    assert (h[0] + h[1]) + h[2] == 0.0 and (h[2] + h[1]) + h[0] > 0.0
