"""The cases of tests/descent_cases.py are what they claim — no GPU: every sum is exact, the tie shares and
sweep counts are the recorded ones, the exact reference is the oracle's descent at every cap around t, and
the cases tell `dE < 0` from `dE <= 0`."""
import fractions

import numpy as np
import pytest

import descent_cases as dc
import oracle

ALL = dc.names()
SENSITIVE = dc.names("ties", "ties_field", "stop", "one_step")


def test_the_table_is_complete():
    assert set(dc.RECORDED) == set(ALL) and len(ALL) == 40
    assert len(dc.names("ties")) == len(dc.names("ties_field")) == len(dc.TIE_SIZES) == 10
    assert [n for n in ALL if n.startswith("domino_t")][:9] == ["domino_t%d" % t for t in dc.DOMINO_T]
    assert max(dc.case(name).n for name in ALL) <= 400  # a few hundred spins at the most


@pytest.mark.parametrize("name", ALL)
def test_every_sum_is_exact(name):
    """The exactness condition per row, under all-up, all-down and 20 random sign vectors, in both
    directions of the sum; and the energy's partial sums, except for one_step (q = 2^-51 beside sums of
    hundreds), whose energies are taken from the oracle's summation tree."""
    c = dc.case(name)
    assert dc.rows_are_exact(c.J, c.h) == 22 * c.n
    assert c.energy_exact == (c.family != "one_step")


@pytest.mark.parametrize("name", ALL)
def test_recorded_counts_are_the_reference(name):
    c = dc.case(name)
    t, flips, ties, visits = c.reference.counts()
    print(name, "t = %d, %d flips, %d of %d visits at dE == 0 (%.1f %%)" % (t, flips, ties, visits, 100.0 * ties / visits))
    assert (t, flips, ties, visits) == dc.RECORDED[name]
    assert visits == t * c.n and t < dc.CAP


@pytest.mark.parametrize("name", dc.names("ties", "ties_field"))
def test_tie_share(name):
    """At least 10 % of the visits of the reference descent have dE == 0, and something flips."""
    t, flips, ties, visits = dc.case(name).reference.counts()
    assert 10 * ties >= visits and flips >= 1


@pytest.mark.parametrize("name", dc.names("ties_field"))
def test_fields_cancel_sums_of_both_signs_at_both_spin_values(name):
    """g = +0 from a non-zero cancellation: sum > 0 with h < 0 and the reverse, at s = +1 and s = -1, so that
    dE = -2 s g is formed as -2 * 0 and as 2 * 0."""
    c = dc.case(name)
    assert dc.cancelled_field_kinds(c.J, c.h) == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert np.count_nonzero(c.h) >= c.n // 4 and np.all(c.h == np.rint(c.h))


def test_domino_sweep_counts():
    """Every t around the chunks of 8 sweeps, each taken from the reference; two flips a sweep."""
    for t in dc.DOMINO_T:
        c = dc.case("domino_t%d" % t)
        assert c.t == t and c.reference.ties == 0
        assert dc.spins_of(c.start, c.n) == [1] * c.n
        assert dc.spins_of(c.reference.words, c.n) == [-1] * (c.n - 1) + [1]
        for cap in range(1, t):  # the cascade: one spin in the first sweep, two in every later one
            assert dc.spins_of(c.descent(cap).words, c.n).count(-1) == min(2 * cap - 1, c.n - 1)
    assert {dc.case("domino_t%d" % t).t for t in dc.DOMINO_T} >= {8, 9, 16, 17}
    still = dc.case("domino_t1")
    assert still.t == 1 and np.array_equal(still.reference.words, still.start)
    assert dc.case("domino_beside_ties").t == 17 and dc.case("domino_cached").t == 18


def test_domino_stops_at_the_spin_without_a_field():
    c = dc.case("domino_stop")
    assert c.h[dc.STOP_AT] == 0.0
    assert dc.spins_of(c.reference.words, c.n) == [-1] * dc.STOP_AT + [1] * (c.n - dc.STOP_AT)
    assert c.t == 12 and c.reference.ties == 2  # the stop's visits in the last two sweeps
    other = c.descent(200, "<=")  # with <= the stop gives way and the cascade runs on to the anchor
    assert other.t > c.t and dc.spins_of(other.words, c.n) == [-1] * (c.n - 1) + [1]


def test_domino_cached_is_below_the_field_cache_threshold():
    """The entry rule of cached mode restated (csrc/sa_sweep.hip: cache_enter_flips_of): a sweep with fewer
    flips than max(1, floor(0.7 blocks / max(1, mean degree))) — here 4, and a sweep of the cascade flips 2.
    Every other case has a threshold of 1 or 2 and no flipping sweep below it: cached mode begins behind
    their last flip."""
    def threshold(c):
        where = dc.positions(c.J)
        blocks = sum({colour: count for colour, _, _, count, _ in where.values()}.values())
        degree = max(1.0, sum(len(row) for row in c.model.rows) / c.n)
        return int(max(1.0, 0.7 * blocks / degree))

    assert threshold(dc.case("domino_cached")) == 4
    for name in ALL:
        c = dc.case(name)
        if name != "domino_cached" and threshold(c) > 1:
            assert threshold(c) == 2
            flips = [c.descent(k).flips - c.descent(k - 1).flips for k in range(1, c.t + 1)]
            assert all(f == 0 or f >= 2 for f in flips), name


def test_one_step_probes_sit_at_the_named_lanes():
    """A probe of each side at lanes 0, 1, 31, 62, 63 of a first block and at 0, 1, 31, 61, 62 of a padded
    last block (63 spins: lane 63 is a dummy), in the oracle's visiting order; the mirror model has the other
    side at the same positions; every h_p is +-q or 0 and the centre never flips."""
    sides = {}
    for mirror in (False, True):
        J, h, probes = dc.one_step(mirror)
        c = dc.case("one_step_mirror" if mirror else "one_step")
        assert np.array_equal(J.toarray(), c.J.toarray()) and np.array_equal(h, c.h)
        where = dc.positions(J)
        before, after = dc.spins_of(c.start, c.n), dc.spins_of(c.reference.words, c.n)
        assert {abs(hp) for _, hp, _ in probes} == {0.0, dc.Q}
        for p, hp, flips in probes:
            colour, block, lane, blocks, last = where[p]
            assert (blocks, last) == (2, 63)
            assert (after[p] != before[p]) == flips and (hp != 0.0 or not flips)
            if hp != 0.0:
                sides.setdefault((block, lane), set()).add((mirror, flips))
        others = set(range(c.n)) - {p for p, _, _ in probes}
        assert all(after[i] == before[i] for i in others)
    for block, lanes in ((0, dc.FIRST_LANES), (1, dc.LAST_LANES)):
        for lane in lanes:
            assert {flips for _, flips in sides[block, lane]} == {False, True}, (block, lane)
            assert len(sides[block, lane]) == 2
    colours = {dc.positions(dc.case("one_step").J)[p][0] for p, _, _ in dc.one_step()[2]}
    assert colours == {0, 1, 2}


@pytest.mark.parametrize("name", ALL)
def test_reference_is_the_oracle_at_every_cap(name):
    c = dc.case(name)
    for cap in sorted({0, 1, max(c.t - 1, 0), c.t, c.t + 1, dc.CAP}):
        words, energy, t = c.expected(cap)
        ox, oe = oracle.greedy_solve(c.J, c.h, max_sweeps=cap)
        assert np.array_equal(ox, words) and oe == energy, (name, cap)
        assert t == min(cap, c.t)
        if cap == 0:
            assert np.array_equal(words, c.start)
        exact = c.model.energy(dc.spins_of(words, c.n))
        if c.energy_exact:
            assert fractions.Fraction(oe) == exact
        else:
            assert abs(fractions.Fraction(oe) - exact) <= fractions.Fraction(1, 2 ** 40)
    if c.t >= 2:  # t is the FIRST sweep that flips nothing
        assert not np.array_equal(c.descent(c.t - 2).words, c.reference.words)


@pytest.mark.parametrize("name", SENSITIVE)
def test_cases_tell_less_from_less_or_equal(name):
    c = dc.case(name)
    cap = c.t + 30
    other = c.descent(cap, "<=")
    assert not np.array_equal(other.words, c.reference.words) or other.t != c.t


def test_cancelling_pair_is_the_model_without_it():
    c = dc.case("cancelling_pair")
    J, h = dc.cancelling(65, 4, dc.TIE_SEEDS[65, 4], with_pair=False)
    assert c.J.nnz == J.nnz + 2 and np.array_equal((c.J + c.J.T).toarray(), (J + J.T).toarray())
    plain = dc.case("ties_65_4")
    assert np.array_equal(plain.J.toarray(), J.toarray())
    assert np.array_equal(c.order, plain.order) and np.array_equal(c.start, plain.start)
    assert np.array_equal(c.expected()[0], plain.expected()[0]) and c.expected()[1:] == plain.expected()[1:]
    # (the oracle keeps a stored pair that cancels out of A as well)
    assert oracle.sa_layout(c.J)[3] == oracle.sa_layout(J)[3]


@pytest.mark.parametrize("base", ["ties_65_4", "domino_t9"])
def test_scaled_cases_keep_words_and_sweeps(base):
    b = dc.case(base)
    for scale, exponent in dc.SCALES.items():
        c = dc.case("%s@%s" % (base, scale))
        assert np.array_equal(c.order, b.order) and np.array_equal(c.start, b.start)
        assert np.array_equal(c.reference.words, b.reference.words) and c.reference.counts() == b.reference.counts()
        assert c.expected()[1] == b.expected()[1] * 2.0 ** exponent and np.isfinite(c.expected()[1])
