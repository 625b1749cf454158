"""(no GPU) The inputs of tests/test_gpu_accept_boundaries.py (tests/accept_cases.py), judged with the
oracle alone: that there are enough probes of every kind, that they would notice an exp(-x) one ulp off
or a filter band that is too narrow, that the models present the x they claim, and that the numpy Philox
is the oracle's."""
import math

import numpy as np
import pytest

import accept_cases as ac
import oracle

from accept_cases import SWEEP_CASES, exchange_case, host_scale, sweep_case


def test_numpy_philox_is_the_oracles():
    rng = np.random.default_rng(1)
    counters = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    counters[::7, 2] = 0xFFFFFFFC
    counters[::5, 1] |= np.uint64(2 ** 31)
    seeds = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    seeds[::9] &= np.uint64(0xFFFFFFFF)
    assert (counters >= 2 ** 31).sum() > 1000 and (seeds >= 2 ** 32).sum() > 800
    for c, seed in zip(counters, seeds):
        want = oracle.philox4x32_10(c.astype(np.uint32), [int(seed) & 0xFFFFFFFF, int(seed) >> 32])
        assert np.array_equal(ac.philox(c[0], c[1], c[2], c[3], int(seed)), want), (c, seed)
    # ... and the two word pickers against the laws' own scalar ones
    import tempering_law

    words = ac.exchange_words(np.arange(5, 40, 2), 3, 2 ** 31 + 1, ac.ExchangeCase.SEED)
    assert [int(w) for w in words] == [tempering_law.draw_word(ac.ExchangeCase.SEED, k, 3, 2 ** 31 + 1)
                                       for k in range(5, 40, 2)]
    replicas = np.arange(3, 14)
    words = ac.proposal_words([0, 77, 16383], 1, replicas, ac.SweepCase.SEED)
    key = [ac.SweepCase.SEED & 0xFFFFFFFF, ac.SweepCase.SEED >> 32]
    for a, spin in enumerate([0, 77, 16383]):
        for b, r in enumerate(replicas):
            assert int(words[a, b]) == int(oracle.philox4x32_10([spin, 1, r >> 2, 0], key)[r & 3])


def test_bisection_finds_adjacent_doubles():
    rng = np.random.default_rng(2)
    for word in [0, 1, 2 ** 31, 2 ** 32 - 1] + [int(w) for w in rng.integers(0, 2 ** 32, 300)]:
        pair = ac.boundary(word)
        if pair is None:
            continue
        xa, xb = pair
        assert np.nextafter(xa, 99.0) == xb and ac.accepts(word, xa) and not ac.accepts(word, xb)
        assert abs(ac.delta_of(word, xa)) < 1e-9
    # Probes' vectorised decisions and distances are `accepts` and `delta_of`
    probes = ac.Probes(rng.integers(0, 2 ** 32, 600, dtype=np.uint64), np.arange(600))
    assert probes.accept.tolist() == [ac.accepts(w, x) for w, x in zip(probes.words, probes.x)]
    assert probes.delta.tolist() == [ac.delta_of(w, x) for w, x in zip(probes.words, probes.x)]


def _check_counts(counts, least_above_8):
    print(counts)
    assert counts["probes"] >= 5000
    assert counts["boundary"] >= 1500
    assert counts["in_band"] >= 1000
    assert counts["x_above_8"] >= least_above_8
    assert counts["x_below_1e-3"] >= 100
    assert 0.35 <= counts["accept_share"] <= 0.65
    assert counts["fallbacks"] <= 0.01 * counts["bisected"]


def _check_sharpness(all_probes):
    changed, boundary = (sum(v) for v in zip(*[p.changed_by_exp(lambda x: float(np.exp(-x))) for p in all_probes]))
    print("numpy.exp changes %d of %d boundary probes" % (changed, boundary))
    assert changed >= 0.05 * boundary
    for e in (3e-6, -3e-6):
        misjudged = sum(p.changed_by_misjudged_band(e) for p in all_probes)
        print("a band misjudged by %g changes %d probes" % (e, misjudged))
        assert misjudged >= 50


@pytest.mark.parametrize("name", sorted(SWEEP_CASES))
def test_sweep_probes(name):
    case = sweep_case(name)
    counts = case.probes.counts()
    _check_counts(counts, 150)
    # the probes aimed at a word alone reach both ends as well (the edge values do by themselves)
    assert counts["x_above_8_aimed"] >= 150 and counts["x_below_1e-3_aimed"] >= 100
    _check_sharpness([case.probes])
    assert case.size <= 16384 and set(np.unique(case.probes.cls)) == {ac.BOUNDARY, ac.LADDER, ac.EDGE}


def test_exchange_probes():
    case = exchange_case()
    assert len(case.steps) == 2 * len(case.draws) and len(case.draws) >= 16
    counts = case.counts()
    _check_counts(counts, 100)
    # ... of probes whose x follows from the word, as in the sweeps
    assert counts["x_above_8_aimed"] >= 100 and counts["x_below_1e-3_aimed"] >= 100
    _check_sharpness(case.all_probes())


def test_exchange_steps_are_the_laws():
    """What the GPU file expects of every step (ExchangeCase.expected: tempering_law.select with the numpy
    Philox words) is tempering_law.exchange with its own scalar Philox, and swaps the pairs whose probe the
    oracle accepts: the ladder presents probes.x."""
    import tempering_law

    case = exchange_case()
    for (parity, draw), (pairs, probes, betas) in sorted(case.steps.items()):
        source, accepted = case.expected(parity, draw)
        law_source, law_accepted = tempering_law.exchange(case.energies, betas, parity, case.SEED, case.SWEEPS_DONE, draw)
        assert np.array_equal(source, law_source) and accepted == law_accepted, (parity, draw)
        assert np.array_equal(source[pairs] == pairs + 1, probes.accept) and accepted == int(probes.accept.sum())


@pytest.mark.parametrize("order", ["colour", "shuffled"])
@pytest.mark.parametrize("model", ["isolated", "pairs"])
@pytest.mark.parametrize("ladder", [False, True], ids=["plain", "ladder"])
def test_model_presents_its_probes(model, order, ladder):
    """A small case through the oracle's annealer: the best configuration it reports is the state after
    sweep 1, where exactly the accepted probe spins are down, the gate is up and the helper is up; the
    accepted counts are K + 2 more."""
    case = ac.SweepCase(model, 190, 18, first=5, order=order, ladder=ladder)
    anneal = oracle.sa_anneal if order == "colour" else oracle.sa_anneal_shuffled
    down = case.expected_down()
    scale, colours, _ = host_scale(case)
    assert colours >= 2 and ac.BIG * 2.0 ** scale >= 1.0
    assert np.array_equal(down[np.arange(case.K), case.designated], case.probes.accept)
    for beta in np.unique(case.chain_betas):
        xs, es, tracked, accepted = anneal(case.J, case.field, case.SEED, beta * case.betas, case.R, case.first,
                                           case.x0, scale)
        for r in np.nonzero(case.chain_betas == beta)[0]:
            bits = np.unpackbits(xs[r].view(np.uint8), bitorder="little")[:case.size]
            assert np.array_equal(bits[:case.K] == 0, down[:, r]), (beta, r)
            assert bits[case.K] == 1 and bits[case.K + 1] == 1
            assert accepted[r] == case.K + 2 + down[:, r].sum()


def test_weight_gaps():
    field, x0, gaps = ac.weight_case()
    signs = 2.0 * ((x0[:, 0][:, None] >> np.arange(ac.WEIGHT_SPINS, dtype=np.uint64)) & np.uint64(1)) - 1.0
    energies = [math.fsum(row * field) for row in signs]
    assert [e - min(energies) for e in energies] == list(gaps)
    assert gaps[0] == 0.0 and gaps[1] == ac.WEIGHT_GRID and gaps[2] < 23.0 == gaps[3] and len(gaps) == 4 + 2 * 264
    import population_law

    q = population_law.weights(energies, 1.0)
    assert q[0] == 2 ** 31 and q[3] == 0 and sum(q) >= 2 ** 31 and len(q) * sum(q) <= 2 ** 63
    # either side of every step: floor(expneg(gap) 2^31) is q above and q - 1 below
    steps = sum(q[j] - q[j + 1] == 1 for j in range(4, len(q), 2))
    print("weight steps straddled: %d of 264" % steps)
    assert steps >= 260
