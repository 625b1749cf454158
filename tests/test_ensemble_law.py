"""No device: the exact joint law of small tempering ensembles (tests/ensemble_exact_law.py) -- the
properties of its operators, the power of every run that tests/test_gpu_ensemble_law.py makes on the
device (a condition on the inputs: starts, betas, rounds and sample counts), and the whole harness
end to end on a plain numpy sampler, with the true process passing and wrong processes rejected."""
import numpy as np
import pytest

import ensemble_exact_law as law
import sa_exact_law

ORDERS = ("colour", "shuffled")
RULES = sorted(law.WRONG_LAWS)
LADDER = (0.3, 0.8, 1.4)      # beta dE < 23 and |dbeta dE| < 23 on system Q: nothing is cut off


def _q():
    return law.system("Q")


def _columns_sum_to_one(M):
    sums = np.asarray(M.sum(axis=0)).ravel()
    return np.max(np.abs(sums - 1.0)) <= 1e-14


def test_system_q_is_what_the_law_tests_need():
    J, h = law.system_q()
    q = _q()
    assert h.shape[0] == 5
    for values in (J, h):
        assert np.array_equal(values * 8, np.round(values * 8)) and np.max(np.abs(values)) <= 2.0
    assert not np.array_equal(J, J.T) and np.any(np.diag(J) != 0.0)
    # frustrated: no configuration satisfies every bond
    c = np.arange(32)
    s = 2.0 * ((c[:, None] >> np.arange(5)) & 1) - 1.0
    bonds = 0.5 * np.einsum("ci,ij,cj->c", s, q.A, s)
    assert bonds.min() > -0.5 * np.abs(q.A).sum()
    # a differing set whose induced graph is disconnected, with a component of more than one site
    comp = law.component_table(q.A, 5)
    D = 0b01101
    assert comp[D, 0] == 0b00001 and comp[D, 2] == 0b01100 and comp[D, 3] == 0b01100
    # the hairpin's and the embedded run's cluster pairs start on such sets
    starts = law.CASES["hairpin"]["starts"]
    assert starts[0] ^ starts[3] == 0b01101 and starts[1] ^ starts[2] == 0b10011
    assert comp[0b10011, 0] == 0b00011 and comp[0b10011, 4] == 0b10000


def test_every_operator_is_column_stochastic():
    q = _q()
    for beta in (0.0, 0.4, 1.25, 4.0, np.inf):
        for order in (q.colour, q.colour[::-1]):
            assert _columns_sum_to_one(law.sweep_operator(q.E, beta, order))
    for rule in [None] + RULES:
        assert _columns_sum_to_one(law.exchange_operator(q.E, 0.4, 1.25, rule))
        assert _columns_sum_to_one(law.exchange_operator(q.E, 3.0, 0.0, rule))     # x beyond 23 both ways
        assert _columns_sum_to_one(law.cluster_operator(q.A, q.n, rule))
    p1 = law.System(*law.system_p1())
    assert _columns_sum_to_one(law.cluster_operator(p1.A, p1.n))
    assert _columns_sum_to_one(law.exchange_operator(p1.E, 0.25, 1.5))


@pytest.mark.parametrize("order", ORDERS)
def test_one_slot_is_the_single_chain_law(order):
    """G = 1: the product of sweep operators is sa_exact_law.propagate's current law, for a ladder with
    beta = 0 and beta = +inf, from a point mass and from the uniform start."""
    q = _q()
    betas = sa_exact_law.LADDER
    orders = q.orders(order, betas.shape[0])
    for x0 in (18, None):
        want = sa_exact_law.propagate(q.E, betas, orders, x0).current
        p = np.full(q.size, 1.0 / q.size) if x0 is None else np.eye(q.size)[x0]
        for t, beta in enumerate(betas):
            p = law.sweep_operator(q.E, beta, orders[t]) @ p
            assert np.max(np.abs(p - want[t + 1])) <= 1e-13
    # ... and through the ensemble's own sweep on a constant beta
    ens = law.Ensemble(q, [0.7], [18])
    for t in range(3):
        ens.sweep(orders[t])
    want = sa_exact_law.propagate(q.E, [0.7] * 3, orders[:3], 18).current[3]
    assert np.max(np.abs(ens.marginal(0) - want)) <= 1e-13


def test_the_cluster_operator_is_symmetric_and_conserves_the_energy_sum():
    for sys_ in (_q(), law.System(*law.system_p1())):
        M = law.cluster_operator(sys_.A, sys_.n)
        assert abs(M - M.T).max() == 0.0
        M = M.tocoo()
        total = (sys_.E[:, None] + sys_.E[None, :]).ravel()
        assert np.array_equal(total[M.row], total[M.col])       # dyadic: exact
        # wrong law H does not conserve it
        H = law.cluster_operator(sys_.A, sys_.n, "H").tocoo()
        assert not np.array_equal(total[H.row], total[H.col])


def test_the_reported_cluster_law_is_a_law_and_tells_e_and_f_apart():
    q = _q()
    pair = np.multiply.outer(law.boltzmann(q.E, 0.4), law.boltzmann(q.E, 0.4))
    true = law.cluster_report_law(q.A, q.n, pair)
    assert abs(true.sum() - 1.0) <= 1e-14
    cells = true.reshape(q.n + 1, q.n + 1)
    assert np.all(cells[np.triu_indices(q.n + 1, 1)] == 0.0)        # size <= differing
    assert cells[0, 0] == pytest.approx(np.trace(pair)) and np.all(cells[1:, 0] == 0.0)
    e = law.cluster_report_law(q.A, q.n, pair, "E").reshape(q.n + 1, q.n + 1)
    f = law.cluster_report_law(q.A, q.n, pair, "F").reshape(q.n + 1, q.n + 1)
    assert np.allclose(e.sum(axis=1), cells.sum(axis=1)) and np.allclose(f.sum(axis=1), cells.sum(axis=1))
    assert np.all(e[:, 2:] == 0.0) and np.all(f == np.diag(np.diag(f)))
    assert np.abs(e - cells).max() > 1e-2 and np.abs(f - cells).max() > 1e-2


def _ladder_is_not_cut_off(q, betas):
    idx = np.arange(q.size)
    de = max(np.max(q.E[idx ^ (1 << i)] - q.E) for i in range(q.n))
    span = q.E.max() - q.E.min()
    return max(betas) * de < 23.0 and (max(betas) - min(betas)) * span < 23.0


def test_the_product_boltzmann_measure_is_a_fixed_point_of_the_true_operators_only():
    q = _q()
    assert _ladder_is_not_cut_off(q, LADDER)
    pi = {beta: law.boltzmann(q.E, beta) for beta in LADDER}
    for beta in LADDER:
        for order in (q.colour, q.colour[::-1]):
            assert np.max(np.abs(law.sweep_operator(q.E, beta, order) @ pi[beta] - pi[beta])) <= 1e-12
        same = np.multiply.outer(pi[beta], pi[beta]).ravel()
        assert np.max(np.abs(law.cluster_operator(q.A, q.n) @ same - same)) <= 1e-12
        for rule in "EH":
            assert np.max(np.abs(law.cluster_operator(q.A, q.n, rule) @ same - same)) > 1e-3
        # F swaps the two replicas and G does nothing: both keep a product of equal factors
        for rule in "FG":
            assert np.max(np.abs(law.cluster_operator(q.A, q.n, rule) @ same - same)) <= 1e-12
    for a in LADDER:
        for b in LADDER:
            both = np.multiply.outer(pi[a], pi[b]).ravel()
            assert np.max(np.abs(law.exchange_operator(q.E, a, b) @ both - both)) <= 1e-12
            if a != b:
                for rule in "BD":
                    assert np.max(np.abs(law.exchange_operator(q.E, a, b, rule) @ both - both)) > 1e-3


@pytest.mark.parametrize("rule", [None] + RULES)
def test_the_product_measure_through_the_hairpin_rounds(rule):
    """The hairpin's rounds from the product Boltzmann measure of (b0, b1, b1, b0): the true composition
    keeps it to 1e-12, and so do the omitted moves A and G and the swap of equal-beta replicas F (which is
    why the invariance run on the device cannot see them); B, C, D, E, H and I do not."""
    q = _q()
    betas = (LADDER[0], LADDER[2], LADDER[2], LADDER[0])
    starts = [law.boltzmann(q.E, beta) for beta in betas]
    ens = law.Ensemble(q, betas, starts, rule)
    orders = q.orders("shuffled", 4)
    for t in range(4):
        ens.sweep(orders[t])
        ens.cluster([(0, 3), (1, 2)])
        ens.exchange([(0, 1), (2, 3)])
    ens.sweep(q.colour)
    joint = ens.joint((0, 1, 2, 3))
    want = np.multiply.outer(np.multiply.outer(starts[0], starts[1]), np.multiply.outer(starts[2], starts[3]))
    assert abs(joint.sum() - 1.0) <= 1e-12
    error = np.max(np.abs(joint - want))
    if rule in (None, "A", "F", "G"):
        assert error <= 1e-12
    else:
        assert error > 1e-4


def test_the_ensemble_applies_the_operators_along_the_right_axes():
    """Ensemble.exchange works cell by cell and Ensemble.cluster through the sparse operator: both are
    the pair operators above on the pair's joint law, whichever axes the pair has in its factor."""
    q = _q()
    rng = np.random.default_rng(5)
    betas = (0.4, 1.25, 0.7)
    starts = [rng.dirichlet(np.ones(q.size)) for _ in betas]
    pair = np.multiply.outer(starts[0], starts[1]).ravel()
    for rule in [None, "A", "B", "C", "D"]:
        ens = law.Ensemble(q, betas, starts, rule)
        swaps = ens.exchange([(0, 1)])
        want = law.exchange_operator(q.E, betas[0], betas[1], rule) @ pair
        assert np.max(np.abs(ens.pair(0, 1).ravel() - want)) <= 1e-15
        assert swaps == pytest.approx(float(law.swap_probability(q.E, betas[0], betas[1], rule).ravel() @ pair))
        assert np.max(np.abs(ens.marginal(2) - starts[2])) == 0.0
    for rule in [None, "E", "F", "G", "H"]:
        ens = law.Ensemble(q, betas, starts, rule)
        ens.cluster([(0, 1)])
        want = law.cluster_operator(q.A, q.n, rule) @ pair
        assert np.max(np.abs(ens.pair(0, 1).ravel() - want)) <= 1e-15
    # the factor's axes in the other order: the true move treats a and b alike
    runs = []
    for first in ((0, 1), (1, 0)):
        ens = law.Ensemble(q, betas, starts)
        ens.cluster([first])
        ens.exchange([(0, 1)])
        ens.cluster([(2, 0)])
        runs.append(ens.joint((0, 1, 2)))
    assert np.max(np.abs(runs[0] - runs[1])) <= 1e-15


def test_forgetting_keeps_what_it_promises():
    """The embedded run's shortcut on system Q, where the four-slot joint law is affordable: after
    ``forget`` the marginals, the cluster pairs' joint laws and the reported law are those of the full
    joint law, and a projection across factors is refused."""
    q = _q()
    betas, starts = (0.4, 1.25, 1.25, 0.4), (18, 1, 18, 31)
    orders = q.orders("shuffled", 4)
    runs = []
    for forget in (False, True):
        ens = law.Ensemble(q, betas, starts)
        for t in range(2):
            ens.sweep(orders[t])
            ens.exchange([(0, 1), (2, 3)])
        ens.sweep(orders[2])
        if forget:
            ens.forget()
        reports = ens.cluster([(0, 3), (1, 2)])
        ens.sweep(orders[3])
        runs.append((ens, reports))
    (full, full_reports), (short, short_reports) = runs
    for a, b in zip(full_reports, short_reports):
        assert np.max(np.abs(a - b)) <= 1e-14
    for g in range(4):
        assert np.max(np.abs(full.marginal(g) - short.marginal(g))) <= 1e-14
    for pair in ((0, 3), (1, 2)):
        assert np.max(np.abs(full.pair(*pair) - short.pair(*pair))) <= 1e-14
    with pytest.raises(AssertionError):
        short.pair(0, 1)
    with pytest.raises(AssertionError):
        short.exchange([(0, 1)])        # slots whose joint law was forgotten


def test_the_invariance_plan():
    q = _q()
    assert _ladder_is_not_cut_off(q, law.INVARIANCE_BETAS)
    R = (1 << 16) + 1
    betas, pairs = law.invariance_plan(R)
    assert betas.shape == (R,) and np.all(betas[1:] != betas[:-1])         # both parities: different betas
    assert np.array_equal(betas[pairs[:, 0]], betas[pairs[:, 1]])          # cluster pairs: equal betas
    assert np.unique(pairs).size == pairs.size and pairs.max() < R
    assert len(set(law.INVARIANCE_BETAS)) == 3


# ----------------------------------------------------------------------------
# the power of the planned device runs
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(law.CASES))
def test_the_planned_run_can_reject_its_wrong_laws(name, order):
    """At the run's sample count some statistic of the run has the noncentrality to bring every listed
    wrong law's p-value below REJECT_P, six standard deviations out."""
    case = law.CASES[name]
    laws = law.laws_of(name, order)
    assert set(laws[None].probs) == set(law.stat_names(case))
    for stats in laws.values():
        for p in stats.probs.values():
            assert abs(p.sum() - 1.0) <= 1e-12 and p.min() >= 0.0
    for rule in case["laws"][order]:
        bounds = law.power(case, laws[None], laws[rule])
        assert min(bounds.values()) <= law.REJECT_P, (name, order, rule, bounds)


def test_every_wrong_law_is_applied_on_the_device():
    for order in ORDERS:
        applied = set("".join(case["laws"][order] for case in law.CASES.values()))
        assert applied == set(law.WRONG_LAWS)
    # the shapes the device tests are asked for
    pairs, hairpin, embedded = (law.CASES[k] for k in ("pairs", "hairpin", "embedded"))
    assert pairs["groups"] * 2 == 1 << 18 and hairpin["groups"] * 4 == 1 << 18 and embedded["groups"] * 4 == 1 << 15
    assert sum(step[0] == "exchange" for step in pairs["steps"]) >= 4
    draws = [step[2] for step in hairpin["steps"] if step[0] == "cluster"]
    assert 1 in draws and hairpin["betas"][0] == hairpin["betas"][3] and hairpin["betas"][1] == hairpin["betas"][2]
    assert embedded["betas"][0] == embedded["betas"][3] != embedded["betas"][1] == embedded["betas"][2]
    assert min(embedded["betas"]) >= sa_exact_law.EMBED_LADDER.min()       # the filler stays frozen


# ----------------------------------------------------------------------------
# the harness end to end on the numpy sampler
# ----------------------------------------------------------------------------

SAMPLER_N = {"pairs": 1 << 13, "hairpin": 1 << 13, "embedded": 1 << 11}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(law.CASES))
def test_the_sampler_follows_the_true_law_and_rejects_the_wrong_ones(name, order, capsys):
    """The run's shape at a reduced N through assert_case: the true process passes; every wrong law
    whose power bound holds at the reduced N too is rejected -- B among them in every case, E and F
    wherever a cluster move is made."""
    case = law.CASES[name]
    N = SAMPLER_N[name]
    true = law.exact_cached(name, order)
    laws = {None: true}
    for rule in case["laws"][order]:
        wrong = law.exact_cached(name, order, rule)
        if min(law.power(case, true, wrong, N).values()) <= law.REJECT_P:
            laws[rule] = wrong
    assert set("BEF") & set(case["laws"][order]) <= set(laws)
    rng = np.random.default_rng([20261020, sorted(law.CASES).index(name), ORDERS.index(order)])
    configs, reports, accepted = law.sample(case, order, N, rng)

    def report(line):
        with capsys.disabled():
            print("\n" + line)

    law.assert_case("numpy sampler %s %s N=%d" % (name, order, N), case, laws, configs, reports, accepted,
                    report=report)


@pytest.mark.parametrize("rule", ["B", "E", "F", "H", "I"])
def test_a_wrong_sampler_follows_its_own_law_and_fails_the_true_one(rule):
    """The sampler run under one changed rule: its counts pass that rule's exact law and assert_case
    refuses them as the true process."""
    name, order, N = "hairpin", "shuffled", 1 << 13
    case = law.CASES[name]
    rng = np.random.default_rng([7, ord(rule)])
    configs, reports, accepted = law.sample(case, order, N, rng, rule)
    observed = law.counts(case, configs, reports)
    own = law.pvalues(observed, law.exact_cached(name, order, rule))
    # (a wrong move reports what it flipped: E and F are compared with the law of that report)
    assert min(own.values()) >= law.PASS_P
    with pytest.raises(AssertionError):
        law.assert_case("wrong sampler", case, {None: law.exact_cached(name, order)}, configs, reports,
                        accepted, report=lambda line: None)
