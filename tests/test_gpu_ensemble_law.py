"""GPU: ladder sweeps, replica exchange and isoenergetic cluster moves (§4.13) composed
on the device, against the exact joint law of tests/ensemble_exact_law.py -- independent of the kernels, of
the oracle and of the two restated laws (tests/tempering_law.py, tests/cluster_move_law.py).

One handle holds R/G independent groups of G slots (``ensemble_exact_law.CASES``): exchange with parity 0
and cluster pairs stay inside a group, every group starts from the same point masses, and the groups'
final configurations, the swaps of every exchange step and the (differing, size) pairs that every cluster
move reports are compared with their exact laws.  Every run must follow the true law and reject the wrong
laws of its case (tests/test_ensemble_law.py proves without a device that it can); after every step of
every run the bookkeeping must hold exactly, since all inputs are dyadic.  The last test runs the loop of
``parallel_tempering_cluster`` on an odd number of slots from the exact Boltzmann law, which must stay
invariant.  No limit on the slots or pairs of a call was met: every run uses one handle of the planned R."""
import numpy as np
import pytest
import scipy.sparse

import ensemble_exact_law as law

pytestmark = pytest.mark.gpu

STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def _report(capsys):
    def report(line):
        with capsys.disabled():
            print("\n" + line)
    return report


class _Target:
    """A system on the device: its Hamiltonian, the members' bit positions, the words every chain shares
    outside the members (``base``) and the energy of that part."""

    def __init__(self, name):
        from annealing_sign_problem_amd import annealer as sa

        self.sys = law.system(name)
        self.members = self.sys.members
        if name == "Q":
            J, h = law.system_q()
            self.ham = sa.Hamiltonian(scipy.sparse.csr_matrix(J), h)
            self.base = np.zeros(1, dtype=np.uint64)
            self.offset = 0.0
        else:
            J, h, x0, filler_energy = law.embedded_system()
            self.ham = sa.Hamiltonian(J, h)
            self.base, self.offset = x0.copy(), filler_energy
            # the filler is frozen at every beta of the run, as embedded_system asserts for its own ladder
            A = (J + J.T).tocsr()
            A.setdiag(0)
            sites = np.arange(h.shape[0])
            bits = ((x0[sites // 64] >> (sites % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
            de = np.where(bits, -2.0, 2.0) * (A @ np.where(bits, 1.0, -1.0) + h)
            filler = np.ones(h.shape[0], dtype=bool)
            filler[self.members] = False
            assert np.min(de[filler]) * min(law.CASES["embedded"]["betas"]) >= 23.0
        self.mask = np.zeros_like(self.base)
        for g in self.members:
            self.mask[g // 64] |= np.uint64(1) << np.uint64(g % 64)
        self.base &= ~self.mask
        self.S = self.ham.info().energy_scale_exp

    def words(self, config):
        x = self.base.copy()
        for i, g in enumerate(self.members):
            if (int(config) >> i) & 1:
                x[g // 64] |= np.uint64(1) << np.uint64(g % 64)
        return x

    def configs(self, xs):
        """Local configurations of packed rows; every bit outside the members must be the shared one."""
        assert np.array_equal(xs & ~self.mask, np.broadcast_to(self.base, xs.shape)), "a filler spin moved"
        return law.local_configs(xs, self.members)

    def check_bookkeeping(self, state):
        """(tracked_best - tracked_current) 2^-S = E(x_best) - E(x_current), exactly, for every chain;
        returns the current configurations."""
        current, best = self.configs(state["x_current"]), self.configs(state["x_best"])
        want = np.ldexp(self.sys.E[best] - self.sys.E[current], self.S)
        assert np.array_equal((state["tracked_best"] - state["tracked_current"]).astype(np.float64), want), \
            "the tracked energies drifted from the configurations"
        return current


def _run(name, order, capsys):
    """One case of ensemble_exact_law.CASES on the device, every step checked, then assert_case."""
    from annealing_sign_problem_amd import annealer as sa

    case = law.CASES[name]
    target = _Target(case["system"])
    E = target.sys.E
    G, N = len(case["betas"]), case["groups"]
    R = G * N
    betas = np.tile(np.asarray(case["betas"], dtype=np.float64), N)
    x0 = np.tile(np.stack([target.words(c) for c in case["starts"]]), (N, 1))
    first = np.arange(0, R, G)
    reports, accepted = {}, []
    with sa.Chains(target.ham, seed=law.SEED, repetitions=R, x0=x0) as chains:
        state = chains.state()
        current = target.check_bookkeeping(state)
        assert np.array_equal(current, np.tile(case["starts"], N))
        for k, step in enumerate(case["steps"]):
            if step[0] == "forget":
                continue
            if step[0] == "sweep":
                chains.advance_ladder(betas, step[1], sweep_order=order)
                after = chains.state()
            elif step[0] == "exchange":
                source, energies, count = chains.exchange(betas, 0, step[1])
                after = chains.state()
                assert np.array_equal(energies, target.offset + E[current]), "the exchange read another energy"
                swapped = source[0::2] != np.arange(0, R, 2)
                want = np.arange(R).reshape(-1, 2)
                want[swapped] = want[swapped][:, ::-1]
                assert np.array_equal(source, want.ravel()) and count == int(swapped.sum())
                for key in STATE:       # all five arrays move together
                    assert np.array_equal(after[key], state[key][source]), key
                accepted.append(swapped.reshape(N, G // 2).sum(axis=1))
            else:
                local = np.asarray(step[1])
                pairs = (first[:, None, None] + local[None]).reshape(-1, 2)
                differing, sizes, deltas = chains.cluster_move(pairs, step[2])
                after = chains.state()
                a, b = pairs[:, 0], pairs[:, 1]
                moved = target.configs(after["x_current"])
                C = moved[a] ^ current[a]
                D = current[a] ^ current[b]
                assert np.array_equal(moved[b] ^ current[b], C) and not np.any(C & ~D)
                assert np.array_equal(differing, law._popcount(D)) and np.array_equal(sizes, law._popcount(C))
                assert np.all((sizes > 0) == (differing > 0))
                # deltas: exactly the energy change of chain a in units of 2^-S, and the tracked energies follow
                assert np.array_equal(deltas.astype(np.float64), np.ldexp(E[moved[a]] - E[current[a]], target.S))
                assert np.array_equal(after["tracked_current"][a] - state["tracked_current"][a], deltas)
                assert np.array_equal(after["tracked_current"][b] - state["tracked_current"][b], -deltas)
                assert np.array_equal(after["accepted"], state["accepted"])
                reports[k] = (differing.reshape(N, -1), sizes.reshape(N, -1))
            state = after
            current = target.check_bookkeeping(state)
        assert np.array_equal(target.ham.energies(state["x_current"]), target.offset + E[current]), \
            "inexact energy of a current configuration"
        assert np.array_equal(chains.result()[1], target.offset + E[target.configs(state["x_best"])])
    law.assert_case("gpu ensemble %s %s" % (name, order), case, law.laws_of(name, order),
                    current.reshape(N, G), reports, np.array(accepted), report=_report(capsys))


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_exchange_pairs_follow_the_exact_joint_law(order, capsys):
    """System Q, 2^17 pairs of slots at (0.3, 1.5) in one handle, five rounds of ladder sweeps and
    exchange with parity 0 (one of them twice at one sweep count, draws 0 and 1): the pair's joint law
    (1024 cells), both marginals and the swaps of every step.  Rejects A, B, C, D and I."""
    _run("pairs", order, capsys)


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_hairpin_groups_with_cluster_moves_follow_the_exact_joint_law(order, capsys):
    """System Q, 2^16 groups of four slots at (b0, b1, b1, b0): rounds of ladder sweeps, cluster moves of
    (4g, 4g+3) and (4g+1, 4g+2) and exchange with parity 0, a first move before any sweep and one round
    with two moves at one sweep count (draws 0 and 1): four marginals, six pair joints, the reported
    (differing, size) of all twelve moves, the swaps of every step.  Rejects every wrong law A-I."""
    _run("hairpin", order, capsys)


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_embedded_multi_word_groups_follow_the_exact_law(order, capsys):
    """P1 at EMBED_AT (words 0, 1, 63 and beyond) of the 20 000-spin frozen filler, 2^15 slots in groups
    of four at (0.25, 1.5, 1.5, 0.25): exchange rounds inside (4g, 4g+1) and (4g+2, 4g+3), then one
    cluster move of the equal-beta pairs (4g, 4g+3) and (4g+1, 4g+2) and a last sweep.  The filler bits of
    x_current and x_best never move; P1's four marginals, the reported (differing, size) and the swaps
    follow the exact law.  Rejects every wrong law A-I."""
    _run("embedded", order, capsys)


def test_the_coupled_ensemble_keeps_the_boltzmann_law_invariant(capsys):
    """System Q on 2^16 + 1 slots (odd: the last slot has no partner at parity 0 and slot 0 none at
    parity 1), slot k at one of three betas by k mod 3, every start drawn on the host from the exact
    Boltzmann law of its slot, then the loop of parallel_tempering_cluster verbatim: ladder sweeps,
    cluster moves of equal-beta pairs, exchange with parity j & 1.  With beta dE < 23 and |dbeta dE| < 23
    throughout nothing is cut off, the product measure is exactly invariant, the slots stay independent
    and the pooled chi-square of each beta class is exact.  The 2^-32 granularity of u and expneg's 4e-16
    relative error move a probability by less than 1e-9, which 2 10^4 slots per class cannot resolve.

    What this run cannot see: an omitted move (no exchange, no cluster move) and the cluster move that
    flips all differing sites (law F, a swap of the two replicas) keep the product measure too.  The
    joint-law runs above are what cover those."""
    from annealing_sign_problem_amd import annealer as sa

    target = _Target("Q")
    E = target.sys.E
    R = (1 << 16) + 1
    betas, pairs = law.invariance_plan(R)
    rng = np.random.default_rng(20261020)
    start = np.zeros(R, dtype=np.int64)
    for beta in law.INVARIANCE_BETAS:
        where = betas == beta
        start[where] = rng.choice(E.shape[0], size=int(where.sum()), p=law.boltzmann(E, beta))
    x0 = start.astype(np.uint64).reshape(R, 1)
    swaps = []
    with sa.Chains(target.ham, seed=law.SEED + 1, repetitions=R, x0=x0) as chains:
        for j in range(law.INVARIANCE_ROUNDS):
            chains.advance_ladder(betas, law.INVARIANCE_SWEEPS, sweep_order="shuffled")
            chains.cluster_move(pairs, 0)
            if j + 1 < law.INVARIANCE_ROUNDS:
                source, _, count = chains.exchange(betas, j & 1, 0)
                assert source[R - 1 if j & 1 == 0 else 0] == (R - 1 if j & 1 == 0 else 0)
                swaps.append(count)
        state = chains.state()
        current = target.check_bookkeeping(state)
        assert np.array_equal(target.ham.energies(state["x_current"]), E[current])
    ps = {}
    for beta in law.INVARIANCE_BETAS:
        counts = np.bincount(current[betas == beta], minlength=E.shape[0])
        ps[beta] = law.chi2_pvalue(counts, law.boltzmann(E, beta))
    line = "gpu ensemble invariance: %s; swaps per exchange step %s of %d pairs" % (
        ", ".join("beta %.2f p = %.3g" % (beta, p) for beta, p in ps.items()), swaps, R // 2)
    _report(capsys)(line)
    assert min(ps.values()) >= law.PASS_P, line
    assert all(0 < s < R // 2 for s in swaps), line
