"""CPU: the oracle's chains against the exact Markov law of ASP-SA-1 / ASP-SA-1S (DESIGN.md §4,
§4.9), computed independently of oracle/sa_oracle.c by tests/sa_exact_law.py on two tiny
systems.  Bit-for-bit parity with the oracle shows that the kernels compute what the oracle
computes; these tests show that what both compute is the specified Metropolis chain, and that
each of sa_exact_law.WRONG_LAWS would have been noticed."""
import numpy as np
import pytest
import scipy.sparse

import oracle
import sa_exact_law as law

REPS = 1 << 18
SCALE_EXP = 40          # dE is a multiple of 1/4 here: every tracked q is exact
SEED = 0x9E3779B97F4A7C15 % (1 << 40) + (1 << 33)   # >= 2**32: both Philox key words in use
THREADS = 16

SYSTEMS = {"P1": law.system_p1, "P2": law.system_p2}


def _setup(name):
    J, h = SYSTEMS[name]()
    n = h.shape[0]
    members = np.arange(n)
    Jc = scipy.sparse.csr_matrix(J)
    return Jc, h, law.energies(J, h), members, law.colour_order(Jc, members)


def _words(x0):
    return None if x0 is None else np.array([x0], dtype=np.uint64)


def _report(capsys):
    def report(line):
        with capsys.disabled():
            print("\n" + line)
    return report


@pytest.mark.parametrize("name", ["P1", "P2"])
@pytest.mark.parametrize("order", ["colour", "shuffled"])
@pytest.mark.parametrize("start", ["uniform", "x0"])
def test_oracle_chains_follow_the_exact_law(name, order, start, capsys):
    """oracle.sa_anneal / sa_anneal_shuffled from the uniform start and from a low-lying x0: the
    law of the returned configuration, exact returned energies, the mean accepted flips; every
    applicable wrong law rejected."""
    Jc, h, E, members, colour = _setup(name)
    x0 = law.X0[name] if start == "x0" else None
    betas = law.LADDER
    if order == "shuffled":
        orders = law.shuffled_orders(SEED, betas.shape[0], members)
        run = oracle.sa_anneal_shuffled
    else:
        orders = [colour] * betas.shape[0]
        run = oracle.sa_anneal
    xs, es, _, accepted = run(Jc, h, SEED, betas, REPS, 0, _words(x0), SCALE_EXP,
                              num_threads=THREADS)
    configs = law.local_configs(xs, members)
    assert np.array_equal(es, E[configs])
    laws = law.laws_for(E, betas, orders, colour, x0, shuffled=order == "shuffled")
    law.assert_law("%s %s %s" % (name, order, start), E, laws, configs, accepted,
                   report=_report(capsys))


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_oracle_trace_follows_the_exact_law(name, capsys):
    """oracle.sa_anneal_trace from a point mass at x0: the returned configuration, and the
    current energy after sweeps 1, 3 (beta = 0), 6 (beta = +inf) and 11 against their exact laws;
    every wrong law rejected."""
    Jc, h, E, members, colour = _setup(name)
    betas = law.LADDER
    x0 = law.X0[name]
    xs, es, trace = oracle.sa_anneal_trace(Jc, h, SEED, betas, REPS, 0, _words(x0), SCALE_EXP,
                                           num_threads=THREADS)
    configs = law.local_configs(xs, members)
    assert np.array_equal(es, E[configs])
    assert np.all(trace[:, 0] == 0)
    current = {t: E[x0] + np.ldexp(trace[:, t].astype(np.float64), -SCALE_EXP)
               for t in (1, 3, 6, 11)}
    laws = law.laws_for(E, betas, [colour] * betas.shape[0], colour, x0=x0)
    law.assert_law("%s trace" % name, E, laws, configs, current_energies=current,
                   report=_report(capsys))


def test_exact_law_is_a_distribution():
    """Sanity of the reference itself: every law sums to one, the beta = 0 sweep flips every
    spin, and a point mass at the ground state with only beta = +inf sweeps stays there."""
    _, _, E, members, colour = _setup("P1")
    laws = law.laws_for(E, law.LADDER, [colour] * law.LADDER.shape[0], colour)
    for lw in laws.values():
        assert abs(lw.best.sum() - 1) < 1e-12
        assert all(abs(c.sum() - 1) < 1e-12 for c in lw.current.values())
    # sweep 3 runs at beta = 0: every proposal accepted, every spin flipped once
    true = laws[None]
    assert np.allclose(true.current[3], true.current[2][np.arange(128) ^ 127], atol=1e-15)
    ground = int(np.argmin(E))
    frozen = law.propagate(E, [np.inf] * 4, [colour] * 4, x0=ground)
    assert frozen.best[ground] == 1.0 and frozen.current[4][ground] == 1.0
