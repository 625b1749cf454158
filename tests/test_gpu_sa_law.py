"""GPU: the annealing kernels against the exact Markov law of ASP-SA-1 / ASP-SA-1S (DESIGN.md §4,
§4.9), computed by tests/sa_exact_law.py independently of the kernels and of the oracle.

Standalone: the tiny systems P1 and P2 through anneal_raw (both orders), anneal_trace_raw and
anneal_batch_raw (both orders), 2^20 chains each -- replica ids far beyond those of the parity
tests.  Embedded: P1 at scattered global ids (63, 64 and 127 among them) of a 20 000-spin frozen
filler, so that the layouts, launch shapes and order builds of production sizes run it.  Every
run must follow the true law, return exact energies and reject every applicable wrong law."""
import numpy as np
import pytest
import scipy.sparse

import sa_exact_law as law

pytestmark = pytest.mark.gpu

REPS = 1 << 20
EMBED_REPS = 1 << 16
SEED = (1 << 40) + 0x5DEECE66D      # >= 2**32: both Philox key words in use
SYSTEMS = {"P1": law.system_p1, "P2": law.system_p2}


def _report(capsys):
    def report(line):
        with capsys.disabled():
            print("\n" + line)
    return report


def _stats(ham, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(ham.plan(), count, _lib.ptr(tracked),
                                             _lib.ptr(accepted)))
    return tracked, accepted


def _words(x0):
    return None if x0 is None else np.array([x0], dtype=np.uint64)


class _Tiny:
    def __init__(self, name):
        from annealing_sign_problem_amd import annealer as sa

        J, h = SYSTEMS[name]()
        self.name = name
        self.members = np.arange(h.shape[0])
        self.J = scipy.sparse.csr_matrix(J)
        self.E = law.energies(J, h)
        self.colour = law.colour_order(self.J, self.members)
        self.ham = sa.Hamiltonian(self.J, h)


_embedded = {}


def _embedded_system():
    if "system" not in _embedded:
        J, h, x0, filler_energy = law.embedded_system()
        Jp, hp = law.system_p1()
        mask = np.zeros_like(x0)
        for g in law.EMBED_AT:
            mask[g // 64] |= np.uint64(1) << np.uint64(g % 64)
        _embedded["system"] = dict(J=J, h=h, x0=x0, filler_energy=filler_energy, mask=mask,
                                   E=law.energies(Jp, hp),
                                   colour=law.colour_order(J, law.EMBED_AT))
    return _embedded["system"]


def _check_embedded(label, xs, es, accepted, laws, filler_bits, capsys):
    """The filler bits come back as ``filler_bits`` in every chain, the energies are exact, and
    P1's returned configurations follow laws[None] and reject every other law."""
    s = _embedded_system()
    keep = ~s["mask"]
    assert np.array_equal(xs & keep, np.broadcast_to(filler_bits & keep, xs.shape)), \
        "a filler spin moved"
    configs = law.local_configs(xs, law.EMBED_AT)
    assert np.array_equal(es, s["filler_energy"] + s["E"][configs]), "inexact returned energy"
    law.assert_law(label, s["E"], laws, configs, accepted, report=_report(capsys))


@pytest.mark.parametrize("name", ["P1", "P2"])
@pytest.mark.parametrize("order", ["colour", "shuffled"])
@pytest.mark.parametrize("start", ["uniform", "x0"])
def test_anneal_raw_follows_the_exact_law(name, order, start, capsys):
    """anneal_raw, 2^20 chains from the uniform start and from a low-lying x0: returned law,
    exact energies, accepted flips per chain; every applicable wrong law rejected."""
    from annealing_sign_problem_amd import annealer as sa

    p = _Tiny(name)
    x0 = law.X0[name] if start == "x0" else None
    shuffled = order == "shuffled"
    betas = law.LADDER
    xs, es = sa.anneal_raw(p.ham, SEED, betas, REPS, 0, _words(x0), shuffled=shuffled)
    _, accepted = _stats(p.ham, REPS)
    configs = law.local_configs(xs, p.members)
    assert np.array_equal(es, p.E[configs]), "inexact returned energy"
    orders = (law.shuffled_orders(SEED, betas.shape[0], p.members) if shuffled
              else [p.colour] * betas.shape[0])
    laws = law.laws_for(p.E, betas, orders, p.colour, x0, shuffled=shuffled)
    law.assert_law("gpu %s %s %s" % (name, order, start), p.E, laws, configs, accepted,
                   report=_report(capsys))


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_anneal_trace_raw_follows_the_exact_law(name, capsys):
    """anneal_trace_raw, 2^20 chains from x0: the returned configuration and the current energy
    after sweeps 1, 3 (beta = 0), 6 (beta = +inf) and 11; every wrong law rejected."""
    from annealing_sign_problem_amd import annealer as sa

    p = _Tiny(name)
    x0 = law.X0[name]
    betas = law.LADDER
    xs, es, trace = sa.anneal_trace_raw(p.ham, SEED, betas, REPS, 0, _words(x0))
    S = p.ham.info().energy_scale_exp
    configs = law.local_configs(xs, p.members)
    assert np.array_equal(es, p.E[configs]), "inexact returned energy"
    assert np.all(trace[:, 0] == 0)
    current = {t: p.E[x0] + np.ldexp(trace[:, t].astype(np.float64), -S) for t in (1, 3, 6, 11)}
    laws = law.laws_for(p.E, betas, [p.colour] * betas.shape[0], p.colour, x0=x0)
    law.assert_law("gpu %s trace" % name, p.E, laws, configs, current_energies=current,
                   report=_report(capsys))


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_anneal_batch_raw_follows_the_exact_law(order, capsys):
    """P1 and P2 (2^20 chains each) and the embedded P1 (2^16 chains) in ONE anneal_batch_raw
    call.  A batch has no x0, so the embedded filler starts uniform: its misaligned spins all
    flip in sweep 0 (dE <= -1000), it is aligned from then on, and its start energy exceeds that
    of every sweep end -- P1's law there is the uniform start with the start never a best
    candidate (law "d")."""
    from annealing_sign_problem_amd import annealer as sa

    shuffled = order == "shuffled"
    tiny = [_Tiny("P1"), _Tiny("P2")]
    s = _embedded_system()
    embedded = sa.Hamiltonian(s["J"], s["h"])
    hams = [t.ham for t in tiny] + [embedded]
    ladders = [law.LADDER, law.LADDER, law.EMBED_LADDER]
    reps = [REPS, REPS, EMBED_REPS]
    results = sa.anneal_batch_raw(hams, [SEED] * 3, ladders, reps, shuffled=shuffled)
    stats = [_stats(h, r) for h, r in zip(hams, reps)]
    for p, (xs, es), (_, accepted) in zip(tiny, results[:2], stats[:2]):
        configs = law.local_configs(xs, p.members)
        assert np.array_equal(es, p.E[configs]), "inexact returned energy"
        orders = (law.shuffled_orders(SEED, law.LADDER.shape[0], p.members) if shuffled
                  else [p.colour] * law.LADDER.shape[0])
        laws = law.laws_for(p.E, law.LADDER, orders, p.colour, shuffled=shuffled)
        law.assert_law("gpu batch %s %s" % (order, p.name), p.E, laws, configs, accepted,
                       report=_report(capsys))
    T = law.EMBED_LADDER.shape[0]
    orders = (law.shuffled_orders(SEED, T, law.EMBED_AT) if shuffled else [s["colour"]] * T)
    true = law.propagate(s["E"], law.EMBED_LADDER, orders, None, rule="d")
    # the filler's accepted flips of sweep 0 are counted too: P1's share is not separable here
    xs, es = results[2]
    _check_embedded("gpu batch %s embedded P1" % order, xs, es, None, {None: true}, s["x0"],
                    capsys)


@pytest.mark.parametrize("m", [1, 4, 8])
def test_embedded_colour_order_follows_the_exact_law(m, capsys):
    """P1 inside the 20 000-spin frozen filler, colour order, the launch forced to m chains per
    group with the byte layout (asp_sa_set_wide(0)): 2^16 chains from x0."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    s = _embedded_system()
    ham = sa.Hamiltonian(s["J"], s["h"])
    lib = _lib.load()
    _lib.check(lib.asp_sa_set_launch(ham.plan(), m, 0))
    _lib.check(lib.asp_sa_set_wide(ham.plan(), 0))
    betas = law.EMBED_LADDER
    xs, es = sa.anneal_raw(ham, SEED, betas, EMBED_REPS, 0, s["x0"])
    _, accepted = _stats(ham, EMBED_REPS)
    laws = law.laws_for(s["E"], betas, [s["colour"]] * betas.shape[0], s["colour"], law.X0["P1"])
    _check_embedded("gpu embedded colour m=%d" % m, xs, es, accepted, laws, s["x0"], capsys)


def test_embedded_shuffled_order_follows_the_exact_law(capsys):
    """P1 inside the 20 000-spin frozen filler, the default (shuffled) order and launch: 2^16
    chains from x0."""
    from annealing_sign_problem_amd import annealer as sa

    s = _embedded_system()
    ham = sa.Hamiltonian(s["J"], s["h"])
    betas = law.EMBED_LADDER
    xs, es = sa.anneal_raw(ham, SEED, betas, EMBED_REPS, 0, s["x0"], shuffled=True)
    _, accepted = _stats(ham, EMBED_REPS)
    orders = law.shuffled_orders(SEED, betas.shape[0], law.EMBED_AT)
    laws = law.laws_for(s["E"], betas, orders, s["colour"], law.X0["P1"], shuffled=True)
    _check_embedded("gpu embedded shuffled", xs, es, accepted, laws, s["x0"], capsys)
