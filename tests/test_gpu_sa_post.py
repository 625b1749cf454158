"""The pass after the sweeps — reported energies and unpermuted configurations from one kernel
(k_sa_post, DESIGN.md §5.2 "Afterwards") — against the CPU oracle and against the older energy and
unpermute kernels (asp_sa_set_post(plan, 0)), bit for bit, on the clusters of tests/sa_post_cases.py
(whose structure tests/test_sa_post_cases.py asserts): a single spin, dummy lanes, one and two blocks,
blocks of 0 to 5 quads, a partial-sum tree of two levels; 1 and 7 configurations (the older kernels on
both sides), 8 and 64 (whole groups of four), 9 and 11 (last groups of one and three)."""
import numpy as np
import pytest

import oracle
import sa_post_cases as cases

pytestmark = pytest.mark.gpu


class _Reference:
    """A cluster, its configurations, schedule and the oracle's results: computed once, never changed."""

    def __init__(self, name):
        from annealing_sign_problem_amd import annealer as sa

        self.J, self.field = cases.CASES[name]()
        self.n = self.J.shape[0]
        self.xs = cases.configurations(self.n, max(cases.COUNTS))
        self.energies = oracle.sa_energy(self.J, self.field, self.xs)
        ham = sa.Hamiltonian(self.J, self.field)
        info = ham.info()
        self.S = info.energy_scale_exp
        self.betas = sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), cases.SWEEPS)
        ham.release()
        for a in (self.xs, self.energies, self.betas):
            a.setflags(write=False)
        self._chains = {}

    def chains(self, count):
        if count not in self._chains:
            out = oracle.sa_anneal(self.J, self.field, 99, self.betas, count, 0, None, self.S, num_threads=4)
            for a in out:
                a.setflags(write=False)
            self._chains[count] = out
        return self._chains[count]


_REFERENCES = {}


@pytest.fixture(params=list(cases.CASES))
def ref(request):
    if request.param not in _REFERENCES:
        _REFERENCES[request.param] = _Reference(request.param)
    return _REFERENCES[request.param]


def _hamiltonian(ref, post):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(ref.J, ref.field)
    _lib.check(_lib.load().asp_sa_set_post(ham.plan(), int(post)))
    return ham


@pytest.mark.parametrize("count", cases.COUNTS)
def test_energies(ref, count):
    xs = np.array(ref.xs[:count])
    results = []
    for post in (True, False):
        ham = _hamiltonian(ref, post)
        results.append(ham.energies(xs))
        ham.release()
    new, old = results
    assert new.tobytes() == ref.energies[:count].tobytes(), "energies differ from the oracle"
    assert old.tobytes() == new.tobytes(), "the two passes differ"


@pytest.mark.parametrize("chains", cases.CHAINS)
def test_anneal(ref, chains):
    from annealing_sign_problem_amd import annealer as sa

    oxs, oes, _, _ = ref.chains(chains)
    ham = _hamiltonian(ref, True)
    xs, es = sa.anneal_raw(ham, 99, ref.betas, chains)
    ham.release()
    assert xs.tobytes() == oxs.tobytes(), "annealed configurations differ from the oracle"
    assert es.tobytes() == oes.tobytes(), "energies differ from the oracle"
    ham = _hamiltonian(ref, False)
    old_xs, old_es = sa.anneal_raw(ham, 99, ref.betas, chains)
    ham.release()
    assert old_xs.tobytes() == xs.tobytes() and old_es.tobytes() == es.tobytes(), "the two passes differ"


def test_set_post_rejects_null_plan():
    from annealing_sign_problem_amd import _lib

    assert _lib.load().asp_sa_set_post(None, 1) != 0
