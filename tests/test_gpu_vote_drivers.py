"""The drivers' consensus selection (common.solve_ising_model / solve_ising_models with
select="consensus"; law ASP-VOTE-1) on three small planted models: equal to
anneal_batch(only_best=False) followed by the numpy restatement and the projection on the frozen spins,
the single-model entry point the same, and select="best" the call without the keyword."""
import numpy as np
import pytest

import vote_cases

pytestmark = pytest.mark.gpu

SIZES = (70, 200, 330)
ARGUMENTS = dict(seed=31, number_sweeps=60, repetitions=16, sweep_order="shuffled")


@pytest.fixture(scope="module")
def models():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, synthetic

    out, frozen = [], []
    for k, size in enumerate(SIZES):
        J, h, _ = synthetic.planted_cluster(size, seed=70 + k)
        if k == 1:  # a model with a field: the vote does not align its chains
            h = np.zeros(size)
            h[::7] = 0.01
        spins = np.arange(size, dtype=np.uint64) * 3 + 1
        out.append(common.IsingModel(spins, None, sa.Hamiltonian(J, h), None))
        frozen.append(spins[np.sort(np.random.default_rng(k).choice(size, size=size // 2, replace=False))])
    yield out, frozen
    for m in out:
        m.ising_hamiltonian.release()


def _expected(models, frozen):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common

    chains = sa.anneal_batch([m.ising_hamiltonian for m in models], only_best=False, **ARGUMENTS)
    out = []
    for m, (xs, es), f in zip(models, chains, frozen):
        law = vote_cases.vote_law(m.size, xs, None, None, int(np.argmin(es)), not np.any(m.ising_hamiltonian.field), 1)
        out.append(common._project_on_frozen(m, law["x"], f))
    return out


def test_consensus_selection_is_the_law_on_the_chains_of_the_batch(models):
    from annealing_sign_problem_amd import common

    models, frozen = models
    want = _expected(models, frozen)
    got = common.solve_ising_models(models, frozen, select="consensus", **ARGUMENTS)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # without frozen spins: the consensus itself
    whole = common.solve_ising_models(models, select="consensus", **ARGUMENTS)
    for m, x, w in zip(models, whole, _expected(models, [None] * 3)):
        assert x.shape == ((m.size + 63) // 64,) and np.array_equal(x, w)
    # the single-model entry point
    for m, f, w in zip(models, frozen, want):
        assert np.array_equal(common.solve_ising_model(m, frozen_spins=f, select="consensus", **ARGUMENTS), w)


def test_best_selection_is_the_call_without_the_keyword(models):
    from annealing_sign_problem_amd import common

    models, frozen = models
    plain = common.solve_ising_models(models, frozen, **ARGUMENTS)
    best = common.solve_ising_models(models, frozen, select="best", **ARGUMENTS)
    voted = common.solve_ising_models(models, frozen, select="consensus", **ARGUMENTS)
    for p, b in zip(plain, best):
        assert np.array_equal(p, b)
    assert len(voted) == len(plain)
    one = common.solve_ising_model(models[0], frozen_spins=frozen[0], **ARGUMENTS)
    assert np.array_equal(one, common.solve_ising_model(models[0], frozen_spins=frozen[0], select="best", **ARGUMENTS))
    assert np.array_equal(one, plain[0])
