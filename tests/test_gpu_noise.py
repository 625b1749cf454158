"""The noise study (annealing_sign_problem_amd/influence_of_noise.py) on the GPU: its
rows do not depend on batching or on plan re-use, the re-use leg builds one plan however many draws it
solves, and reweight_ising_model returns make_ising_model's model — also when an amplitude vanishes,
the pattern changes and the fallback runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ring(n):
    from annealing_sign_problem_amd import operators

    matrix = [[1, 0, 0, 0], [0, -1, 2, 0], [0, 2, -1, 0], [0, 0, 0, 1]]
    config = {"basis": {"number_spins": n, "hamming_weight": n // 2, "symmetries": []},
              "hamiltonian": {"terms": [{"matrix": matrix, "sites": [[i, (i + 1) % n] for i in range(n)]}]}}
    operator = operators.Operator.from_config(config)
    operator.basis.build()
    _, ground_state = operator.ground_state()
    return operator, ground_state


def _build_count():
    from annealing_sign_problem_amd import _lib

    return _lib.load().asp_sa_layout_build_count()


def _rows(operator, ground_state, levels, repetitions, **how):
    from annealing_sign_problem_amd.influence_of_noise import influence_of_noise

    return ["{},{},{}\n".format(*row).encode()
            for row in influence_of_noise(operator, ground_state, levels, repetitions, seed=435834, **how)]


def test_rows_do_not_depend_on_batch_or_reuse():
    operator, ground_state = _ring(10)
    assert operator.basis.number_states == 252
    levels = np.exp(np.linspace(np.log(1e-2), np.log(1e2), 3))
    fresh = _rows(operator, ground_state, levels, 3, reuse=False)
    assert len(fresh) == 9 and len(set(fresh)) == 9
    builds = _build_count()
    assert _rows(operator, ground_state, levels, 3, reuse=True, batch=4) == fresh
    assert _build_count() - builds == 1
    assert _rows(operator, ground_state, levels, 3, reuse=True, batch=1) == fresh
    assert _build_count() - builds == 2


def test_kagome_16_builds_one_plan():
    from annealing_sign_problem_amd import operators, synthetic

    operator = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_16"])
    operator.basis.build()
    _, ground_state = operator.ground_state()
    assert operator.basis.number_states == 12870
    batch = 4
    builds = _build_count()
    reused = _rows(operator, ground_state, [0.01, 100.0], 2, reuse=True, batch=batch)
    assert _build_count() - builds <= batch + 1
    assert reused == _rows(operator, ground_state, [0.01, 100.0], 2, reuse=False)


def test_reweight_ising_model_equals_make_ising_model():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common

    operator, ground_state = _ring(10)
    basis = operator.basis
    base = common.make_ising_model(basis.states, operator,
                                   log_psi_fn=common.ground_state_to_log_coeff_fn(ground_state, basis))
    base.ising_hamiltonian.plan()  # (the one build; the first clone would ask for it otherwise)
    np.random.seed(7)
    pooled = None
    for draw in range(4):
        noisy = common.add_noise_to_amplitudes(ground_state, eps=1.0)
        if draw == 3:
            noisy[17] = 0.0  # a state without amplitude: its couplings vanish, the pattern changes
        with np.errstate(divide="ignore"):
            log_psi_fn = common.ground_state_to_log_coeff_fn(noisy, basis)
            want = common.make_ising_model(basis.states, operator, log_psi_fn=log_psi_fn)
            builds = _build_count()
            got = common.reweight_ising_model(base, log_psi_fn=log_psi_fn, out=pooled)
        if draw < 3:
            assert _build_count() == builds
            assert np.shares_memory(got.ising_hamiltonian.exchange.indices, base.ising_hamiltonian.exchange.indices)
            assert not got.ising_hamiltonian.exchange.data.flags.writeable
            pooled = got  # (the first call clones; the later ones reweight that clone in place)
        else:
            assert got is not pooled and got.ising_hamiltonian is not pooled.ising_hamiltonian
            assert got.ising_hamiltonian.exchange.nnz < base.ising_hamiltonian.exchange.nnz
        for a, b in ((got.ising_hamiltonian.exchange, want.ising_hamiltonian.exchange),):
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            assert np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64))
        assert np.array_equal(got.ising_hamiltonian.field, want.ising_hamiltonian.field)
        assert np.array_equal(got.initial_signs, want.initial_signs)
        assert np.array_equal(got.spins, want.spins)
        x_got, e_got = sa.greedy_solve(got.ising_hamiltonian)
        x_want, e_want = sa.greedy_solve(want.ising_hamiltonian)
        assert np.array_equal(x_got, x_want) and e_got == e_want
