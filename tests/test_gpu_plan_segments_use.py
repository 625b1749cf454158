"""Plans of asp_sa_plan_create_segments in use (law ASP-PLAN-SEG-1): on a round of three
planted clusters of 500, 1000 and 3000 spins and on the value-edge segment every result — anneals in both
orders, the greedy solver with both trees, energies, a clone, a reweight, chains with a cluster move —
equals, bit for bit, the same calls on asp_sa_plan_create plans; plan_hamiltonians leaves planned
Hamiltonians alone; solve_ising_models and the sampled_components driver give the same with and without
the batched plans."""
import numpy as np
import pytest
import scipy.sparse

import plan_cases as pc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _segments():
    return [pc.planted(500, 6.0, seed=11), pc.planted(1000, 8.0, seed=12), pc.planted(3000, 6.0, seed=13),
            pc.value_edge()]


def _hamiltonians(segments):
    from annealing_sign_problem_amd import annealer as sa

    return [sa.Hamiltonian.from_canonical_csr(ip.copy(), ix.copy(), dv.copy(), h.copy()) for ip, ix, dv, h in segments]


@pytest.fixture(scope="module")
def pairs():
    """[(segment, Hamiltonian planned by the segmented call, Hamiltonian planned on its own)], made once."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    segments = _segments()
    batched, single = _hamiltonians(segments), _hamiltonians(segments)
    before = _lib.load().asp_sa_layout_build_count()
    sa.plan_hamiltonians(batched)
    assert _lib.load().asp_sa_layout_build_count() == before + len(segments)
    assert sa.plan_hamiltonians_last_ms() > 0.0
    assert all(h._plan is not None and h._plan_key == h._key() for h in batched)
    for h in single:
        h.plan()
    yield list(zip(segments, batched, single))
    for h in batched + single:
        h.release()


def observe(ham, chains: bool = True):
    """Results of the plan as exactly comparable arrays."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    info = ham.info()
    K = ham.size
    out = {"info": np.frombuffer(bytes(info), dtype=np.uint8).copy()}
    rng = np.random.default_rng(7)
    xs = np.stack([sa.signs_to_bits(rng.choice([-1.0, 1.0], size=K)) for _ in range(8)])
    out["energies"] = _bits(ham.energies(xs))
    # (the value-edge segment's smallest coupling is subnormal: its beta1_auto overflows to inf)
    coldest = info.beta1_auto if np.isfinite(info.beta1_auto) else 100.0 * info.beta0_auto
    betas = sa.make_schedule(info.beta0_auto, coldest, 32)
    for name, shuffled in (("colour", False), ("shuffled", True)):
        x, e = sa.anneal_raw(ham, 3, betas, 64, shuffled=shuffled)
        out[name + "_x"], out[name + "_e"] = np.array(x), _bits(e)
    for tree in ("host", "device"):
        x, e = sa.greedy_solve(ham, tree=tree)
        out["greedy_" + tree + "_x"], out["greedy_" + tree + "_e"] = np.array(x), _bits([e])
    if chains:
        c = sa.Chains(ham, seed=9, repetitions=4)
        try:
            hot = np.full(4, info.beta0_auto)
            out["ladder_trace"] = c.advance_ladder(hot, 3, sweep_order="colour", trace=True)
            out["move"] = np.concatenate([np.asarray(a, dtype=np.int64).ravel() for a in c.cluster_move([(0, 1), (2, 3)])])
            out["segment_trace"] = c.advance(betas[:4], sweep_order="shuffled", trace=True)
            x, e = c.result()
            out["chains_x"], out["chains_e"] = np.array(x), _bits(e)
        finally:
            c.close()
    for name in pc.ARRAYS:
        out["array_" + name] = sa.read_plan_array(ham.plan(), name).view(np.uint8)
    return out


def assert_same(got, expected):
    assert sorted(got) == sorted(expected)
    for name in expected:
        assert np.array_equal(got[name], expected[name]), name


@pytest.mark.parametrize("which", range(4))
def test_results_equal_those_of_asp_sa_plan_create(which, pairs):
    _, batched, single = pairs[which]
    assert_same(observe(batched), observe(single))


@pytest.mark.parametrize("which", [0, 3])
def test_clone_and_reweight_work_on_the_stored_pattern(which, pairs):
    from annealing_sign_problem_amd import _lib

    (ip, ix, dv, h), batched, single = pairs[which]
    clone, clone_single = batched.clone(), single.clone()
    try:
        assert_same(observe(clone, chains=False), observe(clone_single, chains=False))
        # new numbers on the same pattern: the same bits as a plan of its own, without a layout build
        scale = np.random.default_rng(3).uniform(0.5, 2.0, size=dv.size)
        if which == 0:  # (a symmetric matrix stays one: the pairs that cancel keep cancelling either way)
            matrix = scipy.sparse.csr_matrix((scale, ix, ip), shape=(ip.size - 1,) * 2)
            scale = matrix.maximum(matrix.T).tocsr()
            scale.sort_indices()
            scale = scale.data
        else:
            scale = np.full(dv.size, 1.75)
        before = _lib.load().asp_sa_layout_build_count()
        clone.reweight(dv * scale, field=h * 0.5)
        clone_single.reweight(dv * scale, field=h * 0.5)
        assert _lib.load().asp_sa_layout_build_count() == before
        assert_same(observe(clone, chains=False), observe(clone_single, chains=False))
    finally:
        clone.release()
        clone_single.release()


def test_plan_hamiltonians_skips_what_has_a_plan(pairs):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    planned = [b for _, b, _ in pairs]
    handles = [h._plan.value for h in planned]
    fresh = _hamiltonians(_segments()[:2])
    before = lib.asp_sa_layout_build_count()
    sa.plan_hamiltonians(planned)  # nothing to do
    assert lib.asp_sa_layout_build_count() == before
    sa.plan_hamiltonians([planned[0], fresh[0], planned[1], fresh[1], fresh[0]])
    assert lib.asp_sa_layout_build_count() == before + 2
    assert [h._plan.value for h in planned] == handles
    try:
        for h, (_, _, single) in zip(fresh, pairs):
            assert h._plan is not None and h.plan().value == h._plan.value
            assert bytes(h.info()) == bytes(single.info())
    finally:
        for h in fresh:
            h.release()


@pytest.fixture(scope="module")
def kagome():
    """(arguments, hamiltonian, ground state, log amplitudes, 16 clusters) of heisenberg_kagome_16."""
    from annealing_sign_problem_amd import common, sampled_components

    arguments = ["--model", "heisenberg_kagome_16", "--order", "1", "--number-samples", "16", "--seed", "5",
                 "--min-cluster-size", "20", "--max-cluster-size", "100", "--no-annealing", "--batch", "16",
                 "--greedy-batch"]
    args = sampled_components.parse_command_line(arguments + ["--output", "unused.csv"])
    hamiltonian, ground_state = sampled_components.load_input(args)
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, hamiltonian.basis)
    np.random.seed(args.seed)
    clusters = list(sampled_components.generate_clusters(hamiltonian, ground_state, args.number_samples,
                                                         args.sampled_power, args.min_cluster_size,
                                                         args.max_cluster_size, args.keep_probability))
    return arguments, hamiltonian, log_coeff_fn, clusters


@pytest.mark.parametrize("mode", ["greedy", "sa"])
def test_solve_ising_models_is_the_same_with_batched_plans(mode, kagome):
    from annealing_sign_problem_amd import _lib, common

    _, hamiltonian, log_coeff_fn, clusters = kagome
    solutions = {}
    for plan_batch in (False, True):
        models = common.make_ising_models(clusters[:6], hamiltonian, log_psi_fn=log_coeff_fn)
        assert all(m.ising_hamiltonian._plan is None for m in models)
        before = _lib.load().asp_sa_layout_build_count()
        solutions[plan_batch] = common.solve_ising_models(models, clusters[:6], seed=17, number_sweeps=64, repetitions=8,
                                                          mode=mode, plan_batch=plan_batch)
        assert _lib.load().asp_sa_layout_build_count() == before + len(models)
        for m in models:
            m.ising_hamiltonian.release()
    assert len(solutions[True]) == 6
    for a, b in zip(solutions[False], solutions[True]):
        assert np.array_equal(a, b)


def test_the_driver_writes_the_same_bytes(tmp_path, kagome):
    from annealing_sign_problem_amd import sampled_components

    arguments = kagome[0]
    texts = {}
    for name, extra in (("loop", []), ("batch", ["--plan-batch"])):
        out = tmp_path / (name + ".csv")
        sampled_components.main(arguments + ["--output", str(out)] + extra)
        texts[name] = out.read_bytes()
    assert len(texts["loop"].splitlines()) > 16 and texts["loop"] == texts["batch"]
