"""The drivers of the device growth (specification ASP-GROW-1): generate_clusters(grow="device")
against grow_clusters called by hand with the same draws, the cut into calls, the untouched host route, and the
command line."""
import numpy as np
import pytest

import grow_cases as gc
from test_host_logic import _state_by_state_growth

pytestmark = pytest.mark.gpu

SAMPLES, POWER, SMALL, LARGE, KEEP, SEED = 8, 0.1, 5, 60, 0.5, 5


@pytest.fixture(scope="module")
def problem():
    from annealing_sign_problem_amd import sampled_components

    args = sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--order", "0", "--output", "x"])
    return sampled_components.load_input(args)


def _draws(hamiltonian, ground_state):
    """What grow="device" takes from numpy's stream, in its order: seeds, all sizes, one integer."""
    from annealing_sign_problem_amd import common, sampled_components

    np.random.seed(SEED)
    seeds = common.monte_carlo_sampling(hamiltonian.basis.states, ground_state, number_samples=SAMPLES,
                                        sampled_power=POWER).spins
    sizes = [sampled_components.random_cluster_size(SMALL, LARGE) for _ in range(SAMPLES)]
    philox_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return np.asarray(seeds, dtype=np.uint64), np.array(sizes, dtype=np.uint64), philox_seed


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == np.uint64 and np.array_equal(x, y) for x, y in zip(a, b))


def test_generate_clusters_on_the_device_is_grow_clusters_with_the_same_draws(problem):
    from annealing_sign_problem_amd import sampled_components

    hamiltonian, ground_state = problem
    seeds, sizes, philox_seed = _draws(hamiltonian, ground_state)
    after = np.random.rand()
    by_hand = sampled_components.grow_clusters(hamiltonian, seeds, sizes, KEEP, philox_seed)
    for batch in (256, 3, 1):   # rounds of --batch: cluster j keeps stream j
        np.random.seed(SEED)
        got = sampled_components.generate_clusters(hamiltonian, ground_state, SAMPLES, POWER, SMALL, LARGE, KEEP,
                                                   grow="device", batch=batch)
        assert np.random.rand() == after
        assert _same(got, by_hand), batch
    # ... and the law, with ids 0 ... 7
    law = [gc.grow_law(hamiltonian, int(s), int(r), j, KEEP, philox_seed)[0]
           for j, (s, r) in enumerate(zip(seeds, sizes))]
    assert _same(by_hand, law)
    assert all(1 <= c.size <= r and s in c.tolist() for c, s, r in zip(by_hand, seeds.tolist(), sizes.tolist()))


def test_the_cut_into_calls_changes_nothing(problem):
    from annealing_sign_problem_amd import sampled_components

    hamiltonian, ground_state = problem
    seeds, sizes, philox_seed = _draws(hamiltonian, ground_state)
    whole = sampled_components.grow_clusters(hamiltonian, seeds, sizes, KEEP, philox_seed, first_id=100)
    calls = []
    device = hamiltonian.device()
    original = device.grow_segments

    def counted(*args, **kwargs):
        calls.append(len(args[0]))
        return original(*args, **kwargs)

    device.grow_segments = counted
    try:
        per_state = device.max_connections
        for limit in (1, 70 * per_state, (int(sizes[0]) + int(sizes[1])) * per_state):
            del calls[:]
            cut = sampled_components.grow_clusters(hamiltonian, seeds, sizes, KEEP, philox_seed, first_id=100,
                                                   max_connections_per_call=limit)
            assert _same(cut, whole), limit
            assert sum(calls) == SAMPLES and len(calls) > 1
        assert calls != [1] * SAMPLES   # the last limit holds two clusters at least
    finally:
        del device.grow_segments
    shifted = sampled_components.grow_clusters(hamiltonian, seeds[3:], sizes[3:], KEEP, philox_seed, first_id=103)
    assert _same(shifted, whole[3:])


def test_the_host_route_is_untouched(problem):
    from annealing_sign_problem_amd import common, sampled_components

    hamiltonian, ground_state = problem
    for grow in ({}, {"grow": "host"}, {"grow": "host", "batch": 2}):
        np.random.seed(SEED)
        got = sampled_components.generate_clusters(hamiltonian, ground_state, SAMPLES, POWER, SMALL, LARGE, KEEP, **grow)
        after = np.random.rand()
        np.random.seed(SEED)
        seeds = common.monte_carlo_sampling(hamiltonian.basis.states, ground_state, number_samples=SAMPLES,
                                            sampled_power=POWER).spins
        want = []
        for s in seeds:
            size = sampled_components.random_cluster_size(SMALL, LARGE)
            want.append(np.array(_state_by_state_growth(hamiltonian, int(s), size, KEEP), dtype=np.uint64))
        assert after == np.random.rand()
        assert _same(got, want)


def test_the_command_line_grows_on_the_device(tmp_path):
    from annealing_sign_problem_amd import sampled_components

    out = tmp_path / "device.csv"
    arguments = ["--model", "heisenberg_kagome_16", "--order", "0", "--number-samples", str(SAMPLES), "--seed",
                 str(SEED), "--min-cluster-size", str(SMALL), "--max-cluster-size", str(LARGE), "--no-annealing",
                 "--batch", "3"]
    sampled_components.main(arguments + ["--output", str(out), "--grow", "device"])
    lines = [line for line in out.read_text().splitlines() if line and not line.startswith("#")]
    rows = [line.split(",") for line in lines if not line.startswith("size")]
    assert len(rows) == SAMPLES and len(lines) - len(rows) <= 1
    hamiltonian, ground_state = sampled_components.load_input(
        sampled_components.parse_command_line(arguments + ["--output", str(out)]))
    np.random.seed(SEED)
    clusters = sampled_components.generate_clusters(hamiltonian, ground_state, SAMPLES, POWER, SMALL, LARGE, KEEP,
                                                    grow="device", batch=3)
    for row, cluster in zip(rows, clusters):
        assert len(row) == 6 and all(float(x) == float(x) or x.strip().lower() == "nan" for x in row)
        assert np.isfinite(float(row[1])) and np.isfinite(float(row[2]))   # the greedy columns of order 0
        assert int(float(row[0])) == cluster.size   # order 0 is the grown cluster itself
