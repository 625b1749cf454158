"""The drivers' device scoring (specification ASP-SCORE-1): a trial of
full_hilbert_space with --score device against --score host, and a round of sampled_components with and
without --score-batch.  Accuracies are equal (as bits, and as printed); overlaps agree to
(K + 64) * 2^-53, compared chain by chain and solution by solution, never through a threshold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bound(spins: int) -> float:
    return (spins + 64) * 2.0 ** -53


def test_full_hilbert_space_trial_scored_on_the_device():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import full_hilbert_space

    simulation = full_hilbert_space.Simulation("heisenberg_kagome_16")
    seed = 12345
    on_host = simulation.run(100, 64, seed)
    on_device = simulation.run(100, 64, seed, score="device")
    assert on_device[0] == on_host[0] and on_device[2] == on_host[2]  # accuracy and residual fractions
    # the chains of that trial, one by one
    xs, es = sa.anneal(simulation.exact_model.ising_hamiltonian, seed=seed, number_sweeps=100, repetitions=64,
                       only_best=False)
    host = simulation.chain_scores(xs, es, "host")
    device = simulation.chain_scores(xs, es, "device")
    assert np.array_equal(host[:, 0].view(np.uint64), device[:, 0].view(np.uint64))
    assert np.array_equal(host[:, 2].view(np.uint64), device[:, 2].view(np.uint64))
    assert np.all(np.abs(host[:, 1] - device[:, 1]) <= _bound(simulation.exact_model.size))
    assert simulation.analyze(xs, es) == on_host
    with pytest.raises(ValueError):
        simulation.run(100, 64, seed, score="elsewhere")


def test_sampled_components_round_scored_in_one_call(tmp_path):
    from annealing_sign_problem_amd import common, sampled_components

    arguments = ["--model", "heisenberg_kagome_16", "--order", "1", "--number-samples", "3", "--seed", "5",
                 "--max-cluster-size", "300", "--greedy-batch"]
    args = sampled_components.parse_command_line(arguments + ["--output", str(tmp_path / "none.csv")])
    assert sampled_components.score_batch_of(args) == {}
    hamiltonian, ground_state = sampled_components.load_input(args)
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, hamiltonian.basis)
    np.random.seed(args.seed)
    clusters = sampled_components.generate_clusters(hamiltonian, ground_state, args.number_samples,
                                                    args.sampled_power, args.min_cluster_size,
                                                    args.max_cluster_size, args.keep_probability)

    def round_of(**extra):
        return sampled_components.process_clusters_batched(clusters, hamiltonian, ground_state, ground_state,
                                                           log_coeff_fn, args.order, args.global_cutoff, True,
                                                           sweep_order=args.sweep_order, greedy_batch=True, **extra)

    one_by_one, at_once = round_of(), round_of(score_batch=True)
    assert len(one_by_one) == len(at_once) == len(clusters)
    for cluster, columns, batched in zip(clusters, one_by_one, at_once):
        assert len(columns) == len(batched) == args.order + 1
        for r, b in zip(columns, batched):
            printed, printed_batched = r.to_csv_str().split(","), b.to_csv_str().split(",")
            for column in (0, 1, 3, 5):  # size, the two accuracies, the amplitude overlap: as printed
                assert printed[column] == printed_batched[column]
            assert np.float64(r.greedy_accuracy).view(np.uint64) == np.float64(b.greedy_accuracy).view(np.uint64)
            assert np.float64(r.sa_accuracy).view(np.uint64) == np.float64(b.sa_accuracy).view(np.uint64)
            assert abs(r.greedy_overlap - b.greedy_overlap) <= _bound(len(cluster))
            assert abs(r.sa_overlap - b.sa_overlap) <= _bound(len(cluster))
            assert np.isfinite(b.sa_overlap) and np.isfinite(b.greedy_overlap)
    # the command line: the same accuracy columns in the file
    out = tmp_path / "batched.csv"
    sampled_components.main(arguments + ["--output", str(out), "--score-batch"])
    rows = [line.split(",") for line in out.read_text().splitlines() if line and not line.startswith("#")]
    rows = [row for row in rows if not row[0].startswith("size")]
    assert len(rows) == len(clusters)
    for row, batched in zip(rows, at_once):
        want = ",".join(b.to_csv_str() for b in batched).split(",")
        assert len(row) == len(want)
        for k in range(0, len(want), 6):
            assert row[k] == want[k] and row[k + 1] == want[k + 1] and row[k + 3] == want[k + 3]
