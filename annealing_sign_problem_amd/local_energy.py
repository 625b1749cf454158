"""Local energies of recovered signs on Monte-Carlo samples.

The reference ends in this (experiments/sampled_connected_components.py:294-359,
``compute_local_energy_impl``, ``compute_local_energy``, ``create_cluster_for_local_energy``): for
every sample, take its one-hop neighbourhood as a cluster, optimise the cluster's signs through the
extension orders, and evaluate

    E_loc(s) = sum_s' H_ss' (|psi_s'| sign_s') / (|psi_s| sign_s)

Here the clusters of all samples are staged like ``sampled_components.stage_clusters`` stages them,
the last order of every sample is solved in ONE batched call, and the local energies of all samples
come from ONE ``DeviceOperator.local_energy`` call (specification ASP-ELOC-1): one
segment and one row per unique sample, because every cluster's signs are known only up to a global
flip and so belong to that cluster alone.

Nothing here promises a quality: the mean of the local energies over samples drawn from |psi|^2 is
the energy of the state that carries the recovered signs only in so far as the recovered signs of
different clusters are those of ONE state ("what the numbers mean").
"""
from __future__ import annotations

import argparse
import os
from typing import List, Sequence, Tuple

import numpy as np

from . import annealer as sa
from . import common, operators, synthetic

SIGNS = ("greedy", "sa", "exact")


def _amplitudes(log_psi_fn, spins: np.ndarray) -> np.ndarray:
    """``exp(Re log_psi_fn(spins))``."""
    if hasattr(log_psi_fn, "index_of"):  # (ground_state_to_log_coeff_fn's closure)
        log_psi = log_psi_fn.at_index(log_psi_fn.index_of(spins))
    else:
        log_psi = log_psi_fn(spins)
    return np.ascontiguousarray(np.exp(np.asarray(log_psi).real), dtype=np.float64)


def last_order_models(clusters: Sequence[np.ndarray], hamiltonian, log_psi_fn, order: int, global_cutoff: float,
                      external_field: bool = False, jobs: int = 1) -> List[common.IsingModel]:
    """The model of extension order ``order`` of every cluster, built through the orders 0...``order``
    exactly as ``sampled_components.stage_clusters`` builds them (the cluster frozen in the sparsifier).
    Only the returned models are ever solved, so the lower orders never get a device plan."""
    field = {"external_field": True} if external_field else {}

    def stage(cluster):
        h = common.make_ising_model(cluster, hamiltonian, log_psi_fn=log_psi_fn, **field)
        for _ in range(order):
            h = common.make_hamiltonian_extension(h, log_psi_fn, **field)
            h = common.sparsify_using_global_cutoff(h, global_cutoff, cluster)
        return h

    if jobs > 1 and len(clusters) > 1:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=jobs) as pool:
            return list(pool.map(stage, clusters))
    return [stage(cluster) for cluster in clusters]


def sample_local_energies(hamiltonian, ground_state, samples, log_psi_fn, order: int, global_cutoff: float,
                          signs: str = "greedy", external_field: bool = False, seed: int = 12345, jobs: int = 1,
                          number_sweeps: int = 5120, repetitions: int = 64
                          ) -> List[Tuple[int, int, float, int, int]]:
    """Per unique sample ``(state, cluster size, E_loc, missing, count)``, ascending in the state.

    ``samples``: basis states (representatives in a symmetry sector), repeats allowed; ``count`` is
    the multiplicity of a state among them.  The cluster of a sample is its one-hop neighbourhood
    (``common.extension_spins``); its signs come from the greedy solver (``signs="greedy"``) or the
    annealer (``"sa"``, with ``seed``, ``number_sweeps``, ``repetitions``) on the model of extension
    order ``order``, projected on the cluster, or from ``ground_state`` (``"exact"``: no model is
    built); its amplitudes are ``exp(Re log_psi_fn)``.  ``missing`` counts the connections of the
    sample that end outside its cluster with a non-zero matrix element: 0, unless the operator
    reaches a state of norm 0 that the extension leaves out with a coefficient that is not exactly 0.
    This package's device operators only."""
    if signs not in SIGNS:
        raise ValueError("invalid signs specified: '{}'; expected one of {}".format(signs, SIGNS))
    if not common._on_device(hamiltonian):
        raise NotImplementedError(
            "sample_local_energies needs one of this package's device operators (operators.Operator with real "
            "matrices); it is not implemented for foreign operator objects")
    samples = np.asarray(samples, dtype=np.uint64)
    if samples.ndim > 1:
        samples = samples[:, 0]
    states, counts = np.unique(samples, return_counts=True)
    if states.size == 0:
        return []
    clusters = [common.extension_spins(hamiltonian, states[i:i + 1]) for i in range(states.size)]
    if signs == "exact":
        ground_state = np.asarray(ground_state, dtype=np.float64)
        basis = hamiltonian.basis
        cluster_signs = [np.sign(ground_state[np.asarray(basis.batched_index(c), dtype=np.int64)]) for c in clusters]
    else:
        models = last_order_models(clusters, hamiltonian, log_psi_fn, order, global_cutoff, external_field, jobs)
        solved = common.solve_ising_models(models, frozen_spins=clusters, seed=seed, number_sweeps=number_sweeps,
                                           repetitions=repetitions, mode=signs)
        cluster_signs = [sa.bits_to_signs(x, count=c.size) for x, c in zip(solved, clusters)]
        for model in models:
            model.ising_hamiltonian.release()
    offsets = np.zeros(states.size + 1, dtype=np.uint64)
    np.cumsum([c.size for c in clusters], out=offsets[1:])
    keys = np.concatenate(clusters)
    phi = _amplitudes(log_psi_fn, keys) * np.concatenate(cluster_signs)
    rows = np.array([int(offsets[i]) + int(common.binary_search(clusters[i], states[i:i + 1])[0])
                     for i in range(states.size)], dtype=np.uint64)
    _, eloc, missing = hamiltonian.device().local_energy(keys, phi, offsets, rows)
    return [(int(states[i]), int(clusters[i].size), float(eloc[i]), int(missing[i]), int(counts[i]))
            for i in range(states.size)]


def weighted_mean(results) -> Tuple[float, float]:
    """``(mean, standard error)`` of the local energies weighted by the counts: the mean over the
    samples, and ``sqrt(variance / number of samples)`` with the variance over the samples (not an
    error bar for correlated chains; the samples of ``common.monte_carlo_sampling`` are independent)."""
    energy = np.array([r[2] for r in results], dtype=np.float64)
    count = np.array([r[4] for r in results], dtype=np.float64)
    total = count.sum()
    mean = float((count * energy).sum() / total)
    if total < 2:
        return mean, float("nan")
    variance = float((count * (energy - mean) ** 2).sum() / (total - 1))
    return mean, float(np.sqrt(variance / total))


def parse_command_line(argv=None):
    parser = argparse.ArgumentParser(description="Local energies of recovered signs on Monte-Carlo samples.")
    parser.add_argument("--model", type=str, required=True, help="name in models.json")
    parser.add_argument("--hdf5", type=str,
                        help="SpinED output with the ground state, its energy and the basis representatives; "
                             "without it the model is diagonalised on the spot")
    parser.add_argument("--output", type=str, required=True)
    parser.add_argument("--number-samples", type=int, default=1000)
    parser.add_argument("--sampled-power", type=float, default=2.0,
                        help="samples are drawn with probability ~ |psi|^p; only p = 2 makes the mean an energy")
    parser.add_argument("--order", type=int, default=2)
    parser.add_argument("--global-cutoff", type=float, default=1e-6)
    parser.add_argument("--signs", type=str, default="greedy", choices=SIGNS)
    parser.add_argument("--noise", type=float, default=0)
    parser.add_argument("--external-field", default=False, action="store_true")
    parser.add_argument("--seed", type=int, default=12345)
    parser.add_argument("--jobs", type=int, default=1)
    return parser.parse_args(argv)


def load_input(args):
    """``(hamiltonian, ground_state, E0 or None)``."""
    models = synthetic.load_models()
    if args.model not in models:
        raise SystemExit("unknown model '{}'; available: {}".format(args.model, sorted(models)))
    hamiltonian = operators.Operator.from_config(models[args.model])
    if args.hdf5 is None:
        hamiltonian.basis.build()
        energy, ground_state = hamiltonian.ground_state()
        return hamiltonian, ground_state, energy
    ground_state, energy, representatives = common.load_ground_state(args.hdf5)
    order = np.argsort(representatives, kind="stable")
    hamiltonian.basis.build(representatives[order])
    return hamiltonian, np.ascontiguousarray(ground_state[order]), (energy if np.isfinite(energy) else None)


def main(argv=None):
    args = parse_command_line(argv)
    if os.path.exists(args.output):
        raise SystemExit("Output file '{}' already exists: refusing to overwrite".format(args.output))
    np.random.seed(args.seed)
    hamiltonian, ground_state, e0 = load_input(args)
    noisy = common.add_noise_to_amplitudes(ground_state, args.noise) if args.noise > 0 else ground_state
    log_psi_fn = common.ground_state_to_log_coeff_fn(noisy, hamiltonian.basis)
    sampled = common.monte_carlo_sampling(hamiltonian.basis.states, ground_state, args.number_samples,
                                          args.sampled_power)
    results = sample_local_energies(hamiltonian, ground_state, sampled.spins, log_psi_fn, args.order,
                                    args.global_cutoff, signs=args.signs, external_field=args.external_field,
                                    seed=args.seed, jobs=args.jobs)
    mean, error = weighted_mean(results)
    with open(args.output, "w") as f:
        f.write("# Generated by annealing_sign_problem_amd.local_energy\n")
        for key in ["model", "seed", "number_samples", "sampled_power", "order", "global_cutoff", "signs", "noise",
                    "external_field"]:
            f.write("# {} = {}\n".format(key, getattr(args, key)))
        f.write("# mean = {!r}\n".format(mean))
        f.write("# standard_error = {!r}\n".format(error))
        if e0 is not None:
            f.write("# E0 = {!r}\n".format(float(e0)))
        f.write("# missing_total = {}\n".format(sum(r[3] * r[4] for r in results)))
        f.write("# state,size,local_energy,missing,count\n")
        for state, size, energy, missing, count in results:
            f.write("{},{},{!r},{},{}\n".format(state, size, energy, missing, count))
    print("{}: {} samples ({} unique), signs={}, order={}: E = {:.10g} +- {:.3g}{}".format(
        args.model, args.number_samples, len(results), args.signs, args.order, mean, error,
        "" if e0 is None else ", E0 = {:.10g}".format(e0)))


if __name__ == "__main__":
    main()
