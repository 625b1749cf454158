"""How the couplings of a model's Ising problem are distributed and how often they are frustrated —
the reference's ``analyze_coupling_distribution``, ``analyze_probability_of_frustration`` and
``analyze_smallest_amplitude_overlap`` (common.py:940-1024; its ``make experiments/couplings/%.csv``,
``make is_frustrated`` and ``make small_amplitude_overlaps``).  The statistics run on the GPU
(:mod:`.bonds`).

    python -m annealing_sign_problem_amd.coupling_analysis --model heisenberg_kagome_16 \\
        --couplings couplings.csv --is-frustrated is_frustrated.csv
    python -m annealing_sign_problem_amd.coupling_analysis --model heisenberg_kagome_36 --sector \\
        --is-frustrated is_frustrated.csv
    python -m annealing_sign_problem_amd.coupling_analysis --model sk_16_1 --smallest-overlap

``--sector``: the ground state of the model's symmetry sector comes from :mod:`.sector_ed` and stays on
the device, and so does the Ising model built from it (``BondStatistics.from_sector``): the route for
bases whose ``J`` does not fit on the host (heisenberg_kagome_36: 31.5 million representatives).
"""
from __future__ import annotations

import argparse
import sys
from typing import Tuple

import numpy as np

from . import common
from .bonds import BondStatistics
from .influence_of_noise import load_inputs


def whole_basis_model(hamiltonian, ground_state) -> common.IsingModel:
    """The Ising model of the whole basis on the exact amplitudes (common.py:952-953, 973-974)."""
    basis = hamiltonian.basis
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, basis)
    return common.make_ising_model(basis.states, hamiltonian, log_psi_fn=log_coeff_fn)


def smallest_amplitude_overlap(ground_state, trials: int = 100, seed: int = 12345) -> Tuple[float, float, float]:
    """``(mean, median, interquartile range)`` of the overlap of ``|psi|`` with ``trials`` vectors of
    uniform random amplitudes (common.py:1011-1024; host only)."""
    np.random.seed(seed)
    amplitudes = np.abs(np.asarray(ground_state, dtype=np.float64))
    overlaps = np.zeros(trials)
    for i in range(trials):
        noise = np.random.rand(len(amplitudes))
        overlaps[i] = abs(np.dot(amplitudes, noise)) / np.linalg.norm(noise)
    quartiles = np.percentile(overlaps, [25, 50, 75])
    return float(np.mean(overlaps)), float(quartiles[1]), float(quartiles[2] - quartiles[0])


def sector_statistics(model_config, tol: float = 1e-8, log=None) -> BondStatistics:
    """Ground state of the model's symmetry sector by :mod:`.sector_ed` and, from it, the device-resident
    Ising model of the whole sector."""
    import torch

    from . import operators, sector_ed

    operator = operators.Operator.from_config(model_config)
    representatives, norms = sector_ed.enumerate_sector(operator, log=log)
    matrix = sector_ed.SectorMatrix(operator, representatives, norms, log=log)
    _, psi, _ = sector_ed.lanczos_ground_state(matrix, tol=tol, log=log)
    torch.cuda.empty_cache()  # (the Krylov basis: the library allocates outside torch's cache)
    stats = BondStatistics.from_sector(matrix, psi)
    if log:
        summary = stats.summary
        held = summary["stored"] * 12 + summary["num_spins"] * 26
        log("sector Ising model: n = %d, %d couplings, built in %.1f ms, %.2f GB in HBM" % (
            summary["num_spins"], summary["stored"], stats.create_ms, held / 1e9))
    return stats


def write_is_frustrated(filename: str, x, y) -> None:
    np.savetxt(filename, np.vstack([x, y]).T, delimiter=",")


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description="Distribution and frustration of the couplings of a model.")
    parser.add_argument("--model", type=str, help="name in models.json (ground state by ED)")
    parser.add_argument("--yaml", type=str, help="physical_systems/<model>.yaml of the reference")
    parser.add_argument("--hdf5", type=str, help="SpinED output (default <yaml>.h5 with --yaml)")
    parser.add_argument("--couplings", type=str, metavar="OUT", help="|J| of all bonds, descending, one per line")
    parser.add_argument("--is-frustrated", type=str, metavar="OUT",
                        help="'coupling,probability that a bond of that strength is not frustrated' per bin")
    parser.add_argument("--smallest-overlap", action="store_true",
                        help="print mean, median and interquartile range of the overlap with random amplitudes")
    parser.add_argument("--trials", type=int, default=100)
    parser.add_argument("--seed", type=int, default=12345)
    parser.add_argument("--sector", action="store_true",
                        help="ground state and Ising model of the whole symmetry sector on the device")
    args = parser.parse_args(argv)
    if (args.model is None) == (args.yaml is None):
        raise SystemExit("give exactly one of --model and --yaml")
    if not (args.couplings or args.is_frustrated or args.smallest_overlap):
        raise SystemExit("nothing to do: give --couplings, --is-frustrated or --smallest-overlap")

    def log(line):
        print(line, flush=True)

    if args.sector:
        if args.model is None or args.smallest_overlap:
            raise SystemExit("--sector takes --model, and --couplings or --is-frustrated")
        from . import synthetic

        models = synthetic.load_models()
        if args.model not in models:
            raise SystemExit("unknown model '{}'; available: {}".format(args.model, sorted(models)))
        stats = sector_statistics(models[args.model], log=log)
    else:
        hamiltonian, ground_state = load_inputs(args.model, args.yaml, args.hdf5)
        if args.smallest_overlap:
            print("mean: {}, median: {}, interquartile: {}".format(
                *smallest_amplitude_overlap(ground_state, args.trials, args.seed)))
        if not (args.couplings or args.is_frustrated):
            return 0
        model = whole_basis_model(hamiltonian, ground_state)
        stats = BondStatistics(model.ising_hamiltonian, model.initial_signs)
        model.ising_hamiltonian.release()
    with stats:
        summary = stats.summary
        bonds, size = summary["bonds"], summary["num_spins"]
        log("spins={}, bonds={}, frustrated={}, largest_frustrated={}".format(
            size, bonds, summary["frustrated"] / bonds if bonds else float("nan"),
            summary["strongest_frustrated"] / size if size else float("nan")))
        if args.is_frustrated:
            x, y, _, _ = common.probability_of_frustration(stats)
            log("histogram: %.3f ms on the device" % stats.last_ms())
            write_is_frustrated(args.is_frustrated, x, y)
        if args.couplings:
            np.savetxt(args.couplings, stats.magnitudes())
            log("magnitudes: %.3f ms on the device" % stats.last_ms())
    return 0


if __name__ == "__main__":
    sys.exit(main())
