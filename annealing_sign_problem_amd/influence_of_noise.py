"""Influence of amplitude noise on the greedy sign optimisation of a small system, and the quality
of the greedy solver on the exact amplitudes — the reference's ``analyze_influence_of_noise``,
``postprocess_influence_of_noise`` and ``check_greedy_algorithm_quality`` (common.py:838-937; its
``make experiments/noise/%.csv`` and ``make quality_check``, Makefile:37-48; the module of this name
in the reference is a stub).

Every draw multiplies the ground-state amplitudes by ``exp(eps U(-1, 1))``, builds the Ising model of
the WHOLE basis and solves it greedily.  All these models have the same states and — as long as no
amplitude vanishes — the same sparsity pattern, so with ``reuse=True`` only the first draw builds an
annealer plan; every later one reweights a clone of it (``common.reweight_ising_model``, DESIGN.md
§4.14), and a round of ``batch`` draws is solved by one ``sa.greedy_solve_batch``.  The rows do not
depend on ``batch`` or ``reuse``.

    python -m annealing_sign_problem_amd.influence_of_noise --model heisenberg_kagome_16 --seed 435834 \\
        --output noise.csv --steps 1000 --repetitions 100
    python -m annealing_sign_problem_amd.influence_of_noise --model heisenberg_kagome_16 --quality
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np

from . import annealer as sa
from . import common


def influence_of_noise(hamiltonian, ground_state, noise_levels: Iterable[float], repetitions: int,
                       batch: int = 16, reuse: bool = True, seed: Optional[int] = None,
                       from_amplitudes: bool = False) -> Iterator[Tuple[float, float, float]]:
    """Rows ``(eps, amplitude_overlap, sign_overlap)``, ``repetitions`` per noise level, in the
    reference's order (common.py:887-903): ``np.random.seed(seed)`` when a seed is given, then one
    ``add_noise_to_amplitudes`` per row from numpy's global legacy stream — the stream and the rows are
    the same for every ``batch`` and both values of ``reuse``.

    ``reuse=True``: the first draw's model is built (``make_ising_model``); a round of up to ``batch``
    draws reweights a pool of that many clones and is solved by ONE ``greedy_solve_batch``.  A draw
    whose couplings leave the pattern (an amplitude that underflowed to 0) gets a model of its own.
    ``reuse=False``: the reference's loop verbatim, ``make_ising_model`` +
    ``solve_ising_model(mode="greedy")`` per draw — the comparison leg.
    ``from_amplitudes=True`` (opt-in; needs ``reuse``): a round's draws go through ONE
    ``common.reweight_ising_models`` with the pool as ``outs`` — the couplings come from the stored
    matrix elements of a coupling stencil and the new amplitudes alone, without the operator pass
     — and then one ``greedy_solve_batch``.  The rows are the same bytes."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("'batch' must be positive")
    repetitions = int(repetitions)
    if seed is not None:
        np.random.seed(seed)
    ground_state = np.asarray(ground_state, dtype=np.float64)
    basis = hamiltonian.basis
    states = basis.states
    exact_signs = sa.signs_to_bits(np.sign(ground_state))
    weights = ground_state ** 2

    def draw(eps):
        noisy = common.add_noise_to_amplitudes(ground_state, eps=eps)
        amplitude_overlap = np.dot(np.abs(noisy), np.abs(ground_state))
        return amplitude_overlap, common.ground_state_to_log_coeff_fn(noisy, basis)

    def row(eps, amplitude_overlap, x):
        _, sign_overlap = common.compute_accuracy_and_overlap(x, exact_signs, weights)
        return float(eps), float(amplitude_overlap), float(sign_overlap)

    todo = [eps for eps in noise_levels for _ in range(repetitions)]
    if not reuse:
        for eps in todo:
            amplitude_overlap, log_coeff_fn = draw(eps)
            model = common.make_ising_model(states, hamiltonian, log_psi_fn=log_coeff_fn)
            yield row(eps, amplitude_overlap, common.solve_ising_model(model, mode="greedy"))
        return

    base = None   # the one model that is built; its plan is what the pool clones
    pool = []     # models whose Hamiltonians are reweighted in place, one per draw of a round
    try:
        for start in range(0, len(todo), batch):
            round_eps = todo[start:start + batch]
            overlaps, models = [], []
            if from_amplitudes:
                fns = []
                for eps in round_eps:
                    amplitude_overlap, log_coeff_fn = draw(eps)
                    overlaps.append(amplitude_overlap)
                    fns.append(log_coeff_fn)
                if base is None:
                    base = common.make_ising_model(states, hamiltonian, log_psi_fn=fns[0])
                outs = (pool + [None] * len(fns))[:len(fns)]
                models = common.reweight_ising_models(base, log_psi_fns=fns, outs=outs)
                for k, model in enumerate(models):
                    if outs[k] is None and np.shares_memory(model.ising_hamiltonian.exchange.indices,
                                                            base.ising_hamiltonian.exchange.indices):
                        pool.append(model)  # (a new clone; a fallback model shares nothing and is used once)
                round_eps_todo = []
            else:
                round_eps_todo = round_eps
            for k, eps in enumerate(round_eps_todo):
                amplitude_overlap, log_coeff_fn = draw(eps)
                overlaps.append(amplitude_overlap)
                if base is None:
                    base = common.make_ising_model(states, hamiltonian, log_psi_fn=log_coeff_fn)
                if k < len(pool):
                    model = common.reweight_ising_model(base, log_psi_fn=log_coeff_fn, out=pool[k])
                else:
                    model = common.reweight_ising_model(base, log_psi_fn=log_coeff_fn)
                    if np.shares_memory(model.ising_hamiltonian.exchange.indices,
                                        base.ising_hamiltonian.exchange.indices):
                        pool.append(model)  # (a clone; a fallback model shares nothing and is used once)
                models.append(model)
            solved = sa.greedy_solve_batch([m.ising_hamiltonian for m in models])
            for m in models:
                if not any(m is q for q in pool):
                    m.ising_hamiltonian.release()
            for eps, amplitude_overlap, (x, _) in zip(round_eps, overlaps, solved):
                yield row(eps, amplitude_overlap, x)
    finally:  # (also when the consumer stops early: the plans go now, not with the garbage collector)
        for m in pool:
            m.ising_hamiltonian.release()
        if base is not None:
            base.ising_hamiltonian.release()


def postprocess_influence_of_noise(csv_file: str) -> np.ndarray:
    """Quartiles of the sign overlap per bin of the amplitude overlap (common.py:906-937): 100 bins
    ``(edge_i, edge_i+1]`` of [0, 1]; writes ``<csv>_stats.csv`` with the columns ``amplitude_overlap``
    (bin centre), ``median``, ``upper`` (75 %), ``lower`` (25 %) — NaN for an empty bin — and returns
    that table."""
    if not csv_file.endswith(".csv"):
        raise ValueError("'{}' does not end in .csv: the statistics file would have its name".format(csv_file))
    table = np.loadtxt(csv_file, delimiter=",", ndmin=2)
    amplitude_overlap, sign_overlap = table[:, 1], table[:, 2]
    edges = np.linspace(0, 1, 101)
    stats = np.full((100, 4), np.nan)
    stats[:, 0] = 0.5 * (edges[1:] + edges[:-1])
    for i in range(100):
        inside = sign_overlap[(edges[i] < amplitude_overlap) & (amplitude_overlap <= edges[i + 1])]
        if inside.size:
            if np.any(inside > 1):  # (rows that fall in no bin are not looked at, as in the reference)
                raise ValueError("sign overlaps above 1 in '{}'".format(csv_file))
            lower, median, upper = np.percentile(inside, [25, 50, 75])
            stats[i, 1:] = median, upper, lower
    with open(csv_file[:-len(".csv")] + "_stats.csv", "w") as f:
        f.write("amplitude_overlap,median,upper,lower\n")
        np.savetxt(f, stats, delimiter=",")
    return stats


def check_greedy_algorithm_quality(hamiltonian, ground_state) -> Tuple[float, float]:
    """``(sign accuracy, sign overlap)`` of the greedy solution of the whole basis' Ising model on the
    exact amplitudes (common.py:838-856)."""
    ground_state = np.asarray(ground_state, dtype=np.float64)
    basis = hamiltonian.basis
    exact_signs = sa.signs_to_bits(np.sign(ground_state))
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, basis)
    model = common.make_ising_model(basis.states, hamiltonian, log_psi_fn=log_coeff_fn)
    x = common.solve_ising_model(model, mode="greedy")
    accuracy, overlap = common.compute_accuracy_and_overlap(x, exact_signs, ground_state ** 2)
    return float(accuracy), float(overlap)


def load_inputs(model: Optional[str] = None, yaml_filename: Optional[str] = None,
                hdf5_filename: Optional[str] = None):
    """``(operator with its basis built, normalised ground state)``: a name of models.json (ground
    state by exact diagonalisation) or the reference's YAML + SpinED files."""
    from . import operators, synthetic

    if yaml_filename is not None:
        hamiltonian = common.load_hamiltonian(yaml_filename)
        hdf5_filename = hdf5_filename or yaml_filename.replace(".yaml", ".h5")
    else:
        models = synthetic.load_models()
        if model not in models:
            raise ValueError("unknown model '{}'; available: {}".format(model, sorted(models)))
        hamiltonian = operators.Operator.from_config(models[model])
    if hdf5_filename is not None:
        ground_state, _, representatives = common.load_ground_state(hdf5_filename)
        order = np.argsort(representatives, kind="stable")
        hamiltonian.basis.build(representatives[order])
        ground_state = np.ascontiguousarray(ground_state[order])
    else:
        hamiltonian.basis.build()
        _, ground_state = hamiltonian.ground_state()
    if not np.isclose(np.linalg.norm(ground_state), 1):
        raise ValueError("the ground state is not normalised")
    return hamiltonian, ground_state


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description="Influence of noise on greedy optimization (small systems).")
    parser.add_argument("--model", type=str, help="name in models.json (ground state by ED)")
    parser.add_argument("--yaml", type=str, help="physical_systems/<model>.yaml of the reference")
    parser.add_argument("--hdf5", type=str, help="SpinED output (default <yaml>.h5 with --yaml)")
    parser.add_argument("--output", type=str)
    parser.add_argument("--seed", type=int)
    parser.add_argument("--min-noise", type=float, default=1e-2)
    parser.add_argument("--max-noise", type=float, default=1e2)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--repetitions", type=int, default=10)
    parser.add_argument("--batch", type=int, default=16, help="draws solved by one greedy_solve_batch")
    parser.add_argument("--no-reuse", action="store_true",
                        help="build every draw's model and plan from scratch (the reference's loop)")
    parser.add_argument("--from-amplitudes", action="store_true",
                        help="couplings of a round from stored matrix elements and the new amplitudes alone "
                             "(coupling stencil); the same rows")
    parser.add_argument("--quality", action="store_true",
                        help="print 'sign accuracy,sign overlap' of the greedy solver on the exact amplitudes")
    args = parser.parse_args(argv)
    if (args.model is None) == (args.yaml is None):
        raise SystemExit("give exactly one of --model and --yaml")
    if args.quality:
        hamiltonian, ground_state = load_inputs(args.model, args.yaml, args.hdf5)
        print("{},{}".format(*check_greedy_algorithm_quality(hamiltonian, ground_state)))
        return 0
    if args.output is None or args.seed is None:
        raise SystemExit("--output and --seed are required")
    if os.path.exists(args.output):
        print("'{}' exists already and is not overwritten; remove it first to run again".format(args.output),
              file=sys.stderr)
        return 1
    np.random.seed(args.seed)  # (before the inputs are loaded, as in the reference)
    hamiltonian, ground_state = load_inputs(args.model, args.yaml, args.hdf5)
    noise_levels = np.exp(np.linspace(np.log(args.min_noise), np.log(args.max_noise), args.steps))
    rows = influence_of_noise(hamiltonian, ground_state, noise_levels, args.repetitions, batch=args.batch,
                              reuse=not args.no_reuse, from_amplitudes=args.from_amplitudes)
    pending = []
    for done, row in enumerate(rows, 1):
        pending.append("{},{},{}\n".format(*row))
        if len(pending) == args.batch or done == args.steps * args.repetitions:
            with open(args.output, "a") as f:  # one append per round
                f.writelines(pending)
            pending = []
    return 0


if __name__ == "__main__":
    sys.exit(main())
