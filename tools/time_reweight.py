"""Timing of plan re-use on the GPU: asp_sa_plan_reweight against asp_sa_plan_create on
the same matrix, and the noise study's wall time per draw with fresh plans (reuse=False: the loop as it
was before plan re-use existed) against reweighted clones at batch 1 and 16.

    python tools/time_reweight.py [--models a,b] [--rounds 7] [--output profiles/reweight_timing.txt]

Method: a warm-up round first, then the median of `rounds` rounds of 16 draws on a host clock (every
round ends in a device synchronise); the device part of a reweight from HIP events
(asp_sa_plan_reweight_last_ms)."""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import _lib, common, operators, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402
from annealing_sign_problem_amd.influence_of_noise import influence_of_noise  # noqa: E402

DRAWS = 16


def per_draw_ms(operator, ground_state, rounds, **how):
    rows = influence_of_noise(operator, ground_state, [1.0], DRAWS * (rounds + 1), seed=1, **how)
    times = []
    for _ in range(rounds + 1):
        tick = time.perf_counter()
        for _ in range(DRAWS):
            next(rows)
        times.append((time.perf_counter() - tick) * 1e3 / DRAWS)
    rows.close()
    return float(np.median(times[1:])), float(np.min(times[1:])), float(np.max(times[1:]))


def create_and_reweight_ms(operator, ground_state, rounds):
    lib = _lib.load()
    basis = operator.basis
    np.random.seed(2)
    models = []
    for _ in range(2):
        noisy = common.add_noise_to_amplitudes(ground_state, eps=1.0)
        models.append(common.make_ising_model(basis.states, operator,
                                              log_psi_fn=common.ground_state_to_log_coeff_fn(noisy, basis)))
    a, b = (m.ising_hamiltonian for m in models)
    create, reweight, device = [], [], []
    target = sa.Hamiltonian.from_canonical_csr(a.exchange.indptr, a.exchange.indices, a.exchange.data, a.field)
    target.plan()
    for k in range(rounds * DRAWS + 1):
        source = b if k % 2 == 0 else a
        fresh = sa.Hamiltonian.from_canonical_csr(source.exchange.indptr, source.exchange.indices,
                                                  source.exchange.data, source.field)
        tick = time.perf_counter()
        fresh.plan()
        create.append((time.perf_counter() - tick) * 1e3)
        fresh.release()
        tick = time.perf_counter()
        target.reweight(source.exchange.data, source.field)
        reweight.append((time.perf_counter() - tick) * 1e3)
        device.append(float(lib.asp_sa_plan_reweight_last_ms(target.plan())))
    info = target.info()
    return (info.num_spins, a.exchange.nnz, float(np.median(create[1:])), float(np.median(reweight[1:])),
            float(np.median(device[1:])))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--models", default="j1j2_square_4x4,heisenberg_kagome_16")
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--output", default=None)
    args = parser.parse_args(argv)
    lines = ["plan re-use timing: median of %d rounds of %d draws after one warm-up round" % (args.rounds, DRAWS)]
    for name in args.models.split(","):
        operator = operators.Operator.from_config(synthetic.load_models()[name])
        operator.basis.build()
        _, ground_state = operator.ground_state()
        K, nnz, create, reweight, device = create_and_reweight_ms(operator, ground_state, args.rounds)
        lines.append("%s: K = %d, nnz = %d" % (name, K, nnz))
        lines.append("  asp_sa_plan_create   %8.3f ms wall (Hamiltonian.plan)" % create)
        lines.append("  asp_sa_plan_reweight %8.3f ms wall (Hamiltonian.reweight), %.3f ms of it on the device"
                     % (reweight, device))
        legs = (("reuse=False (fresh model and plan per draw)", dict(reuse=False)),
                ("reuse=True, batch=1", dict(reuse=True, batch=1)),
                ("reuse=True, batch=16", dict(reuse=True, batch=DRAWS)))
        for label, how in legs:
            median, least, most = per_draw_ms(operator, ground_state, args.rounds, **how)
            lines.append("  %-44s %8.3f ms per draw (min %.3f, max %.3f); 1000 x 100 draws: %.0f s"
                         % (label, median, least, most, median * 100.0))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
