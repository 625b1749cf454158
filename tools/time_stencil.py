"""Timing of the coupling stencil (ASP-STENCIL-1) on the GPU: what a draw of the noise
study pays for its couplings with the operator pass (DeviceOperator.ising_csr) and from stored matrix
elements (IsingStencil.values), the model-level calls built on them, and the study's three legs.

    python tools/time_stencil.py [--models a,b] [--rounds 7] [--output profiles/stencil_timing.txt]

Method: a warm-up round first, then the median of `rounds` rounds of 16 draws on a host clock around calls
that end in a device synchronise; device parts from HIP events (asp_operator_last_ms,
asp_sa_plan_reweight_stencil_last_ms).  Stencil creation is paid once per model: one timed call."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import common, operators, synthetic  # noqa: E402
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


def median_ms(call, rounds, per=1):
    """Median over `rounds` rounds (after a warm-up round) of the wall time of call(), divided by `per`."""
    times = []
    for _ in range(rounds + 1):
        tick = time.perf_counter()
        call()
        times.append((time.perf_counter() - tick) * 1e3 / per)
    return float(np.median(times[1:]))


def couplings(operator, ground_state, rounds, lines):
    """Stencil creation, ising_csr alone, stencil values for 1 and 16 draws."""
    basis = operator.basis
    keys = basis.states
    device = operator.device()
    np.random.seed(2)
    psis = np.stack([common.add_noise_to_amplitudes(ground_state, eps=1.0) for _ in range(DRAWS)])
    psis /= np.linalg.norm(psis, axis=1, keepdims=True)
    indptr, col, val = device.ising_csr(keys, psis[0])
    pattern = (indptr.copy(), col.copy())
    tick = time.perf_counter()
    stencil = device.ising_stencil(keys, *pattern)
    create = (time.perf_counter() - tick) * 1e3
    info = stencil.info
    lines.append("  K = %d, nnz = %d, in-cluster connections = %d in %d groups (longest %d), silent pairs = %d"
                 % (info.num_spins, info.stored, info.connections, info.groups, info.longest_group, info.silent_pairs))
    lines.append("  stencil creation (once per model)            %8.3f ms wall" % create)
    events = []

    def operator_pass():
        for d in range(DRAWS):
            device.ising_csr(keys, psis[d])
            events.append(device.last_ms)

    wall = median_ms(operator_pass, rounds, DRAWS)
    lines.append("  ising_csr, one draw per call                 %8.3f ms wall per draw, %.3f ms of it on the device"
                 % (wall, float(np.median(events[DRAWS:]))))
    one = median_ms(lambda: [stencil.values(psis[d]) for d in range(DRAWS)], rounds, DRAWS)
    lines.append("  stencil values, one draw per call            %8.3f ms wall per draw" % one)
    many = median_ms(lambda: stencil.values(psis), rounds, DRAWS)
    lines.append("  stencil values, 16 draws per call            %8.3f ms wall per draw" % many)
    data, status = stencil.values(psis)
    assert not status.any() and np.array_equal(data[0].view(np.uint64), val.view(np.uint64))
    stencil.close()


def models(operator, ground_state, rounds, lines):
    """reweight_ising_model against reweight_ising_models per draw, at batch 1 and 16, pools as `out`."""
    basis = operator.basis
    np.random.seed(3)
    fns = [common.ground_state_to_log_coeff_fn(common.add_noise_to_amplitudes(ground_state, eps=1.0), basis)
           for _ in range(DRAWS)]
    base = common.make_ising_model(basis.states, operator, log_psi_fn=fns[0])
    base.ising_hamiltonian.plan()
    pool_one = [common.reweight_ising_model(base, log_psi_fn=fn) for fn in fns]
    pool_many = common.reweight_ising_models(base, log_psi_fns=fns)
    device = []

    def per_model():
        for fn, out in zip(fns, pool_one):
            common.reweight_ising_model(base, log_psi_fn=fn, out=out)

    def batched(size):
        def call():
            for first in range(0, DRAWS, size):
                common.reweight_ising_models(base, log_psi_fns=fns[first:first + size], outs=pool_many[first:first + size])
                device.append(sa.reweight_hamiltonians_last_ms() / size)
        return call

    lines.append("  reweight_ising_model  (operator pass)        %8.3f ms wall per draw" % median_ms(per_model, rounds, DRAWS))
    for size in (1, DRAWS):
        del device[:]
        wall = median_ms(batched(size), rounds, DRAWS)
        lines.append("  reweight_ising_models (stencil), batch %-2d     %8.3f ms wall per draw, %.3f ms of it on the device"
                     % (size, wall, float(np.median(device[DRAWS // size:]))))
    for model in pool_one + pool_many + [base]:
        model.ising_hamiltonian.release()


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--models", default="heisenberg_kagome_16,j1j2_square_4x4")
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--output", default=None)
    args = parser.parse_args(argv)
    lines = ["coupling stencil timing: median of %d rounds of %d draws after one warm-up round" % (args.rounds, DRAWS)]
    for name in args.models.split(","):
        operator = operators.Operator.from_config(synthetic.load_models()[name])
        operator.basis.build()
        _, ground_state = operator.ground_state()
        lines.append("%s:" % name)
        couplings(operator, ground_state, args.rounds, lines)
        models(operator, ground_state, args.rounds, lines)
        legs = (("noise study, reuse=False", dict(reuse=False)),
                ("noise study, reuse=True, batch=16", dict(reuse=True, batch=DRAWS)),
                ("noise study, from_amplitudes=True, batch=16", dict(from_amplitudes=True, batch=DRAWS)))
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
