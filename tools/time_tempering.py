"""Cost of parallel tempering's two pieces (DESIGN.md §4.10 "Ladder law", §4.12) on one planted cluster
of --size spins with --chains chains, in both sweep orders.

    python tools/time_tempering.py [--size 3000] [--chains 64] [--sweeps 10] [--repeat 5]

(a) the per-chain beta: a ladder segment of --sweeps sweeps with ALL betas equal (asp_sa_chains_advance_ladder)
    against asp_sa_chains_advance on the same constant segment, in the same library — the same chains bit
    for bit (checked first), so the difference is what the ladder kernels cost; device time of the sweep
    launches (asp_sa_last_sweep_ms) and of the whole segment (asp_sa_last_total_ms), and wall time.  The
    baseline is the existing path.  A segment on the geometric ladder is timed too, for the record (other
    chains: hot chains flip more).
(b) one exchange step (asp_sa_chains_exchange): wall time and device time (asp_sa_last_total_ms: energies
    to the end of the gather), against the route through the host — Chains.state(), Hamiltonian.energies,
    law ASP-PT-1 in numpy, Chains.load_state() — wall time only (it has no single device span).
Every timed call starts from the same snapshot (load_state, not timed); median and spread over --repeat
rounds after a warm-up.  Output goes to profiles/tempering_timing.txt by hand.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time_population as tp  # noqa: E402  (expneg and Philox restated in numpy)
from annealing_sign_problem_amd import _lib, build, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

STATE = tp.STATE


def law_source(energies, betas, parity, seed, sweeps_done, draw):
    """ASP-PT-1, steps 2-5."""
    R = energies.shape[0]
    source = np.arange(R, dtype=np.int64)
    ks = np.arange(parity, R - 1, 2)
    if ks.size == 0:
        return source
    x = (betas[ks + 1] - betas[ks]) * (energies[ks] - energies[ks + 1])
    p = tp.expneg(np.maximum(x, 0.0))
    for k, cost, threshold in zip(ks, x, p):
        swap = cost <= 0.0
        if not swap and cost < 23.0:
            word = tp.philox_word0((int(k), sweeps_done, 0xFFFFFFFC, draw), (seed & 0xFFFFFFFF, seed >> 32))
            swap = (word + 0.5) * 2.0 ** -32 < threshold
        if swap:
            source[k], source[k + 1] = k + 1, k
    return source


def spread(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def same(a, b):
    return all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in STATE)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=3000)
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--sweeps", type=int, default=10)
    p.add_argument("--repeat", type=int, default=5)
    a = p.parse_args()
    lib = _lib.load()
    print("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
    print("K=%d chains=%d, segments of %d sweeps, repeat=%d" % (a.size, a.chains, a.sweeps, a.repeat), flush=True)
    J, h, _ = synthetic.planted_cluster(a.size, seed=1000)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, a.chains)
    middle = float(ladder[a.chains // 2])
    plan = ham.plan()
    chains = sa.Chains(ham, seed=1, repetitions=a.chains)
    chains.advance_ladder(ladder, 16, sweep_order="shuffled")
    snapshot = chains.state()

    def timed(call):
        chains.load_state(snapshot)
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, float(lib.asp_sa_last_sweep_ms(plan)), float(lib.asp_sa_last_total_ms(plan)), chains.state()

    for order in ("colour", "shuffled"):
        runs = {
            "advance, constant beta": lambda: chains.advance(np.full(a.sweeps, middle), sweep_order=order),
            "advance_ladder, equal betas": lambda: chains.advance_ladder(np.full(a.chains, middle), a.sweeps,
                                                                         sweep_order=order),
            "advance_ladder, geometric ladder": lambda: chains.advance_ladder(ladder, a.sweeps, sweep_order=order),
        }
        figures = {name: [] for name in runs}
        for k in range(a.repeat + 1):
            states = {}
            for name, call in runs.items():
                wall, sweep_ms, total_ms, states[name] = timed(call)
                if k:  # (the first round warms up)
                    figures[name].append((wall, sweep_ms, total_ms))
            if not same(states["advance, constant beta"], states["advance_ladder, equal betas"]):
                raise SystemExit("a ladder segment with equal betas and advance do NOT agree (%s)" % order)
        print("(a) %s order" % order)
        for name, rows in figures.items():
            wall, sweep_ms, total_ms = zip(*rows)
            print("    %-33s: sweep launches %s  segment %s  wall %s" % (name, spread(sweep_ms), spread(total_ms),
                                                                        spread(wall)), flush=True)

    walls_a, devices_a, walls_b = [], [], []
    swaps = 0
    for k in range(a.repeat + 1):
        wall, _, device, after = timed(lambda: chains.exchange(ladder, 0, 0))
        chains.load_state(snapshot)
        t0 = time.perf_counter()
        state = chains.state()
        energies = ham.energies(state["x_current"])
        source = law_source(energies, ladder, 0, chains.seed, int(state["sweeps_done"]), 0)
        moved = {name: np.ascontiguousarray(state[name][source]) for name in STATE}
        moved["sweeps_done"] = state["sweeps_done"]
        chains.load_state(moved)
        wall_b = (time.perf_counter() - t0) * 1e3
        if not same(chains.state(), after):
            raise SystemExit("the host route and asp_sa_chains_exchange do NOT agree")
        swaps = int(np.count_nonzero(source != np.arange(a.chains))) // 2
        if k:
            walls_a.append(wall)
            devices_a.append(device)
            walls_b.append(wall_b)
    print("(b) exchange step, parity 0: %d of %d pairs swapped" % (swaps, a.chains // 2))
    print("    asp_sa_chains_exchange            : wall %s  device %s" % (spread(walls_a), spread(devices_a)))
    print("    export, numpy, import             : wall %s  device NOT MEASURED (no single device span)" % spread(walls_b))
    chains.close()


if __name__ == "__main__":
    main()
