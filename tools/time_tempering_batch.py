"""One round of parallel tempering — a ladder segment plus an exchange step — for MANY handles, on two
routes (DESIGN.md §4.12 "Batched forms"), in both sweep orders.

    python tools/time_tempering_batch.py [--handles 64] [--chains 64] [--sweeps 10] [--repeat 5]
                                         [--min-size 500] [--max-size 3000] [--singles-only]

(a) N single calls: Chains.advance_ladder then Chains.exchange per handle — the code path of the commit
    before the batched forms, unchanged by them (--singles-only runs on that commit too);
(b) the two batched calls: advance_ladder_chains and exchange_chains over all handles.
Workload: --handles planted clusters with sizes spread log-uniformly over [--min-size, --max-size],
--chains chains each on the automatic geometric ladder.  Every timed round starts from the same snapshots
(load_state, not timed); the two routes are checked to leave the same bits first.  Wall time of the
segment, of the exchange and of the round — median and spread over --repeat rounds after a warm-up — and
for route (b) the device time of the sweep launches (asp_sa_chains_batch_last_ms) and of the exchange
(asp_sa_chains_exchange_last_ms).  Output goes to profiles/tempering_batch_timing.txt by hand.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import _lib, build, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def spread(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def same(a, b):
    return all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in STATE)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--handles", type=int, default=64)
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--sweeps", type=int, default=10)
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--min-size", type=int, default=500)
    p.add_argument("--max-size", type=int, default=3000)
    p.add_argument("--singles-only", action="store_true", help="route (a) only: runs without the batched forms")
    a = p.parse_args()
    lib = _lib.load()
    print("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
    sizes = [int(n) for n in np.geomspace(a.min_size, a.max_size, a.handles)]
    print("%d clusters of %d..%d spins (%d in all), %d chains each, segments of %d sweeps, repeat=%d" % (
        a.handles, min(sizes), max(sizes), sum(sizes), a.chains, a.sweeps, a.repeat), flush=True)
    hams, ladders, handles, snapshots = [], [], [], []
    for k, n in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(n, seed=1000 + k)
        ham = sa.Hamiltonian(J, h)
        info = ham.info()
        hams.append(ham)
        ladders.append(sa.make_schedule(info.beta0_auto, info.beta1_auto, a.chains))
        handles.append(sa.Chains(ham, seed=1 + k, repetitions=a.chains))
    for order in ("colour", "shuffled"):
        for c, ladder in zip(handles, ladders):
            c.advance_ladder(ladder, 4, sweep_order=order)
        snapshots = [c.state() for c in handles]

        def restore():
            for c, s in zip(handles, snapshots):
                c.load_state(s)

        def singles():
            t0 = time.perf_counter()
            for c, ladder in zip(handles, ladders):
                c.advance_ladder(ladder, a.sweeps, sweep_order=order)
            t1 = time.perf_counter()
            for c, ladder in zip(handles, ladders):
                c.exchange(ladder, 0, 0)
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3

        def batched():
            t0 = time.perf_counter()
            sa.advance_ladder_chains(handles, ladders, a.sweeps, sweep_order=order)
            t1 = time.perf_counter()
            sweep_ms = float(lib.asp_sa_chains_batch_last_ms())
            sa.exchange_chains(handles, ladders, 0, 0)
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, sweep_ms, float(lib.asp_sa_chains_exchange_last_ms())

        routes = {"(a) N single calls": singles}
        if not a.singles_only:
            routes["(b) two batched calls"] = batched
        figures = {name: [] for name in routes}
        for k in range(a.repeat + 1):
            ends = {}
            for name, call in routes.items():
                restore()
                row = call()
                ends[name] = [c.state() for c in handles]
                if k:  # (the first round warms up)
                    figures[name].append(row)
            if len(ends) == 2:
                first, second = ends.values()
                if not all(same(x, y) for x, y in zip(first, second)):
                    raise SystemExit("the two routes do NOT leave the same bits (%s)" % order)
        print("%s order" % order)
        for name, rows in figures.items():
            columns = list(zip(*rows))
            line = "    %-22s: segment wall %s  exchange wall %s  round wall %s" % (
                name, spread(columns[0]), spread(columns[1]), spread(columns[2]))
            if len(columns) > 3:
                line += "\n    %-22s  sweep launches (device) %s  exchange (device) %s" % (
                    "", spread(columns[3]), spread(columns[4]))
            else:
                line += "\n    %-22s  device spans NOT MEASURED (one per handle, no span of the round)" % ""
            print(line, flush=True)
        if len(figures) == 2:
            med = {name: statistics.median(list(zip(*rows))[2]) for name, rows in figures.items()}
            names = list(med)
            print("    round, (a) / (b): %.2f" % (med[names[0]] / med[names[1]]), flush=True)
    for c in handles:
        c.close()


if __name__ == "__main__":
    main()
