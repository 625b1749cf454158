"""Cost of segmenting an anneal (asp_sa_chains): the reference's default call — a
planted cluster of K = 1e4 spins, 64 chains x 5120 sweeps — as one closed call, as one `advance` of
all sweeps, and cut into 10 segments of 512 and 80 segments of 64 sweeps, in both visiting orders.

    python tools/time_chains.py [--size 10000] [--chains 64] [--sweeps 5120] [--segments 1,10,80]
                                [--repeat 3] [--orders colour,shuffled]

Per case: wall time of the whole run (create .. result included) and device time (the plan's
asp_sa_last_total_ms summed over the segments: permutes / state loads, sweep and order kernels, copies
between the handle and the work buffers), median and spread over --repeat runs after a warm-up; every
segmented run is compared with the closed call bit for bit first.  With ASP_LIB_TAG set (and
ASP_NO_REBUILD=1) the library is an older tagged build without the handle: only the closed call is
timed — the yardstick of the same session.  Output goes to profiles/chains_timing.txt by hand.

    python tools/time_chains.py --batch 64 [--size 3000] [--chains 64] [--sweeps 5120] [--segment 512]

Batch mode (asp_sa_chains_advance_batch): --batch handles of distinct planted clusters of --size spins,
the ladder in segments of --segment sweeps, (a) all handles per segment in one advance_chains call,
(b) the same handles advanced one by one (the only route before the batched call), (c) the closed
asp_sa_anneal_batch on the same problems; wall times, in both orders, (a) and (b) checked against (c)
bit for bit.
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


def spread(values):
    return "%9.2f ms (min %.2f, max %.2f)" % (statistics.median(values), min(values), max(values))


def batch_mode(a):
    problems = [synthetic.planted_cluster(a.size, seed=1000 + k)[:2] for k in range(a.batch)]
    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    ladders = [sa.make_schedule(h.info().beta0_auto, h.info().beta1_auto, a.sweeps) for h in hams]
    print("batch of %d clusters, K=%d chains=%d sweeps=%d segments of %d repeat=%d" % (
        a.batch, a.size, a.chains, a.sweeps, a.segment, a.repeat), flush=True)
    for order in a.orders.split(","):
        shuffled = order == "shuffled"
        timings = {"c closed batch": [], "a batched segments": [], "b one handle at a time": []}
        for k in range(a.repeat + 1):
            t0 = time.perf_counter()
            closed = sa.anneal_batch_raw(hams, [1] * a.batch, ladders, [a.chains] * a.batch, shuffled=shuffled)
            wall_c = (time.perf_counter() - t0) * 1e3
            walls = {}
            for name in ("a batched segments", "b one handle at a time"):
                t0 = time.perf_counter()
                handles = [sa.Chains(h, seed=1, repetitions=a.chains) for h in hams]
                for first in range(0, a.sweeps, a.segment):
                    parts = [ladder[first:first + a.segment] for ladder in ladders]
                    if name.startswith("a"):
                        sa.advance_chains(handles, parts, sweep_order=order, progress=True)
                    else:
                        for c, part in zip(handles, parts):
                            c.advance(part, sweep_order=order)
                results = [c.result() for c in handles]
                for c in handles:
                    c.close()
                walls[name] = (time.perf_counter() - t0) * 1e3
                for (xs, es), (cxs, ces) in zip(results, closed):
                    if not (np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes()):
                        raise SystemExit("%s, %s: NOT the closed batch's chains" % (order, name))
            if k:  # (the first round warms up)
                timings["c closed batch"].append(wall_c)
                for name, wall in walls.items():
                    timings[name].append(wall)
        for name in ("a batched segments", "b one handle at a time", "c closed batch"):
            print("%-8s (%s): wall %s" % (order, name, spread(timings[name])), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=0, help="batch mode: this many handles (see the module's text)")
    p.add_argument("--segment", type=int, default=512)
    p.add_argument("--size", type=int, default=None, help="spins (default 10000; batch mode 3000)")
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--sweeps", type=int, default=5120)
    p.add_argument("--segments", default="1,10,80")
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--orders", default="colour,shuffled")
    a = p.parse_args()
    if a.batch:
        a.size = 3000 if a.size is None else a.size
        _lib.load()
        print("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
        return batch_mode(a)
    a.size = 10000 if a.size is None else a.size
    lib = _lib.load()
    has_chains = hasattr(lib, "asp_sa_chains_create")
    print("library %s fingerprint %s%s" % (os.path.basename(_lib.library_path()), build.built_fingerprint(),
                                           "" if has_chains else "  (no chains handle: closed calls only)"))
    J, h, _ = synthetic.planted_cluster(a.size, seed=783494)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, a.sweeps)
    print("K=%d nnz/K=%.1f chains=%d sweeps=%d repeat=%d" % (a.size, J.nnz / a.size, a.chains, a.sweeps, a.repeat),
          flush=True)
    for order in a.orders.split(","):
        shuffled = order == "shuffled"
        walls, devices = [], []
        for k in range(a.repeat + 1):
            t0 = time.perf_counter()
            xs, es = sa.anneal_raw(ham, 1, betas, a.chains, shuffled=shuffled)
            wall = (time.perf_counter() - t0) * 1e3
            if k:  # (the first run warms up: plan buffers, the shuffled order's static tables)
                walls.append(wall)
                devices.append(lib.asp_sa_last_total_ms(ham.plan()))
        print("%-8s closed call          : wall %s  device %s" % (order, spread(walls), spread(devices)), flush=True)
        if not has_chains:
            continue
        for count in [int(s) for s in a.segments.split(",")]:
            size = (a.sweeps + count - 1) // count
            walls, devices = [], []
            for k in range(a.repeat + 1):
                device = 0.0
                t0 = time.perf_counter()
                with sa.Chains(ham, seed=1, repetitions=a.chains) as chains:
                    for first in range(0, a.sweeps, size):
                        chains.advance(betas[first:first + size], sweep_order=order)
                        device += lib.asp_sa_last_total_ms(ham.plan())
                    cxs, ces = chains.result()
                wall = (time.perf_counter() - t0) * 1e3
                if not (np.array_equal(cxs, xs) and ces.tobytes() == es.tobytes()):
                    raise SystemExit("%s, %d segments: NOT the closed call's chains" % (order, count))
                if k:
                    walls.append(wall)
                    devices.append(device)
            print("%-8s %3d segments of %4d : wall %s  device %s" % (order, count, size, spread(walls), spread(devices)),
                  flush=True)


if __name__ == "__main__":
    main()
