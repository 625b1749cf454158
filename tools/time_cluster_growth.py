"""The device growth of a round of sampled clusters (grow_clusters, asp_operator_grow_segments, specification
ASP-GROW-1) beside the host growth (create_small_cluster_around_point, one cluster after the other,
in place, ONE process): rounds of 256 / 1024 / 4096 clusters with the driver's defaults (seeds ~ |psi|^0.1, sizes
log-uniform in [50, 1000], keep probability 0.5).  Timed is the growth alone: seeds and sizes are drawn beforehand.
The two routes grow DIFFERENT clusters of the same law, so the tool also prints the two size distributions and the
greedy accuracy / overlap (order 0) of 256 clusters grown each way.  heisenberg_kagome_36 where its ground state can
be computed (sector_ed, ~12 s on an MI355X) or is given with --hdf5; otherwise the 16- and 18-site models.
(Development aid; GPU.)

    python tools/time_cluster_growth.py [--runs 3] [--hdf5 FILE] [--small] [--out profiles/cluster_growth_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from annealing_sign_problem_amd import _lib, common, operators, synthetic  # noqa: E402
from annealing_sign_problem_amd import sampled_components as sc  # noqa: E402

ROUNDS = (256, 1024, 4096)
SCORED = 256
POWER, SMALL, LARGE, KEEP = 0.1, 50, 1000, 0.5


def load(name, hdf5):
    op = operators.Operator.from_config(synthetic.load_models()[name])
    if hdf5:
        args = argparse.Namespace(model=name, yaml=None, hdf5=hdf5)
        return sc.load_input(args)
    if op.basis.number_spins > 20:
        from annealing_sign_problem_amd import sector_ed

        _, psi, reps, _ = sector_ed.ground_state(op)
        op.basis.build(reps)
        return op, psi
    op.basis.build()
    return op, op.ground_state()[1]


def deciles(sizes):
    return " ".join("%d" % q for q in np.percentile(sizes, [0, 10, 25, 50, 75, 90, 100]).round().astype(int))


def scores(clusters, op, psi, log_psi):
    rows = [sc.process_cluster(c, op, psi, psi, log_psi, 0, 1e-4, False)[0] for c in clusters]
    accuracy = np.array([r.greedy_accuracy for r in rows])
    overlap = np.array([r.greedy_overlap for r in rows])
    return "greedy accuracy median %.4f mean %.4f, overlap median %.4f mean %.4f" % (
        np.median(accuracy), accuracy.mean(), np.median(overlap), overlap.mean())


def measure(name, op, psi, runs, emit):
    device = op.device()
    log_psi = common.ground_state_to_log_coeff_fn(psi, op.basis)
    emit("%s: %d basis states, %d connections per state at most" % (name, op.basis.number_states,
                                                                   device.max_connections))
    first = {}
    for n in ROUNDS:
        np.random.seed(435834)
        seeds = np.asarray(common.monte_carlo_sampling(op.basis.states, psi, number_samples=n,
                                                       sampled_power=POWER).spins, dtype=np.uint64)
        sizes = np.array([sc.random_cluster_size(SMALL, LARGE) for _ in range(n)], dtype=np.uint64)
        philox_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        # the device route: a warm-up call (code objects, pooled buffers), then `runs` timed calls
        grown, passes = device.grow_segments(seeds, sizes, KEEP, philox_seed)
        wall, on_device = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            again = sc.grow_clusters(op, seeds, sizes, KEEP, philox_seed)
            wall.append((time.perf_counter() - t0) * 1e3)
            on_device.append(device.last_ms)
            assert all(np.array_equal(a, b) for a, b in zip(again, grown))
        # the host route of the parent commit, in place, one process (its draws: numpy's legacy stream)
        np.random.seed(435835)
        sc.create_small_cluster_around_point(int(seeds[0]), op, required_size=int(sizes[0]), keep_probability=KEEP)
        t0 = time.perf_counter()
        hosted = [np.asarray(sc.create_small_cluster_around_point(int(s), op, required_size=int(r),
                                                                  keep_probability=KEEP), dtype=np.uint64)
                  for s, r in zip(seeds, sizes)]
        host_ms = (time.perf_counter() - t0) * 1e3
        device_ms = statistics.median(wall)
        emit("  %d clusters, %d states wanted" % (n, int(sizes.sum())))
        emit("    device, one grow_clusters call   wall %9.2f ms (min %.2f, max %.2f)   launches %.2f ms   "
             "%d passes (segments: median %d)" % (device_ms, min(wall), max(wall), statistics.median(on_device),
                                                  int(passes.max()), int(np.median(passes))))
        emit("    host, cluster after cluster      wall %9.2f ms (one run)   = %.3f ms per cluster" % (
            host_ms, host_ms / n))
        emit("    host / device: %.2fx" % (host_ms / device_ms))
        emit("    sizes grown (min 10%% 25%% 50%% 75%% 90%% max): device %s (%d states) | host %s (%d states) | wanted %s"
             % (deciles([c.size for c in grown]), sum(c.size for c in grown), deciles([c.size for c in hosted]),
                sum(c.size for c in hosted), deciles(sizes)))
        emit("    clusters below their wanted size: device %d, host %d" % (
            sum(c.size < r for c, r in zip(grown, sizes)), sum(c.size < r for c, r in zip(hosted, sizes))))
        if n == SCORED:
            first = {"device": grown, "host": hosted}
    for route in ("device", "host"):
        emit("  %d clusters grown on the %s, order 0: %s" % (SCORED, route, scores(first[route], op, psi, log_psi)))
    emit("")


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--runs", type=int, default=3)
    parser.add_argument("--hdf5", type=str, default=None, help="ground state of heisenberg_kagome_36 (SpinED output)")
    parser.add_argument("--small", action="store_true", help="the 16- and 18-site models instead of kagome_36")
    parser.add_argument("--out", type=str, default=os.path.join("profiles", "cluster_growth_timing.txt"))
    args = parser.parse_args()
    _lib.require_gpu()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("tools/time_cluster_growth.py --runs %d%s" % (args.runs, " --small" if args.small else ""))
    emit("wall: the Python call, uploads and downloads included, median of the runs after a warm-up call; launches: "
         "asp_operator_last_ms (HIP events around the passes).  Seeds and sizes are drawn beforehand; the two routes "
         "grow different clusters of the same law.")
    emit("")
    names = ["heisenberg_kagome_16", "heisenberg_kagome_18"]
    if not args.small:
        try:
            t0 = time.perf_counter()
            op, psi = load("heisenberg_kagome_36", args.hdf5)
            emit("heisenberg_kagome_36: ground state in %.1f s" % (time.perf_counter() - t0))
            measure("heisenberg_kagome_36", op, psi, args.runs, emit)
            names = []
        except Exception as error:  # noqa: BLE001 - reported, and the small models are measured instead
            emit("heisenberg_kagome_36: no ground state (%s: %s); the 16- and 18-site models instead" % (
                type(error).__name__, error))
    for name in names:
        op, psi = load(name, None)
        measure(name, op, psi, args.runs, emit)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
