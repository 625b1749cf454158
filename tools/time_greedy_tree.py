"""The greedy solver's strongest-coupling tree on the host (the pool of at most 8 threads inside
asp_sa_greedy_batch) against the same tree on the device (asp_sa_set_greedy_tree), plans
built beforehand, for three workloads:
  (1) 64 planted clusters of 500 .. 3000 spins;
  (2) 24 planted models of 3e4 .. 2e5 spins at mean degree ~10 (the shape of the order-2 models);
  (3) one model of 1.77e5 spins alone.
Per workload and side: tree time (asp_sa_greedy_batch_last_ms's tree_ms: host wall time of the pool plus
device time of the tree launches) and wall time of the whole asp_sa_greedy_batch call, RUNS alternating runs
per side after a warm-up of both (median, min .. max); the device time split into bonds + sort,
k_greedy_tree and orientation + packing.  The device results are compared with the host's bit for bit
before anything is timed.  Then the wall time of `sampled_components --greedy-batch` on
heisenberg_kagome_16 with both trees.  Writes --output (default profiles/greedy_tree_timing.txt).
(Development aid; GPU.)

    python tools/time_greedy_tree.py [--runs 3] [--large 24] [--output FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from annealing_sign_problem_amd import annealer as sa  # noqa: E402
from annealing_sign_problem_amd import _lib, greedy, synthetic  # noqa: E402


def planted(sizes, seed, mean_degree, max_degree):
    hams = []
    for i, k in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(int(k), seed=seed + i, mean_degree=mean_degree, max_degree=max_degree)
        hams.append(sa.Hamiltonian(J, h))
    return hams


def workloads(large):
    rng = np.random.default_rng(783494)
    small = [int(round(np.exp(rng.uniform(np.log(500.0), np.log(3000.0))))) for _ in range(64)]
    big = [int(round(np.exp(rng.uniform(np.log(3e4), np.log(2e5))))) for _ in range(large)]
    yield "64 planted clusters of 500 .. 3000 spins (mean degree 23)", lambda: planted(small, 1000, 23.0, 37)
    yield "%d planted models of 3e4 .. 2e5 spins (mean degree 10)" % large, lambda: planted(big, 2000, 10.0, 20)
    yield "one model of 1.77e5 spins alone (mean degree 10)", lambda: planted([177000], 3000, 10.0, 20)


def spread(values):
    return "%9.2f ms (min %.2f, max %.2f)" % (statistics.median(values), min(values), max(values))


def measure(label, hams, runs, out):
    for ham in hams:
        ham.plan()
    sizes = [ham.size for ham in hams]
    bonds = sum(ham.exchange.nnz for ham in hams) // 2

    def run(tree):
        t0 = time.perf_counter()
        got = greedy.greedy_solve_batch(hams, return_sweeps=True, tree=tree)
        wall = (time.perf_counter() - t0) * 1e3
        return got, wall, greedy.last_batch_ms()[0], greedy.last_tree_ms()

    host, _, _, _ = run("host")  # warm-up of both sides and the parity check
    device, _, _, _ = run("device")
    for (x, e, t), (y, f, u) in zip(host, device):
        if not (np.array_equal(x, y) and np.float64(e).tobytes() == np.float64(f).tobytes() and t == u):
            raise SystemExit("the device tree changes a result: timing refused")
    times = {side: {"wall": [], "tree": [], "split": []} for side in ("host", "device")}
    for _ in range(runs):
        for side in ("host", "device"):
            _, wall, tree_ms, split = run(side)
            times[side]["wall"].append(wall)
            times[side]["tree"].append(tree_ms)
            times[side]["split"].append(split)
    out.append("%s: %d problems, K %d..%d (sum %d), ~%d bonds, %d alternating runs per side" % (
        label, len(hams), min(sizes), max(sizes), sum(sizes), bonds, runs))
    for side in ("host", "device"):
        out.append("  %-6s tree: tree_ms %s   whole asp_sa_greedy_batch %s" % (
            side, spread(times[side]["tree"]), spread(times[side]["wall"])))
    split = times["device"]["split"]
    out.append("    device tree launches: bonds + sort %s, k_greedy_tree %s, orientation + packing %s" % tuple(
        spread([s[q] for s in split]) for q in (1, 2, 3)))
    out.append("    device / host: tree %.2fx, whole call %.2fx" % (
        statistics.median(times["device"]["tree"]) / statistics.median(times["host"]["tree"]),
        statistics.median(times["device"]["wall"]) / statistics.median(times["host"]["wall"])))
    print("\n".join(out[-5:]), flush=True)
    for ham in hams:
        ham.release()


def pipeline(runs, out):
    from annealing_sign_problem_amd import sampled_components

    args = ["--model", "heisenberg_kagome_16", "--order", "2", "--number-samples", "7", "--seed", "99",
            "--max-cluster-size", "300", "--no-annealing", "--batch", "4", "--greedy-batch"]
    times = {"host": [], "device": []}
    texts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(runs + 1):  # (the first pass of both sides is the warm-up)
            for side in ("host", "device"):
                path = os.path.join(tmp, "%s_%d.csv" % (side, r))
                t0 = time.perf_counter()
                sampled_components.main(args + ["--output", path, "--greedy-tree", side])
                if r:
                    times[side].append((time.perf_counter() - t0) * 1e3)
                with open(path, "rb") as f:
                    texts[side] = f.read()
    if texts["host"] != texts["device"]:
        raise SystemExit("sampled_components writes another file with the device tree")
    out.append("sampled_components --greedy-batch on heisenberg_kagome_16 (%s), wall time, %d alternating runs per "
               "side, the same file:" % (" ".join(args[2:]), runs))
    for side in ("host", "device"):
        out.append("  --greedy-tree %-6s %s" % (side, spread(times[side])))
    print("\n".join(out[-3:]), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--runs", type=int, default=3)
    parser.add_argument("--large", type=int, default=24)
    parser.add_argument("--output", type=str, default=os.path.join(ROOT, "profiles", "greedy_tree_timing.txt"))
    args = parser.parse_args()
    if args.runs < 3:
        raise SystemExit("--runs must be at least 3")
    _lib.require_gpu()
    out = ["tools/time_greedy_tree.py --runs %d --large %d" % (args.runs, args.large),
           "host tree: greedy_tree_signs on the pool of <= 8 threads inside asp_sa_greedy_batch (where = 0, the code "
           "of the parent commit); device tree: where = 1 (csrc/greedy_tree.hip)", ""]
    for label, make in workloads(args.large):
        measure(label, make(), args.runs, out)
        out.append("")
    pipeline(args.runs, out)
    with open(args.output, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.output)


if __name__ == "__main__":
    main()
