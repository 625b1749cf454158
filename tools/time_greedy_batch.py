"""One greedy_solve_batch call against the loops it replaces, plans built beforehand:
  (a) a loop of greedy_solve, one problem after the other;
  (b) the same loop on 16 host threads, as sampled_components --jobs 16 runs it;
  (c) ONE greedy_solve_batch call, with its host-tree and device-descent times apart.
Problems: the batch-tuning mix of DESIGN.md §5.5 (N planted clusters, K log-uniform in [1e2, 1e4],
the seeds of tools/time_shuffled_batch_only.py) for every N given, and — with --hdf5 FILE, the
ground state of heisenberg_kagome_36 — the models of every order up to 2 of one round of sampled
clusters.  Median wall time of REPEAT repetitions after a warm-up of each variant; (a), (b) and
(c) of a repetition run back to back, so they see the same machine.  (c)'s results are compared
with (a)'s bit for bit before anything is timed.  (Development aid; GPU.)

    python tools/time_greedy_batch.py [--repeat 7] [--hdf5 FILE [--clusters 64]] [N ...] (default 128 512)
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from annealing_sign_problem_amd import annealer as sa  # noqa: E402
from annealing_sign_problem_amd import _lib, greedy, synthetic  # noqa: E402

THREADS = 16


def planted_mix(n):
    rng = np.random.default_rng(783494)
    sizes = [int(round(np.exp(rng.uniform(np.log(1e2), np.log(1e4))))) for _ in range(n)]
    hams = []
    for i, k in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(k, seed=783494 + i)
        hams.append(sa.Hamiltonian(J, h))
    return hams


def real_round(hdf5, clusters):
    """The models (orders 0..2, cutoff 1e-6: `make kagome_36`) of one round of sampled clusters."""
    from annealing_sign_problem_amd import common
    from annealing_sign_problem_amd import sampled_components as sc

    args = argparse.Namespace(model="heisenberg_kagome_36", yaml=None, hdf5=hdf5)
    hamiltonian, ground_state = sc.load_input(args)
    np.random.seed(435834)
    log_fn = common.ground_state_to_log_coeff_fn(ground_state, hamiltonian.basis)
    some = sc.generate_clusters(hamiltonian, ground_state, clusters, 0.1, 50, 1000, 0.5)
    hams = []
    for cluster in some:
        h = common.make_ising_model(cluster, hamiltonian, log_psi_fn=log_fn)
        hams.append(h.ising_hamiltonian)
        for _ in range(2):
            h = common.make_hamiltonian_extension(h, log_fn)
            h = common.sparsify_using_global_cutoff(h, 1e-6, cluster)
            hams.append(h.ising_hamiltonian)
    return hams


def measure(label, hams, repeat):
    for ham in hams:
        ham.plan()  # plans are built beforehand in all three variants
    sizes = [ham.size for ham in hams]

    def loop():
        return [greedy.greedy_solve(ham) for ham in hams]

    def threaded():
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            return list(pool.map(greedy.greedy_solve, hams))

    def batch():
        return greedy.greedy_solve_batch(hams)

    # warm-up of every variant (code objects, streams, pooled buffers) and the parity check
    reference = loop()
    threaded()
    got = greedy.greedy_solve_batch(hams, return_sweeps=True)
    for (x, e), (bx, be, _) in zip(reference, got):
        if not (np.array_equal(x, bx) and np.float64(e).tobytes() == np.float64(be).tobytes()):
            raise SystemExit("greedy_solve_batch differs from greedy_solve: timing refused")
    sweeps = [t for _, _, t in got]
    batch()
    times = {"a": [], "b": [], "c": [], "tree": [], "descent": []}
    for _ in range(repeat):
        for key, fn in (("a", loop), ("b", threaded), ("c", batch)):
            t0 = time.perf_counter()
            fn()  # every call ends in a stream synchronise
            times[key].append((time.perf_counter() - t0) * 1e3)
        tree, descent = greedy.last_batch_ms()
        times["tree"].append(tree)
        times["descent"].append(descent)
    med = {k: statistics.median(v) for k, v in times.items()}
    n = len(hams)
    print("%s: %d problems, K %d..%d (sum %d), descent sweeps t %d..%d (sum %d), %d repetitions" % (
        label, n, min(sizes), max(sizes), sum(sizes), min(sweeps), max(sweeps), sum(sweeps), repeat))
    for key, name in (("a", "(a) loop of greedy_solve            "),
                      ("b", "(b) the loop on %d threads           " % THREADS),
                      ("c", "(c) one greedy_solve_batch call      ")):
        print("  %s %9.2f ms  = %7.3f ms per problem   (min %.2f, max %.2f)" % (
            name, med[key], med[key] / n, min(times[key]), max(times[key])))
    print("      of (c): host trees (pool of <= 8 threads) %.2f ms, descent launches on the device %.2f ms, "
          "rest (descriptors, copies, energies) %.2f ms" % (
              med["tree"], med["descent"], med["c"] - med["tree"] - med["descent"]))
    print("      (c) against (a): %.2fx, against (b): %.2fx" % (med["a"] / med["c"], med["b"] / med["c"]),
          flush=True)
    for ham in hams:
        ham.release()


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--repeat", type=int, default=7)
    parser.add_argument("--hdf5", type=str, default=None)
    parser.add_argument("--clusters", type=int, default=64)
    parser.add_argument("sizes", type=int, nargs="*", default=[128, 512])
    args = parser.parse_args()
    if args.repeat < 5:
        raise SystemExit("--repeat must be at least 5")
    _lib.require_gpu()
    for n in args.sizes:
        measure("planted mix", planted_mix(n), args.repeat)
    if args.hdf5 is None:
        print("real order-2 models: skipped (no --hdf5 ground-state file given)")
    elif not os.path.exists(args.hdf5):
        print("real order-2 models: skipped (%s not found)" % args.hdf5)
    else:
        measure("kagome_36 round of %d clusters" % args.clusters, real_round(args.hdf5, args.clusters),
                args.repeat)


if __name__ == "__main__":
    main()
