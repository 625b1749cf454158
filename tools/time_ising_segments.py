"""Wall time and device time of the coupling build of a ROUND of clusters: ONE segmented call
(asp_operator_ising_segments) beside the loop of asp_operator_ising_csr calls over the same clusters — the
per-cluster code path, unchanged in the same library — on 1 and on 16 host threads.

Rounds of 64, 256 and 1024 clusters, grown as the pipeline grows them (create_small_cluster_around_point, log-uniform
50 ... 1000 states, keep probability 0.5) from random basis states, at order-0 table sizes (the clusters) and order-1
table sizes (their one-hop extensions), on heisenberg_kagome_16 (plain basis: k_ising_rows_seg) and on a
symmetry-adapted model (k_merge_rows_seg / k_sym_rows_seg): heisenberg_kagome_36's sector when its ground-state file
--hdf5 is present, heisenberg_kagome_18 otherwise.  Amplitudes are hashed from the keys and normalised per cluster.
Every timing comes after a warm-up call: median (min .. max) over --runs >= 5 repetitions.  The results of the two
routes are compared, indices and bits, before anything is timed.

Then sampled_components on 256 clusters of heisenberg_kagome_16 at order 1 with the greedy solver (--no-annealing
--greedy-batch --jobs 16), with and without --build-batch, three runs each; all six CSV files are compared byte for
byte.

Every step runs in a child process of its own under its own time limit, at most 16 host threads; the first step that
fails ends the run.  Writes --output (default profiles/ising_segments_timing.txt).  (Development aid; GPU.)

    python tools/time_ising_segments.py [--runs 5] [--output FILE] [--hdf5 heisenberg_kagome_36.h5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS = 16
ROUNDS = (64, 256, 1024)
STEP_LIMIT = 420   # seconds per measuring step
PIPELINE_LIMIT = 300


def amplitudes(keys):
    """Hashed positive amplitudes over a few decades."""
    h = (keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return np.exp(-6.0 * h.astype(np.float64) / float(1 << 24)) + 1e-3


def stats(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def build_round(op, count, order, seed):
    """`count` clusters as the pipeline grows them; order 1: their one-hop extensions."""
    from annealing_sign_problem_amd import common, sampled_components

    rng = np.random.default_rng(seed)
    np.random.seed(seed)  # (the growth draws from numpy's global stream)
    states = op.basis.states
    clusters = []
    for start in rng.choice(states, size=count, replace=True).tolist():
        size = sampled_components.random_cluster_size(50, 1000)
        cluster = np.asarray(sampled_components.create_small_cluster_around_point(
            int(start), op, required_size=size, keep_probability=0.5), dtype=np.uint64)
        clusters.append(common.extension_spins(op, cluster) if order == 1 else cluster)
    return clusters


def step(model, hdf5, order, count, runs):
    """One (model, order, round) measurement; prints one JSON line."""
    from concurrent.futures import ThreadPoolExecutor

    from annealing_sign_problem_amd import operators, synthetic

    op = operators.Operator.from_config(synthetic.load_models()[model])
    if hdf5:
        from annealing_sign_problem_amd import common

        _, _, representatives = common.load_ground_state(hdf5)
        op.basis.build(np.sort(representatives))
    else:
        op.basis.build()
    device = op.device()
    clusters = build_round(op, count, order, 1000 * order + count)
    psis = []
    for c in clusters:
        psi = amplitudes(c)
        psis.append(psi / np.linalg.norm(psi))
    keys, psi = np.concatenate(clusters), np.concatenate(psis)
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clusters])]).astype(np.uint64)

    def one(g):
        out = device.ising_csr(clusters[g], psis[g])
        return out, device.last_ms

    def loop(threads):
        started = time.perf_counter()
        if threads == 1:
            parts = [one(g) for g in range(count)]
        else:
            with ThreadPoolExecutor(max_workers=threads) as pool:
                parts = list(pool.map(one, range(count)))
        return 1e3 * (time.perf_counter() - started), parts

    def segmented():
        started = time.perf_counter()
        out = device.ising_csr_segments(keys, psi, offsets)
        return 1e3 * (time.perf_counter() - started), out, device.last_ms

    # warm-up, and the two routes agree: indices equal, values as bits
    _, (indptr, col, val), _ = segmented()
    _, parts = loop(1)
    loop(THREADS)
    at = 0
    for g, ((ip, c, v), _) in enumerate(parts):
        first, last = int(offsets[g]), int(offsets[g + 1])
        assert np.array_equal(indptr[first:last + 1] - indptr[first], ip), "indptr differs in segment %d" % g
        assert np.array_equal(col[at:at + c.size], c) and val[at:at + v.size].tobytes() == v.tobytes(), g
        at += c.size
    assert at == col.size
    result = {"model": model, "order": order, "clusters": count, "rows": int(keys.size), "couplings": int(col.size),
              "unique_targets": bool(device.unique_targets), "runs": runs}
    wall, ms = [], []
    for _ in range(runs):
        w, _, m = segmented()
        wall.append(w)
        ms.append(m)
    result["segmented_wall"], result["segmented_ms"] = wall, ms
    for threads in (1, THREADS):
        wall, ms = [], []
        for _ in range(runs):
            w, parts = loop(threads)
            wall.append(w)
            ms.append(sum(m for _, m in parts))
        result["loop%d_wall" % threads], result["loop%d_ms" % threads] = wall, ms
    print("RESULT " + json.dumps(result), flush=True)


def child(arguments, limit):
    """A step in a process of its own under its time limit; None when it failed (the caller stops)."""
    env = dict(os.environ)
    for name in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[name] = str(min(THREADS, int(env.get(name, THREADS))))
    try:
        return subprocess.run([sys.executable] + arguments, cwd=ROOT, env=env, timeout=limit, check=True,
                              capture_output=True, text=True)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as error:
        sys.stderr.write("step failed: %s\n%s\n" % (" ".join(arguments), getattr(error, "stderr", "") or error))
        return None


def report(lines, r):
    variant = "plain basis, k_ising_rows_seg" if r["unique_targets"] else "duplicate-keeping variant"
    lines.append("%s (%s), order-%d tables: %d clusters, %d rows (mean %.0f per cluster), %d couplings; %d runs" % (
        r["model"], variant, r["order"], r["clusters"], r["rows"], r["rows"] / r["clusters"], r["couplings"], r["runs"]))
    lines.append("  one segmented call           wall %s   device %s" % (stats(r["segmented_wall"]), stats(r["segmented_ms"])))
    for threads in (1, THREADS):
        lines.append("  loop of ising_csr, %2d thread%s wall %s   device %s (sum over the calls)" % (
            threads, " " if threads == 1 else "s", stats(r["loop%d_wall" % threads]), stats(r["loop%d_ms" % threads])))
    lines.append("  wall, loop / segmented:      %.2fx on 1 thread, %.2fx on %d threads" % (
        statistics.median(r["loop1_wall"]) / statistics.median(r["segmented_wall"]),
        statistics.median(r["loop%d_wall" % THREADS]) / statistics.median(r["segmented_wall"]), THREADS))
    lines.append("")
    print("\n".join(lines[-6:]), flush=True)


def pipeline(lines):
    """sampled_components, greedy, 256 clusters, with and without --build-batch; False when a run failed."""
    base = ["-m", "annealing_sign_problem_amd.sampled_components", "--model", "heisenberg_kagome_16", "--order", "1",
            "--number-samples", "256", "--batch", "256", "--no-annealing", "--greedy-batch", "--jobs", str(THREADS),
            "--seed", "12345"]
    lines.append("sampled_components " + " ".join(base[2:]) + " [--build-batch], wall clock of the whole command:")
    with tempfile.TemporaryDirectory() as tmp:
        seconds = {False: [], True: []}
        for run in range(3):
            for flag in (False, True):
                out = os.path.join(tmp, "%s%d.csv" % ("batch" if flag else "loop", run))  # (no overwriting)
                started = time.perf_counter()
                if child(base + ["--output", out] + (["--build-batch"] if flag else []), PIPELINE_LIMIT) is None:
                    return False
                seconds[flag].append(time.perf_counter() - started)
        files = []
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), "rb") as f:
                files.append(f.read())
        same = len(files) == 6 and all(data == files[0] for data in files)
    for flag in (False, True):
        lines.append("  %-22s %s s" % ("with --build-batch:" if flag else "without:",
                                       ", ".join("%.2f" % s for s in seconds[flag])))
    lines.append("  the six CSV files are %s" % ("byte-identical" if same else "DIFFERENT"))
    lines.append("")
    print("\n".join(lines[-5:]), flush=True)
    return same


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "ising_segments_timing.txt"))
    parser.add_argument("--hdf5", default=os.path.join(ROOT, "physical_systems", "data-large", "heisenberg_kagome_36.h5"))
    parser.add_argument("--skip-pipeline", action="store_true")
    parser.add_argument("--step", nargs=4, metavar=("MODEL", "HDF5", "ORDER", "CLUSTERS"), help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.runs < 5:
        parser.error("--runs must be at least 5")
    if args.step:
        model, hdf5, order, count = args.step
        return step(model, "" if hdf5 == "-" else hdf5, int(order), int(count), args.runs)
    sector = ("heisenberg_kagome_36", args.hdf5) if os.path.exists(args.hdf5) else ("heisenberg_kagome_18", "-")
    lines = ["tools/time_ising_segments.py --runs %d" % args.runs,
             "wall: the Python call(s), uploads and downloads included; device: asp_operator_last_ms (HIP events around "
             "the launches, no host<->HBM copies).  Median (min, max) after a warm-up call.", ""]
    ok = True
    for model, hdf5 in (("heisenberg_kagome_16", "-"), sector):
        for order in (0, 1):
            for count in ROUNDS:
                done = child([os.path.abspath(__file__), "--runs", str(args.runs), "--step", model, hdf5, str(order),
                              str(count)], STEP_LIMIT) if ok else None
                if done is None:
                    ok = False
                    break
                for line in done.stdout.splitlines():
                    if line.startswith("RESULT "):
                        report(lines, json.loads(line[len("RESULT "):]))
    if ok and not args.skip_pipeline:
        ok = pipeline(lines)
    if not ok:
        lines.append("(the run ended at the first step that failed)")
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
