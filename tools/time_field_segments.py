"""Wall time and device time of the boundary fields of a ROUND of clusters: ONE segmented call
(asp_operator_field_segments, with asp_operator_extend_segments for the environments) beside the loop of
DeviceOperator.extend + DeviceOperator.field calls over the same clusters — the per-cluster code path, unchanged in
the same library — on 1 and on 16 host threads.

Rounds of 64, 256 and 1024 clusters, grown on the device (asp_operator_grow_segments, log-uniform 50 ... 1000 states,
keep probability 0.5) from random basis states, at order 0 (the clusters) and order 1 (their one-hop extensions), on
heisenberg_kagome_16 (plain basis: k_field_rows_seg) and on heisenberg_kagome_18 in its inversion sector
(k_field_list_seg).  The environment of a table is its one-hop extension.  Amplitudes are hashed from the keys and
normalised per cluster.  Every timing comes after a warm-up call: median (min .. max) over --runs >= 5 repetitions.
The results of the two routes are compared, bits and counts, before anything is timed.

Then reweight_ising_models(external_field=True) for 100 draws of one kagome_16 cluster beside the loop of
reweight_ising_model calls, and sampled_components on 256 clusters of heisenberg_kagome_16 at order 1 with the greedy
solver (--no-annealing --external-field --build-batch --level-batch --greedy-batch --jobs 16), three runs, here and —
with --parent DIR, a built checkout of the parent commit — there; all CSV files are compared byte for byte.

Every step runs in a child process of its own under its own time limit, at most 16 host threads; the first step that
fails ends the run.  Writes --output (default profiles/field_segments_timing.txt).  (Development aid; GPU.)

    python tools/time_field_segments.py [--runs 5] [--output FILE] [--parent DIR]
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
DRAWS = 100
STEP_LIMIT = 300   # seconds per measuring step
PIPELINE_LIMIT = 300


def amplitudes(keys):
    """Hashed signed amplitudes over a few decades."""
    h = (keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    sign = np.where((h & np.uint64(1)) == 0, 1.0, -1.0)
    return sign * (np.exp(-6.0 * h.astype(np.float64) / float(1 << 24)) + 1e-3)


def stats(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def build_round(op, count, order, seed):
    """`count` clusters grown on the device; order 1: their one-hop extensions."""
    from annealing_sign_problem_amd import common

    rng = np.random.default_rng(seed)
    seeds = rng.choice(op.basis.states, size=count, replace=True)
    sizes = np.exp(rng.uniform(np.log(50), np.log(1000), size=count)).astype(np.uint64)
    clusters, _ = op.device().grow_segments(seeds, sizes, 0.5, seed)
    return common.extension_spins_segments(op, clusters) if order == 1 else clusters


def step(model, order, count, runs):
    """One (model, order, round) measurement; prints one JSON line."""
    from concurrent.futures import ThreadPoolExecutor

    from annealing_sign_problem_amd import operators, synthetic

    op = operators.Operator.from_config(synthetic.load_models()[model])
    op.basis.build()
    device = op.device()
    clusters = build_round(op, count, order, 1000 * order + count)
    norms = [np.linalg.norm(amplitudes(c)) for c in clusters]
    psis = [amplitudes(c) / n for c, n in zip(clusters, norms)]
    keys, psi = np.concatenate(clusters), np.concatenate(psis)
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clusters])]).astype(np.uint64)

    def one(g):
        env = device.extend(clusters[g])
        out = device.field(clusters[g], psis[g], env, amplitudes(env) / norms[g])
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
        env_keys, env_offsets = device.extend_segments(keys, offsets)
        env_psi = amplitudes(env_keys) / np.repeat(norms, np.diff(env_offsets.astype(np.int64)))
        between = time.perf_counter()
        out = device.field_segments(keys, psi, offsets, env_keys, env_psi, env_offsets)
        done = time.perf_counter()
        return 1e3 * (done - started), 1e3 * (done - between), out, device.last_ms, int(env_keys.size)

    # warm-up, and the two routes agree: the field as bits, the counts
    _, _, (field, unresolved), _, env_size = segmented()
    _, parts = loop(1)
    loop(THREADS)
    for g, ((f, lost), _) in enumerate(parts):
        first, last = int(offsets[g]), int(offsets[g + 1])
        assert field[first:last].tobytes() == f.tobytes() and int(unresolved[g]) == lost == 0, g
    result = {"model": model, "order": order, "clusters": count, "rows": int(keys.size), "environment": env_size,
              "unique_targets": bool(device.unique_targets), "runs": runs}
    wall, call, ms = [], [], []
    for _ in range(runs):
        w, c, _, m, _ = segmented()
        wall.append(w)
        call.append(c)
        ms.append(m)
    result["segmented_wall"], result["segmented_call"], result["segmented_ms"] = wall, call, ms
    for threads in (1, THREADS):
        wall, ms = [], []
        for _ in range(runs):
            w, parts = loop(threads)
            wall.append(w)
            ms.append(sum(m for _, m in parts))
        result["loop%d_wall" % threads], result["loop%d_ms" % threads] = wall, ms
    print("RESULT " + json.dumps(result), flush=True)


def reweight(runs):
    """reweight_ising_models(external_field=True) for DRAWS draws beside the per-draw loop; one JSON line."""
    from annealing_sign_problem_amd import common, operators, synthetic

    op = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_16"])
    op.basis.build()
    rng = np.random.default_rng(7)
    vector = rng.normal(size=op.basis.states.size) * np.exp(0.5 * rng.normal(size=op.basis.states.size))
    cluster = build_round(op, 1, 0, 77)[0]
    base = common.make_ising_model(cluster, op, log_psi_fn=common.ground_state_to_log_coeff_fn(vector, op.basis),
                                   external_field=True)
    base.ising_hamiltonian.plan()
    np.random.seed(7)
    fns = [common.ground_state_to_log_coeff_fn(common.add_noise_to_amplitudes(vector, eps=0.5), op.basis)
           for _ in range(DRAWS)]
    pools = {"loop": None, "batch": None}

    def loop():
        started = time.perf_counter()
        pool = pools["loop"] or [None] * DRAWS
        pools["loop"] = [common.reweight_ising_model(base, None, fn, True, out) for fn, out in zip(fns, pool)]
        return 1e3 * (time.perf_counter() - started)

    def batch():
        started = time.perf_counter()
        pools["batch"] = common.reweight_ising_models(base, log_psi_fns=fns, external_field=True, outs=pools["batch"])
        return 1e3 * (time.perf_counter() - started)

    loop(), batch()
    for a, b in zip(pools["loop"], pools["batch"]):
        assert a.ising_hamiltonian.field.tobytes() == b.ising_hamiltonian.field.tobytes()
        assert a.ising_hamiltonian.exchange.data.tobytes() == b.ising_hamiltonian.exchange.data.tobytes()
    result = {"states": int(cluster.size), "draws": DRAWS, "runs": runs, "loop": [loop() for _ in range(runs)],
              "batch": [batch() for _ in range(runs)]}
    print("RESULT " + json.dumps(result), flush=True)


def child(arguments, limit, cwd=ROOT):
    """A step in a process of its own under its time limit; None when it failed (the caller stops)."""
    env = dict(os.environ)
    for name in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[name] = str(min(THREADS, int(env.get(name, THREADS))))
    try:
        return subprocess.run([sys.executable] + arguments, cwd=cwd, env=env, timeout=limit, check=True,
                              capture_output=True, text=True)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as error:
        sys.stderr.write("step failed: %s\n%s\n" % (" ".join(arguments), getattr(error, "stderr", "") or error))
        return None


def report(lines, r):
    variant = "plain basis, k_field_rows_seg" if r["unique_targets"] else "connection-list variant, k_field_list_seg"
    lines.append("%s (%s), order-%d tables: %d clusters, %d rows (mean %.0f per cluster), %d environment entries; "
                 "%d runs" % (r["model"], variant, r["order"], r["clusters"], r["rows"], r["rows"] / r["clusters"],
                              r["environment"], r["runs"]))
    lines.append("  extend_segments + field_segments   wall %s" % stats(r["segmented_wall"]))
    lines.append("  of which field_segments            wall %s   device %s" % (stats(r["segmented_call"]),
                                                                              stats(r["segmented_ms"])))
    for threads in (1, THREADS):
        lines.append("  loop of extend + field, %2d thread%s wall %s   device %s (field, sum over the calls)" % (
            threads, " " if threads == 1 else "s", stats(r["loop%d_wall" % threads]), stats(r["loop%d_ms" % threads])))
    lines.append("  wall, loop / segmented:            %.2fx on 1 thread, %.2fx on %d threads" % (
        statistics.median(r["loop1_wall"]) / statistics.median(r["segmented_wall"]),
        statistics.median(r["loop%d_wall" % THREADS]) / statistics.median(r["segmented_wall"]), THREADS))
    lines.append("")
    print("\n".join(lines[-7:]), flush=True)


def pipeline(lines, parent):
    """sampled_components, greedy with the field, 256 clusters, here and in `parent`; False when a run failed."""
    base = ["-m", "annealing_sign_problem_amd.sampled_components", "--model", "heisenberg_kagome_16", "--order", "1",
            "--number-samples", "256", "--batch", "256", "--no-annealing", "--external-field", "--build-batch",
            "--level-batch", "--greedy-batch", "--jobs", str(THREADS), "--seed", "12345"]
    lines.append("sampled_components " + " ".join(base[2:]) + ", wall clock of the whole command:")
    trees = [("this commit", ROOT)] + ([("parent commit", parent)] if parent else [])
    with tempfile.TemporaryDirectory() as tmp:
        seconds = {name: [] for name, _ in trees}
        for run in range(3):
            for at, (name, tree) in enumerate(trees):
                out = os.path.join(tmp, "tree%d_run%d.csv" % (at, run))  # (no overwriting)
                started = time.perf_counter()
                if child(base + ["--output", out], PIPELINE_LIMIT, cwd=tree) is None:
                    return False
                seconds[name].append(time.perf_counter() - started)
        files = []
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), "rb") as f:
                files.append(f.read())
        same = len(files) == 3 * len(trees) and all(data == files[0] for data in files)
    for name, _ in trees:
        lines.append("  %-15s %s s" % (name + ":", ", ".join("%.2f" % s for s in seconds[name])))
    if not parent:
        lines.append("  (no checkout of the parent commit was given: --parent)")
    lines.append("  the %d CSV files are %s" % (len(files), "byte-identical" if same else "DIFFERENT"))
    lines.append("")
    print("\n".join(lines[-5:]), flush=True)
    return same


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "field_segments_timing.txt"))
    parser.add_argument("--parent", default="", help="a built checkout of the parent commit, for the pipeline")
    parser.add_argument("--skip-pipeline", action="store_true")
    parser.add_argument("--step", nargs=3, metavar=("MODEL", "ORDER", "CLUSTERS"), help=argparse.SUPPRESS)
    parser.add_argument("--reweight", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.runs < 5:
        parser.error("--runs must be at least 5")
    if args.step:
        model, order, count = args.step
        return step(model, int(order), int(count), args.runs)
    if args.reweight:
        return reweight(args.runs)
    lines = ["tools/time_field_segments.py --runs %d" % args.runs,
             "wall: the Python call(s), uploads and downloads included; device: asp_operator_last_ms (HIP events around "
             "the device work, no host<->HBM copies).  Median (min, max) after a warm-up call.", ""]
    ok = True
    me = os.path.abspath(__file__)
    for model in ("heisenberg_kagome_16", "heisenberg_kagome_18"):
        for order in (0, 1):
            for count in ROUNDS:
                done = child([me, "--runs", str(args.runs), "--step", model, str(order), str(count)],
                             STEP_LIMIT) if ok else None
                if done is None:
                    ok = False
                    break
                for line in done.stdout.splitlines():
                    if line.startswith("RESULT "):
                        report(lines, json.loads(line[len("RESULT "):]))
    done = child([me, "--runs", str(args.runs), "--reweight"], STEP_LIMIT) if ok else None
    if done is None:
        ok = False
    else:
        for line in done.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[len("RESULT "):])
                lines.append("reweight_ising_models(external_field=True), heisenberg_kagome_16, one cluster of %d states, "
                             "%d draws; %d runs" % (r["states"], r["draws"], r["runs"]))
                lines.append("  one call (one field_segments)   wall %s" % stats(r["batch"]))
                lines.append("  loop of reweight_ising_model    wall %s" % stats(r["loop"]))
                lines.append("  wall, loop / one call:          %.2fx" % (statistics.median(r["loop"]) /
                                                                          statistics.median(r["batch"])))
                lines.append("")
                print("\n".join(lines[-5:]), flush=True)
    if ok and not args.skip_pipeline:
        ok = pipeline(lines, os.path.abspath(args.parent) if args.parent else "")
    if not ok:
        lines.append("(the run ended at the first step that failed)")
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
