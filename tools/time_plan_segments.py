"""Wall time and device time of the sweep plans of a round: ONE segmented call
(asp_sa_plan_create_segments) beside the loop of asp_sa_plan_create over the same models — unchanged in the same
library — on 1 and on 16 host threads.  The loop is the comparison, never the new code against itself.

Rounds of 64, 256 and 1024 clusters of heisenberg_kagome_16 at order 1, sampled and grown as the pipeline does
(generate_clusters from the exact ground state), their models built by make_ising_models and taken one level up by
extend_and_sparsify_models; and one round of 32 planted_cluster(100000, mean_degree=8).  Every timing comes after a
warm-up call: median (min, max) over --runs repetitions (three for the planted round); the plans are destroyed
outside the timed region in both routes.  The routes alternate run by run.  One more segmented call per run has
ASP_PLAN_SEGMENTS_TIMING=1 and reports the wall time of its steps: front (uploads, device front, downloads), host
(colouring, permutation, blocks and the host's ELL copy on at most 16 threads), handles (a stream and four events
per plan), alloc (the plans' device arrays) and back (the staged upload and the fill kernel).  Before anything is
timed, asp_sa_plan_info and every device array of the two routes are compared on a sample of the segments.

Then sampled_components on 256 clusters of heisenberg_kagome_16 at order 1 with the greedy solver (--no-annealing
--greedy-batch --build-batch --level-batch --jobs 16), with and without --plan-batch, three runs each; all six CSV
files are compared byte for byte.

Every step runs in a child process of its own under its own time limit, at most 16 host threads; the first step
that fails ends the run.  Writes --output (default profiles/plan_segments_timing.txt).  (Development aid; GPU.)

    python tools/time_plan_segments.py [--runs 5] [--output FILE]
"""
import argparse
import ctypes
import json
import os
import re
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
PLANTED = (32, 100000, 8.0)
STEP_LIMIT = 420   # seconds per measuring step
PIPELINE_LIMIT = 240
STEPS = ("front", "host", "handles", "alloc", "back")


def stats(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def kagome_round(count):
    """[(indptr, indices, data, field)] of the order-1 models of `count` sampled clusters."""
    from annealing_sign_problem_amd import common, sampled_components

    args = sampled_components.parse_command_line(["--model", "heisenberg_kagome_16", "--order", "1", "--number-samples",
                                                  str(count), "--seed", "12345", "--output", "unused.csv"])
    hamiltonian, ground_state = sampled_components.load_input(args)
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, hamiltonian.basis)
    np.random.seed(args.seed)
    clusters = list(sampled_components.generate_clusters(hamiltonian, ground_state, args.number_samples,
                                                         args.sampled_power, args.min_cluster_size,
                                                         args.max_cluster_size, args.keep_probability))
    models = common.make_ising_models(clusters, hamiltonian, log_psi_fn=log_coeff_fn)
    models = common.extend_and_sparsify_models(models, log_coeff_fn, args.global_cutoff, clusters)
    return [m.ising_hamiltonian._arrays() for m in models]


def planted_round(count, spins, mean_degree):
    from annealing_sign_problem_amd import synthetic

    out = []
    for g in range(count):
        matrix, field, _ = synthetic.planted_cluster(spins, mean_degree=mean_degree, seed=1000 + g)
        matrix = matrix.tocsr()
        matrix.sort_indices()
        out.append((matrix.indptr.astype(np.int64), matrix.indices.astype(np.int32), matrix.data.astype(np.float64),
                    np.ascontiguousarray(field, dtype=np.float64)))
    return out


def timed(function, count, threads):
    """``[function(g) for g in range(count)]`` on `threads` host threads: (wall ms, results)."""
    from concurrent.futures import ThreadPoolExecutor

    started = time.perf_counter()
    if threads == 1:
        parts = [function(g) for g in range(count)]
    else:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            parts = list(pool.map(function, range(count)))
    return 1e3 * (time.perf_counter() - started), parts


def with_stderr_captured(function):
    """function() with the process's stderr (the C library's too) collected: (result, text)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as sink:
        os.dup2(sink.fileno(), 2)
        try:
            result = function()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        sink.seek(0)
        return result, sink.read().decode("utf-8", "replace")


def step(kind, count, runs):
    """One round's measurement; prints one JSON line."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    _lib.require_gpu()
    segments = kagome_round(count) if kind == "kagome" else planted_round(*PLANTED)
    count = len(segments)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([s[0].size - 1 for s in segments], dtype=np.uint64)
    parts, entries = [np.zeros(1, dtype=np.int64)], 0
    for ip, _, _, _ in segments:
        parts.append(ip[1:] + entries)
        entries += int(ip[-1])
    indptr = np.concatenate(parts)
    indices = np.ascontiguousarray(np.concatenate([s[1] for s in segments]), dtype=np.int32)
    data = np.ascontiguousarray(np.concatenate([s[2] for s in segments]), dtype=np.float64)
    field = np.ascontiguousarray(np.concatenate([s[3] for s in segments]), dtype=np.float64)

    def segmented():
        plans = (ctypes.c_void_p * count)()
        started = time.perf_counter()
        _lib.check(lib.asp_sa_plan_create_segments(ctypes.c_uint64(count), _lib.ptr(offsets), _lib.ptr(indptr),
                                                   _lib.ptr(indices), _lib.ptr(data), _lib.ptr(field), plans))
        wall = 1e3 * (time.perf_counter() - started)
        return wall, float(lib.asp_sa_plan_segments_last_ms()), [ctypes.c_void_p(p) for p in plans]

    def one(g):
        ip, ix, dv, h = segments[g]
        handle = lib.asp_sa_plan_create(ctypes.c_uint64(ip.size - 1), _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv), _lib.ptr(h))
        if not handle:
            raise _lib.AspError(lib.asp_last_error_code(), _lib.last_error())
        return ctypes.c_void_p(handle)

    def destroy(plans):
        for p in plans:
            lib.asp_sa_plan_destroy(p)

    # the two routes give the same plans (also the warm-up of both)
    _, _, batch = segmented()
    _, loop = timed(one, count, 1)
    for g in range(0, count, max(1, count // 16)):
        a, b = _lib.SaInfo(), _lib.SaInfo()
        _lib.check(lib.asp_sa_plan_info(batch[g], ctypes.byref(a)))
        _lib.check(lib.asp_sa_plan_info(loop[g], ctypes.byref(b)))
        assert bytes(a) == bytes(b), "asp_sa_plan_info differs in segment %d" % g
        for name in sa.PLAN_ARRAYS:
            assert sa.read_plan_array(batch[g], name).tobytes() == sa.read_plan_array(loop[g], name).tobytes(), (
                "%s differs in segment %d" % (name, g))
    destroy(batch)
    destroy(loop)
    destroy(timed(one, count, THREADS)[1])
    result = {"kind": kind, "segments": count, "spins": int(offsets[-1]), "stored": int(indices.size), "runs": runs}
    # the three routes alternate, run by run: what else the machine does reaches all of them alike
    result.update({"segmented_wall": [], "segmented_ms": [], "loop1_wall": [], "loop%d_wall" % THREADS: []})
    steps = {name: [] for name in STEPS}
    for _ in range(runs):
        w, m, plans = segmented()
        destroy(plans)
        result["segmented_wall"].append(w)
        result["segmented_ms"].append(m)
        for threads in (1, THREADS):
            w, plans = timed(one, count, threads)
            destroy(plans)
            result["loop%d_wall" % threads].append(w)
        os.environ["ASP_PLAN_SEGMENTS_TIMING"] = "1"
        (_, _, plans), text = with_stderr_captured(segmented)
        del os.environ["ASP_PLAN_SEGMENTS_TIMING"]
        destroy(plans)
        for name in STEPS:
            found = re.search(r"plan segments %s\s+([0-9.]+) ms" % name, text)
            steps[name].append(float(found.group(1)) if found else float("nan"))
    for name in STEPS:
        result["step_" + name] = statistics.median(steps[name])
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
    before = len(lines)
    what = ("heisenberg_kagome_16, order 1" if r["kind"] == "kagome"
            else "planted_cluster(%d, mean_degree=%g)" % (PLANTED[1], PLANTED[2]))
    lines.append("%s: %d models, %d spins (mean %.0f per model), %d stored couplings; %d runs" % (
        what, r["segments"], r["spins"], r["spins"] / r["segments"], r["stored"], r["runs"]))
    lines.append("    one asp_sa_plan_create_segments call  wall %s   device %s" % (
        stats(r["segmented_wall"]), stats(r["segmented_ms"])))
    for threads in (1, THREADS):
        lines.append("    loop of asp_sa_plan_create, %2d thr.    wall %s" % (threads, stats(r["loop%d_wall" % threads])))
    lines.append("    wall, loop / segmented:               %.2fx on 1 thread, %.2fx on %d threads" % (
        statistics.median(r["loop1_wall"]) / statistics.median(r["segmented_wall"]),
        statistics.median(r["loop%d_wall" % THREADS]) / statistics.median(r["segmented_wall"]), THREADS))
    total = sum(r["step_" + name] for name in STEPS)
    lines.append("    steps of a segmented call (wall, median): " + ", ".join(
        "%s %.3f ms (%.0f %%)" % (name, r["step_" + name], 100 * r["step_" + name] / total) for name in STEPS))
    lines.append("")
    print("\n".join(lines[before:]), flush=True)


def pipeline(lines):
    """sampled_components, greedy, 256 clusters, with and without --plan-batch; False when a run failed or the
    files differ."""
    base = ["-m", "annealing_sign_problem_amd.sampled_components", "--model", "heisenberg_kagome_16", "--order", "1",
            "--number-samples", "256", "--batch", "256", "--no-annealing", "--greedy-batch", "--build-batch",
            "--level-batch", "--jobs", str(THREADS), "--seed", "12345"]
    before = len(lines)
    lines.append("sampled_components " + " ".join(base[2:]) + " [--plan-batch], wall clock of the whole command:")
    with tempfile.TemporaryDirectory() as tmp:
        seconds = {False: [], True: []}
        for run in range(3):
            for flag in (False, True):
                out = os.path.join(tmp, "%s%d.csv" % ("batch" if flag else "loop", run))  # (no overwriting)
                started = time.perf_counter()
                if child(base + ["--output", out] + (["--plan-batch"] if flag else []), PIPELINE_LIMIT) is None:
                    return False
                seconds[flag].append(time.perf_counter() - started)
        files = []
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), "rb") as f:
                files.append(f.read())
        same = len(files) == 6 and all(data == files[0] for data in files)
    for flag in (False, True):
        lines.append("  %-22s %s s" % ("with --plan-batch:" if flag else "without:",
                                       ", ".join("%.2f" % s for s in seconds[flag])))
    lines.append("  the six CSV files are %s" % ("byte-identical" if same else "DIFFERENT"))
    lines.append("")
    print("\n".join(lines[before:]), flush=True)
    return same


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "plan_segments_timing.txt"))
    parser.add_argument("--skip-pipeline", action="store_true")
    parser.add_argument("--step", nargs=2, metavar=("KIND", "CLUSTERS"), help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.runs < 3:
        parser.error("--runs must be at least 3")
    if args.step:
        return step(args.step[0], int(args.step[1]), args.runs if args.step[0] == "kagome" else 3)
    lines = ["tools/time_plan_segments.py --runs %d" % args.runs,
             "wall: the C call(s) from Python, uploads and downloads included, asp_sa_plan_destroy excluded; device: "
             "asp_sa_plan_segments_last_ms (HIP events around the launches, no host<->HBM copies).  Median (min, max) "
             "after a warm-up call of each route.", ""]
    ok = True
    for kind, count in [("kagome", c) for c in ROUNDS] + [("planted", PLANTED[0])]:
        done = child([os.path.abspath(__file__), "--runs", str(args.runs), "--step", kind, str(count)],
                     STEP_LIMIT) if ok else None
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
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
