"""Wall time and device time of one LEVEL of a round of clusters: the ONE segmented
extension call (asp_operator_extend_segments) and the ONE segmented cutoff call (asp_sparsify_component_segments),
each beside the loop of the existing per-cluster calls over the same clusters — asp_operator_extend and
asp_sparsify_component, unchanged in the same library — on 1 and on 16 host threads.  The loop is the comparison,
never the new code against itself.

Rounds of 64, 256 and 1024 clusters at order 1, grown as the pipeline grows them (create_small_cluster_around_point,
log-uniform 50 ... 1000 states, keep probability 0.5) from random basis states, on heisenberg_kagome_16 (plain basis)
and heisenberg_kagome_18 (symmetry-adapted basis).  The extension is timed on the clusters; the cutoff on the Ising
models of their extensions (asp_operator_ising_segments; amplitudes hashed from the keys, normalised per cluster) at
reltol 1e-4, the cluster's own states frozen as far as they hang together under that cutoff (a first mask-only
pass with the anchor alone frozen finds them; freezing more only adds couplings, so no frozen spin is stranded).
Every timing comes after a warm-up call: median (min .. max) over --runs >= 5 repetitions.  The results of the two
routes are compared, integers and bits, before anything is timed.

Then sampled_components on 256 clusters of heisenberg_kagome_16 at order 1 with the greedy solver (--no-annealing
--greedy-batch --build-batch --jobs 16), with and without --level-batch, three runs each; all six CSV files are
compared byte for byte.

Every step runs in a child process of its own under its own time limit, at most 16 host threads; the first step that
fails ends the run.  Writes --output (default profiles/level_batch_timing.txt).  (Development aid; GPU.)

    python tools/time_level_batch.py [--runs 5] [--output FILE]
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
MODELS = ("heisenberg_kagome_16", "heisenberg_kagome_18")
RELTOL = 1e-4
STEP_LIMIT = 360   # seconds per measuring step
PIPELINE_LIMIT = 240


def amplitudes(keys):
    """Hashed positive amplitudes over a few decades."""
    h = (keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return np.exp(-6.0 * h.astype(np.float64) / float(1 << 24)) + 1e-3


def stats(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def build_round(op, count, seed):
    """`count` clusters as the pipeline grows them."""
    from annealing_sign_problem_amd import sampled_components

    rng = np.random.default_rng(seed)
    np.random.seed(seed)  # (the growth draws from numpy's global stream)
    clusters = []
    for start in rng.choice(op.basis.states, size=count, replace=True).tolist():
        size = sampled_components.random_cluster_size(50, 1000)
        clusters.append(np.asarray(sampled_components.create_small_cluster_around_point(
            int(start), op, required_size=size, keep_probability=0.5), dtype=np.uint64))
    return clusters


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


def measure(result, name, segmented, one, count, runs):
    """Fills result[name + ...]: `segmented()` -> (output, device ms); `one(g)` -> (output, device ms)."""
    wall, ms = [], []
    for _ in range(runs):
        started = time.perf_counter()
        _, m = segmented()
        wall.append(1e3 * (time.perf_counter() - started))
        ms.append(m)
    result[name + "_segmented_wall"], result[name + "_segmented_ms"] = wall, ms
    for threads in (1, THREADS):
        wall, ms = [], []
        for _ in range(runs):
            w, parts = timed(one, count, threads)
            wall.append(w)
            ms.append(sum(m for _, m in parts))
        result[name + "_loop%d_wall" % threads], result[name + "_loop%d_ms" % threads] = wall, ms


def step(model, count, runs):
    """One (model, round) measurement; prints one JSON line."""
    import scipy.sparse

    from annealing_sign_problem_amd import _lib, common, operators, synthetic

    op = operators.Operator.from_config(synthetic.load_models()[model])
    op.basis.build()
    device = op.device()
    lib = _lib.load()
    clusters = build_round(op, count, 1000 + count)
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clusters])]).astype(np.uint64)
    keys = np.concatenate(clusters)

    # ---- the extension -------------------------------------------------------------------------------------
    def extend_segmented():
        return device.extend_segments(keys, offsets), device.last_ms

    def extend_one(g):
        return device.extend(clusters[g]), device.last_ms

    (states, out_offsets), _ = extend_segmented()
    _, parts = timed(extend_one, count, 1)
    timed(extend_one, count, THREADS)
    extended = [states[int(out_offsets[g]):int(out_offsets[g + 1])] for g in range(count)]
    for g, (own, _) in enumerate(parts):
        assert np.array_equal(extended[g], own), "the extension differs in segment %d" % g
    result = {"model": model, "clusters": count, "keys": int(keys.size), "extended": int(states.size),
              "unique_targets": bool(device.unique_targets), "runs": runs}
    measure(result, "extend", extend_segmented, extend_one, count, runs)

    # ---- the models of the extensions (the existing segmented build), then the cutoff -----------------------
    psis = []
    for c in extended:
        psi = amplitudes(c)
        psis.append(psi / np.linalg.norm(psi))
    indptr, col, val = device.ising_csr_segments(states, np.concatenate(psis), out_offsets)
    anchors = np.zeros(count, dtype=np.uint64)
    frozen = np.zeros(states.size, dtype=bool)
    for g in range(count):
        anchors[g] = np.searchsorted(extended[g], clusters[g][0])
        frozen[int(out_offsets[g]) + int(anchors[g])] = True
    keep = common.sparsify_component_segments(out_offsets, indptr, col, val, frozen, RELTOL, anchors)[0]
    for g in range(count):  # the cluster's own states that hang together with the anchor under the cutoff
        where = int(out_offsets[g]) + np.searchsorted(extended[g], clusters[g])
        frozen[where[keep[where]]] = True
    matrices = []
    for g in range(count):
        first, last = int(out_offsets[g]), int(out_offsets[g + 1])
        begin, end = int(indptr[first]), int(indptr[last])
        m = scipy.sparse.csr_matrix((val[begin:end], col[begin:end], indptr[first:last + 1] - begin),
                                    shape=(last - first, last - first))
        m.has_sorted_indices = True
        m.has_canonical_format = True
        matrices.append((m, frozen[first:last].copy(), int(anchors[g])))

    def cut_segmented():
        out = common.sparsify_component_segments(out_offsets, indptr, col, val, frozen, RELTOL, anchors)
        return out, float(lib.asp_sparsify_last_ms())

    def cut_one(g):
        out = common.sparsify_component(matrices[g][0], matrices[g][1], RELTOL, matrices[g][2])
        return out, float(lib.asp_sparsify_last_ms())

    (keep, kept_offsets, out_indptr, out_indices, out_data), _ = cut_segmented()
    _, parts = timed(cut_one, count, 1)
    timed(cut_one, count, THREADS)
    for g, ((own_keep, block), _) in enumerate(parts):
        first, last = int(kept_offsets[g]), int(kept_offsets[g + 1])
        begin, end = int(out_indptr[first]), int(out_indptr[last])
        assert np.array_equal(keep[int(out_offsets[g]):int(out_offsets[g + 1])], own_keep), "keep differs in segment %d" % g
        assert np.array_equal(out_indptr[first:last + 1] - begin, block.indptr), "indptr differs in segment %d" % g
        assert np.array_equal(out_indices[begin:end], block.indices), "columns differ in segment %d" % g
        assert out_data[begin:end].tobytes() == block.data.tobytes(), "couplings differ in segment %d" % g
    result.update({"spins": int(states.size), "couplings": int(col.size), "kept_spins": int(kept_offsets[-1]),
                   "kept_couplings": int(out_data.size)})
    measure(result, "cut", cut_segmented, cut_one, count, runs)
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
    basis = "plain basis" if r["unique_targets"] else "symmetry-adapted basis"
    before = len(lines)
    lines.append("%s (%s), order 1: %d clusters, %d keys (mean %.0f per cluster) -> %d extended states; cutoff %g: "
                 "%d spins, %d couplings -> %d spins, %d couplings; %d runs" % (
                     r["model"], basis, r["clusters"], r["keys"], r["keys"] / r["clusters"], r["extended"], RELTOL,
                     r["spins"], r["couplings"], r["kept_spins"], r["kept_couplings"], r["runs"]))
    for name, single, call in (("extend", "asp_operator_extend", "asp_operator_extend_segments"),
                               ("cut", "asp_sparsify_component", "asp_sparsify_component_segments")):
        lines.append("  %s" % call)
        lines.append("    one segmented call             wall %s   device %s" % (
            stats(r[name + "_segmented_wall"]), stats(r[name + "_segmented_ms"])))
        for threads in (1, THREADS):
            lines.append("    loop of %-22s wall %s   device %s (sum over the calls)" % (
                "%s, %d thr." % (single.replace("asp_", ""), threads), stats(r[name + "_loop%d_wall" % threads]),
                stats(r[name + "_loop%d_ms" % threads])))
        lines.append("    wall, loop / segmented:        %.2fx on 1 thread, %.2fx on %d threads" % (
            statistics.median(r[name + "_loop1_wall"]) / statistics.median(r[name + "_segmented_wall"]),
            statistics.median(r[name + "_loop%d_wall" % THREADS]) / statistics.median(r[name + "_segmented_wall"]),
            THREADS))
    lines.append("")
    print("\n".join(lines[before:]), flush=True)


def pipeline(lines):
    """sampled_components, greedy, 256 clusters, --build-batch with and without --level-batch; False when a run
    failed or the files differ."""
    base = ["-m", "annealing_sign_problem_amd.sampled_components", "--model", "heisenberg_kagome_16", "--order", "1",
            "--number-samples", "256", "--batch", "256", "--no-annealing", "--greedy-batch", "--build-batch", "--jobs",
            str(THREADS), "--seed", "12345"]
    before = len(lines)
    lines.append("sampled_components " + " ".join(base[2:]) + " [--level-batch], wall clock of the whole command:")
    with tempfile.TemporaryDirectory() as tmp:
        seconds = {False: [], True: []}
        for run in range(3):
            for flag in (False, True):
                out = os.path.join(tmp, "%s%d.csv" % ("level" if flag else "loop", run))  # (no overwriting)
                started = time.perf_counter()
                if child(base + ["--output", out] + (["--level-batch"] if flag else []), PIPELINE_LIMIT) is None:
                    return False
                seconds[flag].append(time.perf_counter() - started)
        files = []
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), "rb") as f:
                files.append(f.read())
        same = len(files) == 6 and all(data == files[0] for data in files)
    for flag in (False, True):
        lines.append("  %-22s %s s" % ("with --level-batch:" if flag else "without:",
                                       ", ".join("%.2f" % s for s in seconds[flag])))
    lines.append("  the six CSV files are %s" % ("byte-identical" if same else "DIFFERENT"))
    lines.append("")
    print("\n".join(lines[before:]), flush=True)
    return same


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "level_batch_timing.txt"))
    parser.add_argument("--skip-pipeline", action="store_true")
    parser.add_argument("--step", nargs=2, metavar=("MODEL", "CLUSTERS"), help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.runs < 5:
        parser.error("--runs must be at least 5")
    if args.step:
        return step(args.step[0], int(args.step[1]), args.runs)
    lines = ["tools/time_level_batch.py --runs %d" % args.runs,
             "wall: the Python call(s), uploads and downloads included; device: asp_operator_last_ms / "
             "asp_sparsify_last_ms (HIP events around the launches, no host<->HBM copies).  Median (min, max) after a "
             "warm-up call.", ""]
    ok = True
    for model in MODELS:
        for count in ROUNDS:
            done = child([os.path.abspath(__file__), "--runs", str(args.runs), "--step", model, str(count)],
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
        f.write("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
