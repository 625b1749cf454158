"""Device time of the local energies (asp_operator_local_energy) from asp_operator_last_ms, RUNS
calls after a warm-up (median, min .. max), on three workloads:

  * one segment of K = 1e4 and of K = 1e5 random keys of hamming weight 18 of the 36-site kagome operator (72 bonds,
    plain basis: k_eloc_rows), every entry a row, beside asp_operator_field on the same keys with their one-hop
    extension as environment;
  * 50 000 segments — the one-hop neighbourhoods of 50 000 such keys — with one row each (plain basis);
  * 1e4 representatives of the model's symmetry sector in one segment (heisenberg_kagome_36: k_eloc_list).

Beside each, the wall clock of the numpy route on the host: `Operator.batched_apply` of the row keys plus one
`searchsorted` per segment (for the sector on 500 of the rows: the host's symmetrisation is slow).  The device
result is compared with that route before anything is timed.  Writes --output (default
profiles/local_energy_timing.txt).

With --quality: instead, runs `make local_energy` (child processes) on heisenberg_kagome_16 and _18 — 1000 samples,
SIGNS=greedy at orders 0, 1, 2 with and without EXTERNAL_FIELD=1, and SIGNS=exact (which depends on neither) — and
writes the count-weighted mean, its standard error and E0 of every run to --quality-output (default
profiles/local_energy_quality.txt).  (Development aid; GPU.)

    python tools/time_local_energy.py [--runs 5] [--output FILE] [--quality] [--quality-output FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from annealing_sign_problem_amd import operators, synthetic  # noqa: E402
from time_field import amplitudes, random_keys  # noqa: E402


def signed(keys):
    """Hashed amplitudes with hashed signs."""
    sign = np.where((keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63), -1.0, 1.0)
    return amplitudes(keys) * sign


def numpy_route(op, keys, phi, offsets, rows):
    """hphi of the rows on the host: the connections of the row keys, then per segment one searchsorted."""
    other, coeffs, counts = op.batched_apply(keys[rows])
    other, coeffs = other[:, 0], coeffs.real
    segment = np.searchsorted(offsets, rows, side="right") - 1
    entry_segment = np.repeat(segment, counts)
    terms = np.zeros(other.size)
    order = np.argsort(entry_segment, kind="stable")
    bounds = np.searchsorted(entry_segment[order], np.arange(offsets.size))
    for g in np.unique(segment):
        mine = order[bounds[g]:bounds[g + 1]]
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        at = np.minimum(np.searchsorted(keys[lo:hi], other[mine]), hi - lo - 1)
        found = keys[lo + at] == other[mine]
        terms[mine] = np.where(found, coeffs[mine] * phi[lo + at], 0.0)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.add.reduceat(terms, starts)


def stats(ms):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(ms), min(ms), max(ms))


def measure(lines, label, op, keys, phi, offsets, rows, runs, field=False, host_rows=None):
    device = op.device()
    hphi, eloc, missing = device.local_energy(keys, phi, offsets, rows)  # warm-up
    subset = np.arange(rows.size) if host_rows is None else np.arange(0, rows.size, max(1, rows.size // host_rows))
    started = time.perf_counter()
    want = numpy_route(op, keys, phi, offsets.astype(np.int64), rows[subset].astype(np.int64))
    host_s = time.perf_counter() - started
    scale = np.abs(want).max()
    assert np.all(np.abs(hphi[subset] - want) <= 1e-12 * scale), "the device differs from the numpy route"
    ms = []
    for _ in range(runs):
        device.local_energy(keys, phi, offsets, rows)
        ms.append(device.last_ms)
    lines.append("%s: T = %d table entries in %d segments, N = %d rows, %d connections leave their segment, %d calls"
                 % (label, keys.size, offsets.size - 1, rows.size, int(missing.sum(dtype=np.int64)), runs))
    lines.append("  asp_operator_local_energy  %s" % stats(ms))
    if field:
        psi = np.abs(phi) / np.linalg.norm(phi)
        env_keys = device.extend(keys)
        env_psi = amplitudes(env_keys) / np.linalg.norm(phi)
        device.field(keys, psi, env_keys, env_psi)
        field_ms = []
        for _ in range(runs):
            device.field(keys, psi, env_keys, env_psi)
            field_ms.append(device.last_ms)
        lines.append("  asp_operator_field         %s   (E = %d environment states)" % (stats(field_ms), env_keys.size))
    lines.append("  numpy route, wall clock    %9.3f ms for %d rows (batched_apply + searchsorted per segment)"
                 % (1e3 * host_s, subset.size))
    lines.append("")
    print("\n".join(lines[-(5 if field else 4):]), flush=True)


def neighbourhood_segments(op, centres):
    """One segment per centre: its targets (the centre included; distinct in a plain basis), ascending."""
    other, _, counts = op.device().apply(centres)
    segment = np.repeat(np.arange(centres.size), counts)
    order = np.lexsort((other, segment))
    keys = other[order]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    rows = np.flatnonzero(keys == np.repeat(centres, counts)).astype(np.uint64)
    assert rows.size == centres.size
    return keys, offsets, rows


def quality(path, samples, seed, jobs):
    """`make local_energy` over the settings; one line per run from the `#` lines of its CSV."""
    settings = "NUMBER_SAMPLES=%d SEED=%d CUTOFF=1e-6 NOISE=0 JOBS=%d" % (samples, seed, jobs)
    lines = ["tools/time_local_energy.py --quality: make local_energy MODEL=<model> ORDER=<order> SIGNS=<signs> "
             "[EXTERNAL_FIELD=1] " + settings,
             "samples drawn from |psi|^2 of the exact ground state; mean = count-weighted mean of E_loc over the "
             "samples, +- its standard error; exact: the ground state's own signs (independent of ORDER and "
             "EXTERNAL_FIELD, run once)", ""]
    with tempfile.TemporaryDirectory() as tmp:
        for model in ("heisenberg_kagome_16", "heisenberg_kagome_18"):
            runs = [("exact", 0, False)] + [("greedy", order, field) for order in range(3) for field in (False, True)]
            for signs, order, field in runs:
                command = ["make", "-s", "local_energy", "MODEL=" + model, "ORDER=%d" % order, "SIGNS=" + signs,
                           "OUT=" + tmp, "PYTHON=" + sys.executable] + settings.split()
                command += ["EXTERNAL_FIELD=1"] if field else []
                started = time.perf_counter()
                subprocess.run(command, check=True, cwd=ROOT, timeout=900, stdout=subprocess.DEVNULL)
                seconds = time.perf_counter() - started
                name = "%s_order%d_%s%s.csv" % (model, order, signs, "_field" if field else "")
                head = {}
                with open(os.path.join(tmp, "local_energy", name)) as f:
                    for line in f:
                        if line.startswith("# ") and " = " in line:
                            key, value = line[2:].strip().split(" = ", 1)
                            head[key] = value
                rows = np.loadtxt(os.path.join(tmp, "local_energy", name), delimiter=",", comments="#", ndmin=2)
                mean, error, e0 = float(head["mean"]), float(head["standard_error"]), float(head["E0"])
                # (with exact signs every sample sits at E0 and the spread is rounding noise: no ratio then)
                sigmas = ("%+.1f standard errors" % ((mean - e0) / error) if error > 1e-9 * abs(mean)
                          else "spread at rounding level")
                lines.append("%-21s signs=%-6s order %d %-15s mean %+.6f +- %.3g   E0 %+.6f   mean - E0 = %+.3g (%s); "
                             "%d unique samples, mean cluster %.1f states, missing %s; %.1f s"
                             % (model, signs, order, "external field" if field else "", mean, error, e0, mean - e0,
                                sigmas, rows.shape[0], rows[:, 1].mean(), head["missing_total"], seconds))
                print(lines[-1], flush=True)
            lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "local_energy_timing.txt"))
    parser.add_argument("--quality", action="store_true")
    parser.add_argument("--quality-output", default=os.path.join(ROOT, "profiles", "local_energy_quality.txt"))
    parser.add_argument("--quality-samples", type=int, default=1000)
    parser.add_argument("--quality-seed", type=int, default=435834)
    parser.add_argument("--quality-jobs", type=int, default=16)
    args = parser.parse_args()
    if args.quality:
        return quality(args.quality_output, args.quality_samples, args.quality_seed, args.quality_jobs)
    lines = ["tools/time_local_energy.py --runs %d" % args.runs,
             "device time (asp_operator_last_ms: HIP events around the launches — hash build, connection list where "
             "there is one, and the row kernel; no host<->HBM copies) of the local energies", ""]
    plain = operators.Operator.from_config(synthetic.kagome_lattice())
    for count in (10_000, 100_000):
        keys = random_keys(count, count)
        measure(lines, "36-site kagome, 72 bonds, plain basis, one segment (k_eloc_rows)", plain, keys, signed(keys),
                np.array([0, keys.size], dtype=np.uint64), np.arange(keys.size, dtype=np.uint64), args.runs, field=True)
    keys, offsets, rows = neighbourhood_segments(plain, random_keys(50_000, 50))
    measure(lines, "36-site kagome, plain basis, one-hop neighbourhoods, one row each (k_eloc_rows)", plain, keys,
            signed(keys), offsets, rows, args.runs)
    sector = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_36"])
    representatives, _, norm = sector.device().state_info(random_keys(10_000, 7))
    keys = np.unique(representatives[norm > 0])
    measure(lines, "heisenberg_kagome_36, symmetry sector, one segment (k_eloc_list)", sector, keys, signed(keys),
            np.array([0, keys.size], dtype=np.uint64), np.arange(keys.size, dtype=np.uint64), args.runs, host_rows=500)
    with open(args.output, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
