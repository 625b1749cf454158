"""Device time of the boundary field (asp_operator_field) beside the fused coupling build
(asp_operator_ising_csr) on the same clusters, both from asp_operator_last_ms: K = 1e4 and 1e5 random keys of
hamming weight 18 of the 36-site kagome operator (72 bonds, no lattice symmetries: k_field_rows; and, at K = 1e4,
the representatives of the same keys in the model's symmetry sector: k_field_list), the environment their one-hop
extension with hashed amplitudes.  RUNS calls per side after a warm-up (median, min .. max).  The first cluster's
field is compared with the sequential law on 200 of its rows before anything is timed.  Writes --output (default
profiles/field_timing.txt).

With --quality: runs `sampled_components --model heisenberg_kagome_16 --order 2` with and without
--external-field on one seed (child processes) and writes the mean greedy and SA overlap per order to
--quality-output (default profiles/field_quality.txt).  (Development aid; GPU.)

    python tools/time_field.py [--runs 5] [--output FILE] [--quality] [--quality-output FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from annealing_sign_problem_amd import operators, synthetic  # noqa: E402


def random_keys(count, seed, sites=36, weight=18):
    rng = np.random.default_rng(seed)
    keys = np.zeros(0, dtype=np.uint64)
    while keys.size < count:
        order = np.argsort(rng.random((2 * count, sites)), axis=1)[:, :weight].astype(np.uint64)
        fresh = np.bitwise_or.reduce(np.uint64(1) << order, axis=1)
        keys = np.unique(np.concatenate([keys, fresh]))
    return np.sort(rng.permutation(keys)[:count])


def amplitudes(keys):
    return np.ascontiguousarray(np.exp(synthetic.hashed_log_amplitudes(keys)).real)


def law_rows(op, keys, psi, env_keys, env_psi, rows, scale):
    """The sequential law (tests/field_cases.py: field_law) on some rows."""
    other, coeffs, counts = op.batched_apply(keys[rows])
    other, coeffs = other[:, 0], coeffs.real
    out, e = np.zeros(rows.size), 0
    for i, r in enumerate(rows):
        acc = 0.0
        for _ in range(int(counts[i])):
            at = np.searchsorted(keys, other[e])
            if not (at < keys.size and keys[at] == other[e]):
                p = np.searchsorted(env_keys, other[e])
                if p < env_keys.size and env_keys[p] == other[e]:
                    acc = acc + ((float(coeffs[e]) * abs(float(psi[r]))) * float(env_psi[p]))
            e += 1
        out[i] = scale * acc
    return out


def measure(lines, label, op, keys, runs, check):
    device = op.device()
    norm = np.linalg.norm(amplitudes(keys))
    psi = amplitudes(keys) / norm
    env_keys = device.extend(keys)
    env_psi = amplitudes(env_keys) / norm
    field, unresolved = device.field(keys, psi, env_keys, env_psi)  # warm-up
    assert unresolved == 0
    if check:
        rows = np.arange(0, keys.size, max(1, keys.size // 200))
        want = law_rows(op, keys, psi, env_keys, env_psi, rows, 2.0)
        assert np.array_equal(field[rows].view(np.uint64), want.view(np.uint64)), "the field is not the law's"
    device.ising_csr(keys, psi)
    field_ms, build_ms, nnz = [], [], 0
    for _ in range(runs):
        device.field(keys, psi, env_keys, env_psi)
        field_ms.append(device.last_ms)
        nnz = device.ising_csr(keys, psi)[1].size
        build_ms.append(device.last_ms)

    def stats(ms):
        return "%8.3f ms (min %.3f, max %.3f)" % (statistics.median(ms), min(ms), max(ms))

    lines.append("%s: K = %d, E = %d environment states, %d couplings, %d rows with a non-zero field, %d calls per side"
                 % (label, keys.size, env_keys.size, nnz, np.count_nonzero(field), runs))
    lines.append("  asp_operator_field      %s" % stats(field_ms))
    lines.append("  asp_operator_ising_csr  %s" % stats(build_ms))
    lines.append("    field / build: %.2fx" % (statistics.median(field_ms) / statistics.median(build_ms)))
    lines.append("")
    print("\n".join(lines[-5:]), flush=True)


def quality(path, samples, seed):
    """Mean overlaps of the driver with and without --external-field, one seed."""
    lines = ["tools/time_field.py --quality: python -m annealing_sign_problem_amd.sampled_components --model "
             "heisenberg_kagome_16 --order 2 --number-samples %d --seed %d [--external-field]; mean over the "
             "clusters, per order (0: the cluster, 1 and 2: its extensions)" % (samples, seed), ""]
    with tempfile.TemporaryDirectory() as tmp:
        for flag in ([], ["--external-field"]):
            out = os.path.join(tmp, "with.csv" if flag else "without.csv")
            command = [sys.executable, "-m", "annealing_sign_problem_amd.sampled_components", "--model",
                       "heisenberg_kagome_16", "--order", "2", "--number-samples", str(samples), "--seed", str(seed),
                       "--output", out] + flag
            subprocess.run(command, check=True, cwd=ROOT, timeout=900)
            rows = np.loadtxt(out, delimiter=",", comments="#", ndmin=2)
            lines.append("with --external-field:" if flag else "without:")
            for order in range(3):
                size, _, greedy, _, sa, _ = (rows[:, 6 * order + c] for c in range(6))
                lines.append("  order %d: %d clusters, mean size %7.1f, greedy overlap %.4f, SA overlap %.4f"
                             % (order, rows.shape[0], size.mean(), greedy.mean(), sa.mean()))
            lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "field_timing.txt"))
    parser.add_argument("--quality", action="store_true")
    parser.add_argument("--quality-output", default=os.path.join(ROOT, "profiles", "field_quality.txt"))
    parser.add_argument("--quality-samples", type=int, default=40)
    parser.add_argument("--quality-seed", type=int, default=12345)
    args = parser.parse_args()
    lines = ["tools/time_field.py --runs %d" % args.runs,
             "device time (asp_operator_last_ms: HIP events around the launches, no host<->HBM copies) of the boundary "
             "field beside the fused coupling build on the same cluster", ""]
    plain = operators.Operator.from_config(synthetic.kagome_lattice())
    for count in (10_000, 100_000):
        measure(lines, "36-site kagome, 72 bonds, plain basis (k_field_rows)", plain, random_keys(count, count),
                args.runs, check=count == 10_000)
    sector = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_36"])
    representatives, _, norm = sector.device().state_info(random_keys(10_000, 7))
    measure(lines, "heisenberg_kagome_36, symmetry sector (k_field_list)", sector,
            np.unique(representatives[norm > 0]), args.runs, check=False)
    with open(args.output, "w") as f:
        f.write("\n".join(lines))
    if args.quality:
        quality(args.quality_output, args.quality_samples, args.quality_seed)


if __name__ == "__main__":
    main()
