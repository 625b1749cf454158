"""Timing of the bond statistics on the GPU: the row pass (asp_bonds_create /
asp_bonds_set_signs), a 49-bin histogram and the sorted magnitudes, from asp_bonds_last_ms, beside the
host time of the numpy route on the same matrix and the bytes each pass must read.

    python tools/time_bonds.py [--rounds 5] [--output profiles/bond_stats_timing.txt]

Method: one warm-up call, then `rounds` calls each; device times are HIP events around the kernels
(copies excluded), host times a wall clock around the reference's numpy formulas.  Bytes: 12 B per
stored entry (column and value) plus the sign words; the row pointers (8 B per row) are not counted."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import common, operators, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402
from annealing_sign_problem_amd.bonds import BondStatistics, log_edges  # noqa: E402


def numpy_route(exchange, signs, edges_log):
    """The reference's formulas (common.py:977-995, 955-959): (histogram seconds, sort seconds)."""
    tick = time.perf_counter()
    matrix = exchange.tocoo()
    keep = (matrix.row != matrix.col) & (matrix.data != 0)
    row, col, data = matrix.row[keep], matrix.col[keep], matrix.data[keep]
    is_frustrated = signs[row] * signs[col] * data > 0
    logs = np.log(np.abs(data))
    np.histogram(logs[is_frustrated], bins=edges_log)
    np.histogram(logs[~is_frustrated], bins=edges_log)
    histogram = time.perf_counter() - tick
    tick = time.perf_counter()
    np.sort(np.abs(data))[::-1]
    return histogram, time.perf_counter() - tick


def measure(name, exchange, bits, rounds, emit):
    n = exchange.shape[0]
    signs = sa.bits_to_signs(bits, n)
    stats = BondStatistics(exchange, bits)
    summary = stats.summary
    hi = np.log(summary["max_abs"])
    lo = max(hi - 20.0, np.log(summary["min_abs"]))
    edges = log_edges(lo, hi, 50)
    bytes_read = 12 * summary["stored"] + 8 * ((n + 63) // 64)
    rows_ms, hist_ms, sort_ms = [], [], []
    for k in range(rounds + 1):
        stats.set_signs(bits)
        rows_ms.append(stats.last_ms())
        stats.histogram(edges)
        hist_ms.append(stats.last_ms())
        stats.magnitudes()
        sort_ms.append(stats.last_ms())
    stats.release()
    host_hist, host_sort = numpy_route(exchange, signs, np.linspace(lo, hi, 50))
    lengths = np.diff(exchange.indptr)
    emit("%s: %d rows, %d stored, %d bonds, %.4f frustrated; longest row %d, mean %.1f; %.2f MB per pass"
         % (name, n, summary["stored"], summary["bonds"], summary["frustrated"] / summary["bonds"],
            lengths.max(), lengths.mean(), bytes_read / 1e6))
    for label, times, host in (("row pass", rows_ms, None), ("histogram(49)", hist_ms, host_hist),
                               ("magnitudes", sort_ms, host_sort)):
        times = np.asarray(times[1:])
        line = "  %-14s device ms %s  median %.4f" % (label, " ".join("%.4f" % t for t in times), np.median(times))
        if label != "magnitudes":
            line += "  = %.1f GB/s" % (bytes_read / (np.median(times) * 1e-3) / 1e9)
        if host is not None:
            line += "  | numpy on the host %.1f ms" % (host * 1e3)
        emit(line)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--planted", type=int, default=100000)
    parser.add_argument("--output", default=None)
    args = parser.parse_args(argv)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    matrix, _, planted = synthetic.planted_cluster(args.planted)
    measure("planted_cluster(%d)" % args.planted, matrix, sa.signs_to_bits(planted), args.rounds, emit)
    operator = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_16"])
    operator.basis.build()
    _, ground_state = operator.ground_state()
    model = common.make_ising_model(operator.basis.states, operator,
                                    log_psi_fn=common.ground_state_to_log_coeff_fn(ground_state, operator.basis))
    measure("heisenberg_kagome_16 (whole basis)", model.ising_hamiltonian.exchange, model.initial_signs,
            args.rounds, emit)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
