"""Timing of the sign scores on the GPU against the host route they replace, the loop
over common.compute_accuracy_and_overlap on 1 and on 16 threads:

  trial      one trial of `make small`: K = 12 870 spins x 1024 chains, one sign_scores call
  rounds     64 / 256 / 1024 cluster solutions of kagome_36 size (log-uniform 50 .. 1000 spins, one
             configuration each) through compute_accuracies_and_overlaps (one batch call)
  distances  K = 10^4 and 10^5 x 1024 chains against a numpy popcount

    python tools/time_sign_scores.py [--rounds 5] [--output profiles/sign_scores_timing.txt]

Method: one warm-up call of every shape, then `rounds` calls; "device" is asp_sign_scores_last_ms (HIP
events around the kernels, no copies), "wall" a host clock around the Python call, which ends in a device
synchronise and holds the copies.  Medians.  Inputs are random: the time does not depend on the content."""
from __future__ import annotations

import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import common, scores  # noqa: E402


def _words(spins: int) -> int:
    return (spins + 63) // 64


_BYTE_BITS = np.array([bin(b).count("1") for b in range(256)], dtype=np.uint8)


def _popcount(words: np.ndarray) -> np.ndarray:
    """Set bits per 64-bit word: np.bitwise_count (numpy 2), else a table over the bytes."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(words)
    return _BYTE_BITS[words.view(np.uint8)].reshape(words.shape + (8,)).sum(axis=-1, dtype=np.uint8)


def _random_problem(rng, spins: int, count: int):
    xs = rng.integers(0, 2**63, size=(count, _words(spins)), dtype=np.uint64) << np.uint64(1)
    exact = rng.integers(0, 2**63, size=_words(spins), dtype=np.uint64) << np.uint64(1)
    weights = np.exp(rng.normal(0.0, 3.0, size=spins)) ** 2
    weights /= np.sum(weights)
    return xs, exact, weights


def _median_ms(function, rounds: int):
    """(median wall ms, median device ms) of `function` after one warm-up call."""
    function()
    wall, device = [], []
    for _ in range(rounds):
        tick = time.perf_counter()
        function()
        wall.append((time.perf_counter() - tick) * 1e3)
        device.append(scores.last_ms())
    return float(np.median(wall)), float(np.median(device))


def _host_loop_ms(triples, threads: int, rounds: int) -> float:
    """The parent route: one compute_accuracy_and_overlap call per configuration."""
    def one(t):
        return common.compute_accuracy_and_overlap(*t)

    def run():
        if threads == 1:
            return [one(t) for t in triples]
        with ThreadPoolExecutor(max_workers=threads) as pool:
            return list(pool.map(one, triples, chunksize=max(1, len(triples) // (4 * threads))))

    run()
    times = []
    for _ in range(rounds):
        tick = time.perf_counter()
        run()
        times.append((time.perf_counter() - tick) * 1e3)
    return float(np.median(times))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--output", default=None)
    parser.add_argument("--skip-large-numpy", action="store_true",
                        help="leave out the numpy popcount at K = 10^5 (it takes several seconds per round)")
    args = parser.parse_args(argv)
    rng = np.random.default_rng(7)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("| leg | shape | device: wall / kernels ms | host loop, 1 thread ms | host loop, 16 threads ms | host / device wall, 1 / 16 threads |")
    emit("|---|---|---|---|---|---|")

    xs, exact, weights = _random_problem(rng, 12870, 1024)
    wall, device = _median_ms(lambda: scores.accuracy_and_overlap(xs, exact, weights), args.rounds)
    triples = [(x, exact, weights) for x in xs]
    one, many = _host_loop_ms(triples, 1, args.rounds), _host_loop_ms(triples, 16, args.rounds)
    emit("| trial | K = 12870 x 1024 chains | %.3f / %.3f | %.2f | %.2f | %.1fx / %.1fx |"
         % (wall, device, one, many, one / wall, many / wall))

    for count in (64, 256, 1024):
        sizes = np.exp(rng.uniform(np.log(50), np.log(1000), size=count)).astype(int)
        problems = [_random_problem(rng, int(k), 1) for k in sizes]
        predicted = [p[0][0] for p in problems]
        exacts, weight_list = [p[1] for p in problems], [p[2] for p in problems]
        wall, device = _median_ms(lambda: common.compute_accuracies_and_overlaps(predicted, exacts, weight_list),
                                  args.rounds)
        triples = list(zip(predicted, exacts, weight_list))
        one, many = _host_loop_ms(triples, 1, args.rounds), _host_loop_ms(triples, 16, args.rounds)
        emit("| round | %d solutions, %d spins in all | %.3f / %.3f | %.2f | %.2f | %.1fx / %.1fx |"
             % (count, int(sizes.sum()), wall, device, one, many, one / wall, many / wall))

    for spins in (10**4, 10**5):
        xs, _, _ = _random_problem(rng, spins, 1024)
        wall, device = _median_ms(lambda: scores.sign_distances(xs, spins), args.rounds)
        if spins > 10**4 and args.skip_large_numpy:
            emit("| distances | K = %d x 1024 chains | %.3f / %.3f | not measured | - | - |" % (spins, wall, device))
            continue
        masked = xs.copy()
        if spins % 64:
            masked[:, -1] &= np.uint64((1 << (spins % 64)) - 1)

        def numpy_popcount():
            out = np.zeros((1024, 1024), dtype=np.uint32)
            for a in range(1024):  # (row by row: the whole [C, C, W] array does not fit)
                out[a] = _popcount(masked ^ masked[a]).sum(axis=1, dtype=np.uint32)
            return out

        assert np.array_equal(numpy_popcount(), scores.sign_distances(xs, spins))
        tick = time.perf_counter()
        numpy_popcount()
        host = (time.perf_counter() - tick) * 1e3
        emit("| distances | K = %d x 1024 chains | %.3f / %.3f | %.1f (numpy popcount, once) | - | %.0fx |"
             % (spins, wall, device, host, host / wall))

    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
