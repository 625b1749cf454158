"""Batched isoenergetic cluster moves (asp_sa_chains_cluster_move_batch, DESIGN.md §4.13 "Batched form") on
the models the pipeline makes: sampled clusters of heisenberg_kagome_16, extended to order 1 and cut at 1e-6.

    python tools/time_cluster_move_batch.py [--rounds 64,256,1024] [--chains 64] [--repeat 5]
                                            [--tempering-rounds 40] [--quality-samples 128]
                                            [--quality-sweeps 1280] [--output FILE]

(a) Speed.  Per round size N: N handles of --chains chains, one ladder segment of ten sweeps with every
    chain at the model's cold end (beta1_auto), then ONE cluster move of the pairs (k, chains - 1 - k) on
    four routes from the same snapshots (load_state, not timed): the batched call, the batched call with
    ASP_CLUSTER_NO_PACKED on every item (a workgroup per pair), a loop of Chains.cluster_move on one host
    thread and the same loop on 16 host threads.  Wall time of each, the device time of the batched calls
    (asp_sa_chains_cluster_move_batch_last_ms) and, for the loop on one thread, the sum of the calls' device
    times (asp_sa_chains_cluster_move_last_ms) — median and spread over --repeat moves after a warm-up.  The
    routes are checked to leave the same bits first.
(b) Percolation.  |C| / n per move — the flipped cluster's share of the differing sites — and n / K on those
    models: for the cold snapshots of (a), and per rung over --tempering-rounds rounds of
    parallel_tempering_cluster_batch's loop (hairpin ladder, ten sweeps, a move on every rung, an exchange),
    second half of the rounds.  The same for planted clusters of mean degree 24, where DESIGN.md §4.13
    found the differing sites to percolate.
(c) Solver quality.  One sampled_components round of --quality-samples clusters at order 1: the sign
    accuracy of the greedy solver and of common.solve_ising_models with method "anneal", "tempering" and
    "tempering-cluster" at --quality-sweeps sweeps and 64 chains each, per order.

Everything is printed and, with --output, written to that file too, line by line (profiles/cluster_move_batch_timing.txt
is the record).
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import _lib, build, common, sampled_components, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")
MODEL = "heisenberg_kagome_16"
CUTOFF = "1e-6"
OUTPUT = [None]


def say(text=""):
    print(text, flush=True)
    if OUTPUT[0]:
        with open(OUTPUT[0], "a") as f:  # (line by line: what a run got to is on file)
            f.write(text + "\n")


def spread(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def same(a, b):
    return all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in STATE)


def quantiles(values):
    q = np.quantile(np.asarray(values, dtype=np.float64), [0.1, 0.25, 0.5, 0.75, 0.9])
    return "10%% %.3f  25%% %.3f  median %.3f  75%% %.3f  90%% %.3f" % tuple(q)


def sampled_round(count, seed=12345):
    """(args, operator, ground state, amplitude closure, clusters) of `count` sampled clusters."""
    args = sampled_components.parse_command_line(["--model", MODEL, "--order", "1", "--global-cutoff", CUTOFF,
                                                  "--number-samples", str(count), "--seed", str(seed),
                                                  "--output", "unused.csv"])
    operator, ground_state = sampled_components.load_input(args)
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, operator.basis)
    np.random.seed(args.seed)
    clusters = list(sampled_components.generate_clusters(operator, ground_state, args.number_samples,
                                                         args.sampled_power, args.min_cluster_size,
                                                         args.max_cluster_size, args.keep_probability))
    return args, operator, ground_state, log_coeff_fn, clusters


def order_one_hamiltonians(count):
    args, operator, _, log_coeff_fn, clusters = sampled_round(count)
    models = common.make_ising_models(clusters, operator, log_psi_fn=log_coeff_fn)
    models = common.extend_and_sparsify_models(models, log_coeff_fn, args.global_cutoff, clusters)
    return [m.ising_hamiltonian for m in models]


def describe(hams):
    sizes = np.array([h.size for h in hams])
    degrees = np.array([h.exchange.nnz / max(h.size, 1) for h in hams])
    return "%d models, %d..%d spins (median %d, %d in all), stored entries per row: median %.1f, max %.1f; " \
           "%d of them at most 2048 spins (a wavefront per pair)" % (
               len(hams), sizes.min(), sizes.max(), int(np.median(sizes)), sizes.sum(), np.median(degrees),
               degrees.max(), int(np.count_nonzero(sizes <= 2048)))


def open_cold(hams, chains, sweeps=10):
    """Handles after one segment with every chain at the model's cold end, and their snapshots."""
    sa.plan_hamiltonians(hams)
    handles = [sa.Chains(h, seed=1 + k, repetitions=chains) for k, h in enumerate(hams)]
    cold = [np.full(chains, h.info().beta1_auto) for h in hams]
    sa.advance_ladder_chains(handles, cold, sweeps, sweep_order="shuffled")
    return handles, [c.state() for c in handles]


def speed(hams, chains, repeat):
    lib = _lib.load()
    n = len(hams)
    handles, snapshots = open_cold(hams, chains)
    pairs = np.array([(k, chains - 1 - k) for k in range(chains // 2)], dtype=np.uint32)

    def restore():
        for c, s in zip(handles, snapshots):
            c.load_state(s)

    def batched(flags):
        t0 = time.perf_counter()
        sa.cluster_move_chains(handles, [pairs] * n, 0, flags)
        wall = (time.perf_counter() - t0) * 1e3
        return wall, float(lib.asp_sa_chains_cluster_move_batch_last_ms())

    def one(c):
        c.cluster_move(pairs, 0)
        return float(lib.asp_sa_chains_cluster_move_last_ms())  # (this thread's last call)

    def singles(threads):
        t0 = time.perf_counter()
        if threads == 1:
            device = [one(c) for c in handles]
        else:
            with ThreadPoolExecutor(max_workers=threads) as pool:
                device = list(pool.map(one, handles))
        return (time.perf_counter() - t0) * 1e3, sum(device)

    routes = {"batched call": lambda: batched(0),
              "batched call, ASP_CLUSTER_NO_PACKED": lambda: batched(sa.CLUSTER_NO_PACKED),
              "loop of single calls, 1 host thread": lambda: singles(1),
              "loop of single calls, 16 host threads": lambda: singles(16)}
    figures = {name: [] for name in routes}
    for k in range(repeat + 1):
        ends = []
        for name, call in routes.items():  # (the routes alternate within a repetition)
            restore()
            row = call()
            ends.append([c.state() for c in handles])
            if k:  # (the first repetition warms up)
                figures[name].append(row)
        for other in ends[1:]:
            if not all(same(x, y) for x, y in zip(ends[0], other)):
                raise SystemExit("the routes do NOT leave the same bits")
    say("  " + describe(hams))
    say("  %d chains, %d pairs per handle: %d pairs per move" % (chains, len(pairs), n * len(pairs)))
    for name, rows in figures.items():
        wall, device = zip(*rows)
        what = "device" if name.startswith("batched") else "device, sum of the calls"
        if name.endswith("16 host threads"):
            say("    %-38s: wall %s  (device spans overlap: NOT MEASURED)" % (name, spread(wall)))
        else:
            say("    %-38s: wall %s  %s %s" % (name, spread(wall), what, spread(device)))
    med = {name: statistics.median([row[0] for row in rows]) for name, rows in figures.items()}
    names = list(med)
    say("    wall, loop on 1 thread / batched: %.2f   loop on 16 threads / batched: %.2f   batched NO_PACKED / "
        "batched: %.2f" % (med[names[2]] / med[names[0]], med[names[3]] / med[names[0]], med[names[1]] / med[names[0]]))
    dev = {name: statistics.median([row[1] for row in rows]) for name, rows in figures.items()}
    say("    device, batched NO_PACKED / batched: %.2f   sum of the single calls / batched: %.2f" % (
        dev[names[1]] / dev[names[0]], dev[names[2]] / dev[names[0]]))
    for c in handles:
        c.close()


def shares(differing, sizes, spins):
    """(|C| / n of the moves with n > 0, n / K of all moves, the moves) of per-handle outputs."""
    ratio, density, moves = [], [], 0
    for d, s, K in zip(differing, sizes, spins):
        d, s = np.asarray(d, dtype=np.float64), np.asarray(s, dtype=np.float64)
        moves += d.size
        density.extend(d / K)
        ratio.extend(s[d > 0] / d[d > 0])
    return np.array(ratio), np.array(density), moves


def report_shares(label, ratio, density, moves):
    if ratio.size == 0:
        say("    %-30s: %d moves, no pair differs" % (label, moves))
        return
    say("    %-30s: %d moves, %.1f %% with n = 0;  n / K: %s" % (
        label, moves, 100.0 * (moves - ratio.size) / moves, quantiles(density)))
    say("    %-30s  |C| / n: %s;  mean %.3f;  |C| = n in %.1f %%, |C| / n >= 0.9 in %.1f %%, <= 0.5 in %.1f %% "
        "of the moves with n > 0" % ("", quantiles(ratio), ratio.mean(), 100.0 * np.mean(ratio == 1.0),
                                     100.0 * np.mean(ratio >= 0.9), 100.0 * np.mean(ratio <= 0.5)))


def percolation(hams, chains, rounds, label):
    n = len(hams)
    spins = [h.size for h in hams]
    rungs = chains // 2
    pairs = np.array([(k, chains - 1 - k) for k in range(rungs)], dtype=np.uint32)
    say("  %s: %s" % (label, describe(hams)))
    handles, _ = open_cold(hams, chains)
    out = sa.cluster_move_chains(handles, [pairs] * n, 0)
    report_shares("all chains cold, ten sweeps", *shares([o[0] for o in out], [o[1] for o in out], spins))
    for c in handles:
        c.close()
    # the driver's loop (hairpin ladder: pair k is rung k, the last rungs are the cold ones)
    hairpins = []
    for h in hams:
        info = h.info()
        ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, rungs)
        hairpins.append(np.concatenate([ladder, ladder[::-1]]))
    handles = [sa.Chains(h, seed=101 + k, repetitions=chains) for k, h in enumerate(hams)]
    kept = []
    for j in range(rounds):
        sa.advance_ladder_chains(handles, hairpins, 10, sweep_order="shuffled")
        out = sa.cluster_move_chains(handles, [pairs] * n, 0)
        if j >= rounds // 2:
            kept.append(out)
        if j + 1 < rounds:
            sa.exchange_chains(handles, hairpins, j & 1, 0)
    for c in handles:
        c.close()
    groups = (("coldest rung", [rungs - 1]), ("4 coldest rungs", range(rungs - 4, rungs)),
              ("colder half of the ladder", range(rungs // 2, rungs)), ("hotter half of the ladder", range(rungs // 2)))
    say("    tempering with moves, rounds %d..%d of %d (ten sweeps each):" % (rounds // 2, rounds - 1, rounds))
    for name, which in groups:
        which = list(which)
        d = [np.concatenate([out[i][0][which] for out in kept]) for i in range(n)]
        s = [np.concatenate([out[i][1][which] for out in kept]) for i in range(n)]
        report_shares(name, *shares(d, s, spins))


def quality(samples, sweeps):
    args, operator, ground_state, log_coeff_fn, clusters = sampled_round(samples, seed=777)
    staged = sampled_components.stage_clusters(clusters, operator, ground_state, ground_state, log_coeff_fn, 1,
                                               args.global_cutoff, greedy_batch=True, build_batch=True,
                                               level_batch=True)
    models = [m for _, m, _, _, _ in staged]
    frozen = [clusters[c] for c, _, _, _, _ in staged]
    order_of = np.array([k % 2 for k in range(len(staged))])  # (stage_clusters: order 0, 1 of cluster 0, then ...)
    assert all(staged[k][0] == k // 2 for k in range(len(staged)))
    say("  %d clusters (%d..%d states), models of order 0 (%d..%d spins) and order 1 (%d..%d spins), cutoff %s, "
        "%d sweeps, 64 chains, shuffled order, seed 12345" % (
            len(clusters), min(len(c) for c in clusters), max(len(c) for c in clusters),
            min(m.size for m in models[0::2]), max(m.size for m in models[0::2]),
            min(m.size for m in models[1::2]), max(m.size for m in models[1::2]), CUTOFF, sweeps))

    def report(name, accuracy, seconds=None):
        accuracy = np.asarray(accuracy, dtype=np.float64)
        parts = []
        for order in (0, 1):
            a = accuracy[order_of == order]
            parts.append("order %d: mean %.5f  median %.5f  min %.5f  exact in %5.1f %%" % (
                order, a.mean(), np.median(a), a.min(), 100.0 * np.mean(a == 1.0)))
        say("    %-18s %s%s" % (name, "   ".join(parts), "" if seconds is None else "   solve %.1f s" % seconds))

    report("greedy", [r.greedy_accuracy for _, _, _, _, r in staged])
    for method in ("anneal", "tempering", "tempering-cluster"):
        started = time.perf_counter()
        solutions = common.solve_ising_models(models, frozen, number_sweeps=sweeps, repetitions=64,
                                              sweep_order="shuffled", method=method)
        seconds = time.perf_counter() - started
        report(method, [a for a, _ in sampled_components.score_solutions(staged, solutions)], seconds)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", default="64,256,1024")
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--tempering-rounds", type=int, default=40)
    p.add_argument("--percolation-models", type=int, default=256)
    p.add_argument("--quality-samples", type=int, default=128)
    p.add_argument("--quality-sweeps", type=int, default=1280)
    p.add_argument("--output", default=None)
    a = p.parse_args()
    _lib.require_gpu()
    if a.output:
        OUTPUT[0] = a.output
        open(a.output, "w").close()
    rounds = [int(x) for x in a.rounds.split(",") if x]
    say("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
    started = time.perf_counter()
    hams = order_one_hamiltonians(max(rounds + [a.percolation_models]))
    say("%s order 1, cutoff %s: %d sampled clusters grown and their models built in %.1f s" % (
        MODEL, CUTOFF, len(hams), time.perf_counter() - started))
    say()
    say("(a) one cluster move of a round: %d repetitions after a warm-up, the routes alternating" % a.repeat)
    for count in rounds:
        say("  round of %d handles" % count)
        speed(hams[:count], a.chains, a.repeat)
    say()
    say("(b) the flipped cluster's share of the differing sites")
    percolation(hams[:a.percolation_models], a.chains, a.tempering_rounds, "sampled clusters")
    planted = []
    for k in range(16):
        J, h, _ = synthetic.planted_cluster(500, seed=1000 + k)
        planted.append(sa.Hamiltonian(J, h))
    percolation(planted, a.chains, a.tempering_rounds, "planted clusters (mean degree 24)")
    say()
    say("(c) sign accuracy of one sampled_components round")
    quality(a.quality_samples, a.quality_sweeps)


if __name__ == "__main__":
    main()
