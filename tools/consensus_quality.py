"""Does the consensus vote (law ASP-VOTE-1) recover more signs than the chain of lowest
energy, and what does it cost?  Three sections, written to profiles/consensus_quality.txt:

  quality   full-basis models (default heisenberg_kagome_16 and sk_16_1, K = 12 870), 1024 chains, `trials`
            anneals per sweep count in the default sweep order: sign accuracy and overlap of the best chain,
            of the uniform vote and of the Boltzmann vote at the schedule's last beta, each with 1 and 2 rounds
  clusters  sampled_components on kagome_16 clusters at orders 0-2, --anneal-select best against consensus
  timing    the vote on the device (asp_sign_vote_last_ms, and the wall time of the Python call) beside the
            numpy restatement of tests/vote_cases.py on configurations that are on the host already, for
            R = 64 / 1024 and K = 1e3 / 1e5; and a round of resident handles through consensus_chains against
            the loop of single calls and against export + numpy

    python tools/consensus_quality.py [--sections quality,clusters,timing] [--models a,b] [--sweeps 100,1600,25600]
                                      [--trials 10,10,10] [--chains 1024] [--clusters 256] [--handles 256] [--rounds 5]
                                      [--output profiles/consensus_quality.txt] [--append]

Method of the timings: one warm-up call of every shape, then `rounds` calls, medians; "kernels" is
asp_sign_vote_last_ms (HIP events around the launches, no copies), "wall" a host clock around the Python call,
which ends in a device synchronise and holds the copies.  The settings of a run are written with its numbers."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vote_cases  # noqa: E402  (the numpy restatement of the law)

from annealing_sign_problem_amd import annealer as sa  # noqa: E402
from annealing_sign_problem_amd import full_hilbert_space, sampled_components, scores, synthetic  # noqa: E402

CHAINS = 1024


def quality(emit, models, sweeps, trials, seed, chains=CHAINS):
    emit("## quality: %d chains, default sweep order; mean over the trials of accuracy / overlap, and the fraction "
         "of trials with accuracy > 0.995" % chains)
    emit("| model | sweeps | trials | best chain | uniform vote, 1 round | uniform, 2 rounds | Boltzmann vote, 1 round "
         "| Boltzmann, 2 rounds | flipped chains (mean) | sites changed by round 2 (uniform, mean) |")
    emit("|---|---|---|---|---|---|---|---|---|---|")
    for model in models:
        simulation = full_hilbert_space.Simulation(model)
        ham = simulation.exact_model.ising_hamiltonian
        exact, weights, spins = simulation.exact_model.initial_signs, simulation.weights, ham.size
        beta = float(ham.info().beta1_auto)
        for number_sweeps, count in zip(sweeps, trials):
            rows, flipped, changed = [], [], []
            for trial in range(count):
                xs, es = sa.anneal(ham, seed=seed + 1000 * trial + number_sweeps, number_sweeps=number_sweeps,
                                   repetitions=chains, only_best=False)
                best = int(np.argmin(es))
                boltzmann = scores.vote_weights(es, beta)
                votes = scores.consensus_batch([(xs, spins, None, None, best, True, 1),
                                                (xs, spins, None, None, best, True, 2),
                                                (xs, spins, boltzmann, None, best, True, 1),
                                                (xs, spins, boltzmann, None, best, True, 2)])
                configurations = np.stack([xs[best]] + [v.x for v in votes])
                accuracy, overlap = scores.accuracy_and_overlap(configurations, exact, weights, spins)
                rows.append(np.stack([accuracy, overlap], axis=1))
                flipped.append(votes[0].flipped.sum())
                changed.append(votes[1].changed)
            rows = np.array(rows)  # [trial, configuration, (accuracy, overlap)]
            cells = ["%.4f / %.4f, %.2f" % (rows[:, k, 0].mean(), rows[:, k, 1].mean(), (rows[:, k, 0] > 0.995).mean())
                     for k in range(5)]
            emit("| %s | %d | %d | %s | %.1f | %.1f |" % (model, number_sweeps, count, " | ".join(cells),
                                                          np.mean(flipped), np.mean(changed)))


def clusters(emit, number, seed):
    emit("## clusters: sampled_components on heisenberg_kagome_16, %d clusters, orders 0-2, the SA columns with "
         "--anneal-select best and consensus (mean / median over the clusters)" % number)
    emit("| order | accuracy, best | accuracy, consensus | overlap, best | overlap, consensus | seconds, best / consensus |")
    emit("|---|---|---|---|---|---|")
    columns, seconds = {}, {}
    with tempfile.TemporaryDirectory() as folder:
        for select in ("best", "consensus"):
            out = os.path.join(folder, select + ".csv")
            tick = time.perf_counter()
            sampled_components.main(["--model", "heisenberg_kagome_16", "--order", "2", "--number-samples", str(number),
                                     "--seed", str(seed), "--greedy-batch", "--output", out, "--anneal-select", select])
            seconds[select] = time.perf_counter() - tick
            rows = [line.split(",") for line in open(out).read().splitlines() if line and not line.startswith("#")]
            columns[select] = np.array([[float(v) for v in row] for row in rows if not row[0].startswith("size")])
    for order in range(3):
        cells = []
        for column in (3, 4):  # sa_accuracy, sa_overlap of this order
            for select in ("best", "consensus"):
                values = columns[select][:, 6 * order + column]
                cells.append("%.4f / %.4f" % (values.mean(), np.median(values)))
        emit("| %d | %s | %.1f / %.1f |" % (order, " | ".join(cells), seconds["best"], seconds["consensus"]))


def _median_ms(function, rounds):
    """(median wall ms, median kernel ms) of `function` after one warm-up call."""
    function()
    wall, device = [], []
    for _ in range(rounds):
        tick = time.perf_counter()
        function()
        wall.append((time.perf_counter() - tick) * 1e3)
        device.append(scores.vote_last_ms())
    return float(np.median(wall)), float(np.median(device))


def _host_ms(function, rounds):
    tick = time.perf_counter()
    function()
    first = (time.perf_counter() - tick) * 1e3
    if first > 500.0:  # (seconds a call: once is enough)
        return first
    times = []
    for _ in range(rounds):
        tick = time.perf_counter()
        function()
        times.append((time.perf_counter() - tick) * 1e3)
    return float(np.median(times))


def timing(emit, handles, rounds):
    rng = np.random.default_rng(11)
    emit("## timing: medians of %d calls after a warm-up, ms" % rounds)
    emit("| shape | device, every output: wall / kernels | device, consensus only: wall / kernels | "
         "device, weighted, 2 rounds: wall / kernels | numpy restatement on host configurations | numpy / device wall |")
    emit("|---|---|---|---|---|---|")
    for count in (64, 1024):
        for spins in (10**3, 10**5):
            # (random words: the time does not depend on the content)
            xs = rng.integers(0, 2**63, size=(count, (spins + 63) // 64), dtype=np.uint64) << np.uint64(1)
            weights = vote_cases.make_weights("lognormal", count, rng)
            full = _median_ms(lambda: scores.consensus(xs, spins), rounds)
            weighted = _median_ms(lambda: scores.consensus(xs, spins, weights, rounds=2), rounds)

            def only_x():
                vote = scores._as_vote((xs, spins))
                raw = (scores._lib.SignVoteItem * 1)()
                vote.fill(raw[0])
                raw[0].out_ones = raw[0].out_plus = raw[0].out_minus = None
                scores._lib.check(scores._lib.load().asp_sign_vote_batch(raw, 1))

            lean = _median_ms(only_x, rounds)
            host = _host_ms(lambda: vote_cases.vote_law(spins, xs), rounds)
            emit("| R = %d, K = %d | %.3f / %.3f | %.3f / %.3f | %.3f / %.3f | %.1f | %.0fx |"
                 % (count, spins, full[0], full[1], lean[0], lean[1], weighted[0], weighted[1], host, host / full[0]))
    # a round of resident handles
    sizes = np.exp(rng.uniform(np.log(50), np.log(1000), size=handles)).astype(int)
    hams, chains = [], []
    for k, size in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(int(size), seed=1000 + k)
        hams.append(sa.Hamiltonian(J, h))
        chains.append(sa.Chains(hams[-1], seed=k, repetitions=64))
    for c in chains:
        info = c.hamiltonian.info()
        c.advance(sa.make_schedule(info.beta0_auto, info.beta1_auto, 20), sweep_order="shuffled")
    batch = _median_ms(lambda: sa.consensus_chains(chains, anchor=0), rounds)
    loop = _median_ms(lambda: [c.consensus(anchor=0) for c in chains], rounds)
    export = _host_ms(lambda: [vote_cases.vote_law(c.hamiltonian.size, c.result()[0]) for c in chains], rounds)
    emit("")
    emit("| round of %d handles, 64 chains, %d spins in all (50 .. 1000 each), anchor 0, with the energy of every "
         "consensus | wall / kernels |" % (handles, int(sizes.sum())))
    emit("|---|---|")
    emit("| consensus_chains, one call | %.2f / %.3f |" % batch)
    emit("| loop of Chains.consensus | %.2f / %.3f (kernels: the last handle's) |" % loop)
    emit("| loop of Chains.result() + numpy restatement | %.1f |" % export)
    for c in chains:
        c.close()
    for h in hams:
        h.release()


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--sections", default="quality,clusters,timing")
    parser.add_argument("--models", default="heisenberg_kagome_16,sk_16_1")
    parser.add_argument("--sweeps", default="100,1600,25600")
    parser.add_argument("--trials", default="10,10,10", help="trials per sweep count")
    parser.add_argument("--chains", type=int, default=CHAINS, help="chains of an anneal of the quality section")
    parser.add_argument("--clusters", type=int, default=256)
    parser.add_argument("--handles", type=int, default=256)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--seed", type=int, default=2024)
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles", "consensus_quality.txt"))
    parser.add_argument("--append", action="store_true")
    args = parser.parse_args(argv)
    sweeps = [int(s) for s in args.sweeps.split(",")]
    trials = [int(t) for t in args.trials.split(",")]
    if len(trials) != len(sweeps):
        parser.error("--trials needs one count per entry of --sweeps")
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a" if args.append else "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit("# python tools/consensus_quality.py " + " ".join(sys.argv[1:] if argv is None else argv))
        for section in args.sections.split(","):
            if section == "quality":
                quality(emit, args.models.split(","), sweeps, trials, args.seed, args.chains)
            elif section == "clusters":
                clusters(emit, args.clusters, args.seed)
            elif section == "timing":
                timing(emit, args.handles, args.rounds)
            else:
                parser.error("unknown section '%s'" % section)
            emit("")


if __name__ == "__main__":
    main()
