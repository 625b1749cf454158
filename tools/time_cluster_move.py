"""Cost and effect of the isoenergetic cluster move (law ASP-ICM-1).

    python tools/time_cluster_move.py [--sizes 3000,100000] [--chains 64] [--repeat 9]
                                      [--effect-sizes 500,1000,3000] [--seeds 8] [--rounds 64]

(1) one move of --chains / 2 pairs (slot k with slot R - 1 - k) on a planted cluster, after a cold segment
    of 20 sweeps from random starts: device time (asp_sa_chains_cluster_move_last_ms) and wall time of
    Chains.cluster_move, with the bit planes where the library puts them and, for the largest size, forced
    into LDS and into HBM; beside it the route through the host — Chains.state(), the law in numpy / scipy
    (scipy.sparse.csgraph.connected_components on the induced graph), Chains.load_state() — wall time only
    (it has no single device span).  The two routes are compared bit for bit in every round.  Every timed
    call starts from the same snapshot (load_state, not timed); median and range over --repeat rounds after
    a warm-up.
(2) what the move buys: the best reported energy of parallel_tempering and of parallel_tempering_cluster
    at equal sweeps and equal repetitions on planted clusters, --seeds seeds each, beside the planted
    energy.  A record, not a claim.
Output goes to profiles/cluster_move_timing.txt by hand.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time_population as tp  # noqa: E402  (Philox restated in numpy)
from annealing_sign_problem_amd import _lib, build, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

STATE = tp.STATE


def unpack(x, K):
    return np.unpackbits(np.ascontiguousarray(x, dtype="<u8").view(np.uint8), bitorder="little")[:K].astype(bool)


def pack(up):
    padded = np.zeros((up.shape[0] + 63) // 64 * 64, dtype=np.uint8)
    padded[:up.shape[0]] = up
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def host_move(A, h, S, state, seed, pairs, draw):
    """ASP-ICM-1 on a state() dict with numpy and scipy.  The row sums are scipy's CSR product with the
    sites of d = 1 zeroed: sequential in ascending column, and a term of +-0.0 changes no sum."""
    K = A.shape[0]
    new = {name: np.array(state[name], copy=True) for name in STATE}
    new["sweeps_done"] = state["sweeps_done"]
    for a, b in pairs:
        up_a, up_b = unpack(state["x_current"][a], K), unpack(state["x_current"][b], K)
        d = up_a ^ up_b
        sites = np.flatnonzero(d)
        n = sites.shape[0]
        if n == 0:
            continue
        v = tp.philox_word0((int(a), int(state["sweeps_done"]), 0xFFFFFFFB, draw), (seed & 0xFFFFFFFF, seed >> 32))
        i0 = sites[(int(v) * n) >> 32]
        induced = A[sites][:, sites]
        _, label = scipy.sparse.csgraph.connected_components(induced, directed=False)
        inside = np.zeros(K, dtype=bool)
        inside[sites[label == label[np.searchsorted(sites, i0)]]] = True
        s = np.where(up_a, 1.0, -1.0)
        g = A[inside] @ np.where(d, 0.0, s) + h[inside]
        de = np.where(up_a[inside], -2.0, 2.0) * g
        Q = int(np.rint(de * 2.0 ** S).astype(np.int64).sum())
        new["x_current"][a], new["x_current"][b] = pack(up_a ^ inside), pack(up_b ^ inside)
        new["tracked_current"][a] += Q
        new["tracked_current"][b] -= Q
        for r in (a, b):
            if new["tracked_current"][r] < new["tracked_best"][r]:
                new["tracked_best"][r] = new["tracked_current"][r]
                new["x_best"][r] = new["x_current"][r]
    return new


def spread(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def same(a, b):
    return all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in STATE)


def time_moves(size, R, repeat, forms):
    lib = _lib.load()
    J, h, _ = synthetic.planted_cluster(size, seed=1000)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    m = scipy.sparse.csr_matrix(J)
    A = scipy.sparse.csr_matrix(m + m.T)
    A.setdiag(0.0)
    A.eliminate_zeros()
    A.sort_indices()
    pairs = [(k, R - 1 - k) for k in range(R // 2)]
    chains = sa.Chains(ham, seed=1, repetitions=R)
    chains.advance(np.full(20, info.beta1_auto))
    snapshot = chains.state()
    figures = {form: ([], []) for form in forms}
    host = []
    for k in range(repeat + 1):
        after = None
        for form in forms:
            _lib.check(lib.asp_sa_chains_set_cluster_planes(chains._live(), ctypes.c_int(form)))
            chains.load_state(snapshot)
            t0 = time.perf_counter()
            differing, sizes, _ = chains.cluster_move(pairs, 0)
            wall = (time.perf_counter() - t0) * 1e3
            device = float(lib.asp_sa_chains_cluster_move_last_ms())
            now = chains.state()
            if after is not None and not same(now, after):
                raise SystemExit("the plane forms do NOT agree")
            after = now
            if k:  # (the first round warms up)
                figures[form][0].append(wall)
                figures[form][1].append(device)
        chains.load_state(snapshot)
        t0 = time.perf_counter()
        state = chains.state()
        chains.load_state(host_move(A, h, info.energy_scale_exp, state, chains.seed, pairs, 0))
        wall = (time.perf_counter() - t0) * 1e3
        if not same(chains.state(), after):
            raise SystemExit("the host route and asp_sa_chains_cluster_move do NOT agree")
        if k:
            host.append(wall)
    print("(1) K=%d, %d chains, %d pairs: differing sites median %d (min %d, max %d), cluster median %d (min %d, max %d)"
          % (size, R, len(pairs), np.median(differing), differing.min(), differing.max(), np.median(sizes),
             sizes.min(), sizes.max()))
    names = {0: "planes automatic", 1: "planes in LDS", 2: "planes in HBM"}
    for form in forms:
        print("    asp_sa_chains_cluster_move, %-17s: wall %s  device %s" % (names[form], spread(figures[form][0]),
                                                                            spread(figures[form][1])))
    print("    export, numpy / scipy, import                 : wall %s  device NOT MEASURED (no single device span)"
          % spread(host), flush=True)
    chains.close()


def effect(size, seeds, rounds, R):
    J, h, planted = synthetic.planted_cluster(size, seed=2000 + size)
    ham = sa.Hamiltonian(J, h)
    planted_energy = ham.energy(sa.signs_to_bits(planted))
    plain, moved = [], []
    for seed in range(1, seeds + 1):
        plain.append(sa.parallel_tempering(ham, seed=seed, number_rounds=rounds, repetitions=R)[1])
        moved.append(sa.parallel_tempering_cluster(ham, seed=seed, number_rounds=rounds, repetitions=R)[1])
    print("(2) K=%d, %d rounds of 10 sweeps, %d chains, planted energy %.9f" % (size, rounds, R, planted_energy))
    print("    parallel_tempering        : best energy per seed " + " ".join("%.6f" % e for e in plain))
    print("    parallel_tempering_cluster: best energy per seed " + " ".join("%.6f" % e for e in moved))
    print("    lower with moves %d, equal %d, higher %d of %d seeds; at or below the planted energy: %d without, %d with"
          % (sum(m < p for m, p in zip(moved, plain)), sum(m == p for m, p in zip(moved, plain)),
             sum(m > p for m, p in zip(moved, plain)), seeds,
             sum(p <= planted_energy + 1e-9 * abs(planted_energy) for p in plain),
             sum(m <= planted_energy + 1e-9 * abs(planted_energy) for m in moved)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=str, default="3000,100000")
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--repeat", type=int, default=9)
    p.add_argument("--effect-sizes", type=str, default="500,1000,3000")
    p.add_argument("--seeds", type=int, default=8)
    p.add_argument("--rounds", type=int, default=64)
    a = p.parse_args()
    _lib.load()
    print("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
    sizes = [int(s) for s in a.sizes.split(",") if s]
    for size in sizes:
        time_moves(size, a.chains, a.repeat, (0, 1, 2) if size == max(sizes) else (0,))
    for size in [int(s) for s in a.effect_sizes.split(",") if s]:
        effect(size, a.seeds, a.rounds, a.chains)


if __name__ == "__main__":
    main()
