"""Cost of one population-annealing resample step (asp_sa_chains_resample_batch): a
batch of --batch handles of distinct planted clusters of --size spins with --chains chains, advanced
--sweeps sweeps so that the energies differ, then resampled once with dbeta = --gaps / (spread of the
handle's energies).

    python tools/time_population.py [--batch 64] [--size 3000] [--chains 64] [--sweeps 16] [--repeat 5]

(a) all handles in one resample_chains call: wall time, and the call's device time
    (asp_sa_chains_resample_last_ms: first energy launch to the end of the gather);
(b) the route the library offered before: per handle Chains.state() (export of five arrays), law
    ASP-PA-1 restated in numpy on Hamiltonian.energies of the exported configurations, and
    Chains.load_state() (import): wall time, and its three parts apart (numpy has no fma, so the
    restated expneg calls the C library's per element: that part is the host's arithmetic, not a
    transfer); it has no device time of its own to report.
Both start from the same snapshot every round (load_state, not timed) and are compared bit for bit
first; median and spread over --repeat rounds after a warm-up.  Output goes to
profiles/population_timing.txt by hand.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from annealing_sign_problem_amd import _lib, build, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")
_LOG2E, _LN2_HI, _LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42fee00000p-1"), \
    float.fromhex("0x1.a39ef35793c76p-33")
_TAYLOR = [float.fromhex(c) for c in (
    "0x1.6124613a86d09p-33", "0x1.1eed8eff8d898p-29", "0x1.ae64567f544e4p-26", "0x1.27e4fb7789f5cp-22",
    "0x1.71de3a556c734p-19", "0x1.a01a01a01a01ap-16", "0x1.a01a01a01a01ap-13", "0x1.6c16c16c16c17p-10",
    "0x1.1111111111111p-7", "0x1.5555555555555p-5", "0x1.5555555555555p-3", "0x1.0000000000000p-1", "1.0", "1.0")]


def _scalar_fma():
    import math

    if hasattr(math, "fma"):
        return math.fma
    import ctypes.util

    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    return libm.fma


_FMA = np.frompyfunc(_scalar_fma(), 3, 1)


def _fma(a, b, c):
    """fma(a, b, c) with one rounding, element-wise (numpy has none: the C library's, a call per element)."""
    return _FMA(a, b, c).astype(np.float64)


def expneg(x):
    """DESIGN.md §4.4's exp(-x) on a float64 array, operation for operation."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    live = x < 23.0
    y = -x[live]
    kf = np.rint(y * _LOG2E)
    r = _fma(kf, -_LN2_HI, y)
    r = _fma(kf, -_LN2_LO, r)
    p = np.full_like(r, _TAYLOR[0])
    for c in _TAYLOR[1:]:
        p = _fma(p, r, c)
    out[live] = p * np.ldexp(1.0, kf.astype(np.int64))
    return out


def philox_word0(counter, key):
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c[0]


def law_source(energies, dbeta, seed, sweeps_done, draw):
    """ASP-PA-1, steps 2-5, in numpy with Python integers where 64 bits would not do."""
    R = energies.shape[0]
    q = (expneg(dbeta * (energies - energies.min())) * 2.0 ** 31).astype(np.uint64)
    prefix = np.cumsum(q.astype(object))  # C_{s+1}
    T = int(prefix[-1])
    U = (philox_word0((sweeps_done, draw, 0xFFFFFFFD, 0), (seed & 0xFFFFFFFF, seed >> 32)) * T) >> 32
    keys = [j * T + U for j in range(R)]
    bounds = [R * int(c) for c in prefix]
    return np.searchsorted(np.array(bounds, dtype=object), np.array(keys, dtype=object), side="right").astype(np.uint32)


def host_route(chains, ham, dbeta, draw, parts):
    """parts += seconds of (export and energies, the law in numpy, import)."""
    t0 = time.perf_counter()
    state = chains.state()
    energies = ham.energies(state["x_current"])
    t1 = time.perf_counter()
    source = law_source(energies, dbeta, chains.seed, int(state["sweeps_done"]), draw).astype(np.int64)
    moved = {name: np.ascontiguousarray(state[name][source]) for name in STATE}
    moved["sweeps_done"] = state["sweeps_done"]
    t2 = time.perf_counter()
    chains.load_state(moved)
    t3 = time.perf_counter()
    parts += np.array([t1 - t0, t2 - t1, t3 - t2])


def spread(values):
    return "%9.3f ms (min %.3f, max %.3f)" % (statistics.median(values), min(values), max(values))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=3000)
    p.add_argument("--chains", type=int, default=64)
    p.add_argument("--sweeps", type=int, default=16)
    p.add_argument("--gaps", type=float, default=4.0, help="dbeta times the spread of a handle's energies")
    p.add_argument("--repeat", type=int, default=5)
    a = p.parse_args()
    lib = _lib.load()
    print("library %s fingerprint %s" % (os.path.basename(_lib.library_path()), build.built_fingerprint()))
    print("batch of %d clusters, K=%d chains=%d, %d sweeps before the step, dbeta = %g / spread, repeat=%d" % (
        a.batch, a.size, a.chains, a.sweeps, a.gaps, a.repeat), flush=True)
    hams = [sa.Hamiltonian(*synthetic.planted_cluster(a.size, seed=1000 + k)[:2]) for k in range(a.batch)]
    handles = [sa.Chains(h, seed=1, repetitions=a.chains) for h in hams]
    ladders = [sa.make_schedule(h.info().beta0_auto, h.info().beta1_auto, 5120)[:a.sweeps] for h in hams]
    sa.advance_chains(handles, ladders, sweep_order="shuffled")
    snapshots = [c.state() for c in handles]
    dbetas = []
    for h, snap in zip(hams, snapshots):
        e = h.energies(snap["x_current"])
        dbetas.append(a.gaps / float(e.max() - e.min()))
    walls_a, devices_a, walls_b, parts_b = [], [], [], []
    for k in range(a.repeat + 1):
        t0 = time.perf_counter()
        told = sa.resample_chains(handles, dbetas, 0)
        wall_a = (time.perf_counter() - t0) * 1e3
        device_a = float(lib.asp_sa_chains_resample_last_ms())
        after_a = [c.state() for c in handles]
        for c, snap in zip(handles, snapshots):
            c.load_state(snap)
        parts = np.zeros(3)
        t0 = time.perf_counter()
        for c, h, dbeta in zip(handles, hams, dbetas):
            host_route(c, h, dbeta, 0, parts)
        wall_b = (time.perf_counter() - t0) * 1e3
        for c, snap, mine in zip(handles, snapshots, after_a):
            now = c.state()
            if any(now[name].tobytes() != mine[name].tobytes() for name in STATE):
                raise SystemExit("the host route and the batched call do NOT agree")
            c.load_state(snap)
        if k:  # (the first round warms up)
            walls_a.append(wall_a)
            devices_a.append(device_a)
            walls_b.append(wall_b)
            parts_b.append(parts * 1e3)
    survivors = [s for _, _, s in told]
    print("survivors per handle: min %d, median %d, max %d of %d" % (min(survivors), statistics.median(survivors),
                                                                     max(survivors), a.chains))
    print("(a) one resample_chains call        : wall %s  device %s" % (spread(walls_a), spread(devices_a)))
    print("(b) export, numpy, import per handle: wall %s  device NOT MEASURED (no single device span)" % spread(walls_b))
    for name, column in zip(("export and asp_sa_energy", "the law in numpy (fma: a C call per element)", "import"),
                            np.array(parts_b).T):
        print("    of which %-45s: wall %s" % (name, spread(list(column))))
    for c in handles:
        c.close()


if __name__ == "__main__":
    main()
