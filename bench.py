"""Headline benchmark: simulated-annealing spin-flips/s on kagome_36-sized clusters.

    python bench.py --gpus N --steps K --warmup W

One STEP = one pass of the hot path over one batch of synthetic input: for each of
the three kagome_36-sized planted clusters of SURVEY §8d C3 (K = 1e4, 3e4, 1e5;
mean row degree 24 incl. diagonal) run `--replicas` (default 1024) independent
annealing chains per GPU for `--sweeps` (default 128) sweeps over the full
automatic beta ladder, return per-chain best configurations and energies, and
(N > 1) gather energies and each rank's best configuration over RCCL.  The plans
(couplings in sliced-ELL form) are resident in HBM before the timed region.

Weak scaling: every rank runs its own 1024 chains (global replica ids
rank*1024 ...); value = all ranks' flip attempts / max-over-ranks wall time.
`ms_per_step` is the wall time of one timed step.

    --dump-outputs DIR  after the timed steps, write what the last step returned (rank 0's
                        chains) as DIR/<name>.npy: see dump_outputs().
    --full              also run the secondary measurements below (minutes); a plain run sets up,
                        warms up, times the steps and prints the line.

The JSON line also carries
  roofline      for the sweep kernel, against the resource that binds it — VALU
                issue: (VALU instructions per flip from the committed PMC summary, per
                cluster size) x (SIMD cycles per instruction from the on-chip probe) x
                (flips/s from HIP events on the launch stream, live) over 1024 SIMDs x
                2.4 GHz; beside it the measured HBM fraction, the useful-f64-FMA
                fraction, the algorithmic bytes/s (B_flip = 12*dbar + 16) and
                the rate with every proposal evaluated (field cache / inert skipping
                off).  Every case of the PMC summary carries the fingerprint of the sources
                its kernel is built from (kernel file, plan builder, headers, flags) as
                measured: a case whose sources have changed since is dropped — its `frac`
                is null and `frac_null_reason` / `stale_counter_cases` say so.  The rate
                with every proposal evaluated takes runs of its own: --full only;

and, with --full (N = 1):
  shuffled_order  the same clusters, chains and sweeps with the reference annealer's
                visiting order (a fresh random permutation every sweep,
                asp_sa_anneal_shuffled), and the reference's default call (64 chains x
                5120 sweeps);
  cpu_baseline  the oracle's OpenMP port of the same sweep on the host cores,
                timed on a bounded sample (rank 0, N = 1 only);
  build         the coupling build (build_matrix) on the K = 1e5 cluster, device
                resident, next to the reference's own C timed on a sample;
  reference_default_call  the reference's default solve (5120 sweeps x 64 chains)
                on one 1e5-spin cluster, team sweep vs one workgroup per chain;
  batched_small_clusters  the production shape: 128 clusters of 1e2..1e4 spins, 64
                chains x 5120 sweeps each, one batched call vs the per-cluster loop.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
NUM_SIMDS = 1024        # 256 CUs x 4
CLOCK_GHZ = 2.4         # peak engine clock: the VALU-issue peak is NUM_SIMDS * CLOCK_GHZ cycles/s
F64_VALU_PEAK_TFLOPS = 78.6  # vector f64 (MI355X_MICROARCH.md: half the 157.3 TF f32 vector peak)
CLUSTER_SIZES = (10000, 30000, 100000)
CLUSTER_SEED = 783494  # experiments/sampled_connected_components.py:621
DUMP_CHAINS = 64              # chains per cluster whose configurations --dump-outputs writes
DUMP_SPIN_BYTES = 48 << 20    # cap on those configurations (float32), all clusters together


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5, help="timed steps")
    p.add_argument("--warmup", type=int, default=1, help="untimed steps before them")
    p.add_argument("--full", action="store_true",
                   help="also the secondary measurements (CPU baseline, coupling build, other workloads, "
                        "shuffled order, rate without skipping): minutes")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's results as DIR/<name>.npy")
    p.add_argument("--replicas", type=int, default=1024, help="chains per GPU")
    p.add_argument("--sweeps", type=int, default=128, help="sweeps per step")
    p.add_argument("--sizes", type=str, default=",".join(str(k) for k in CLUSTER_SIZES))
    p.add_argument("--group", type=int, default=0, help="replicas per workgroup (0 = auto)")
    p.add_argument("--threads", type=int, default=0, help="threads per workgroup (0 = auto)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="(--full) leave out the CPU baseline")
    p.add_argument("--no-build", action="store_true",
                   help="(--full) leave out the build, default-call, batched, large- and real-cluster legs "
                        "and the rate without skipping")
    p.add_argument("--cpu-seconds", type=float, default=12.0)
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if args.warmup < 0:
        p.error("--warmup must not be negative")
    return args


def dump_outputs(directory, clusters, replicas):
    """--dump-outputs: what the last timed step returned to its caller, per cluster of K spins
    (rank 0's chains):

      energies_K<K>.npy  float64 [replicas]: every chain's best energy;
      spins_K<K>.npy     float32 [64, K]: the best configurations (bit values 0 / 1, bit j of word
                         j // 64) of a fixed, seeded sample of 64 chains — beyond 48 MB over all
                         clusters, of a fixed, seeded sample of the spins as well.

    The inputs are fixed by the arguments (CLUSTER_SEED, seed 12345), so two builds can be
    compared file by file."""
    os.makedirs(directory, exist_ok=True)
    total_spins = sum(c["J"].shape[0] for c in clusters)
    chains_kept = min(replicas, DUMP_CHAINS)
    for c in clusters:
        k = c["J"].shape[0]
        xs, es = c["last"]
        xs = np.asarray(xs).view(np.uint64)
        rng = np.random.default_rng([CLUSTER_SEED, k])
        chains = np.sort(rng.choice(replicas, chains_kept, replace=False))
        words = np.ascontiguousarray(xs[chains])
        bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :k]
        spins_kept = int(DUMP_SPIN_BYTES * k / total_spins) // (4 * chains_kept)
        if spins_kept < k:
            bits = bits[:, np.sort(rng.choice(k, max(1, spins_kept), replace=False))]
        np.save(os.path.join(directory, "energies_K%d.npy" % k), np.asarray(es, dtype=np.float64))
        np.save(os.path.join(directory, "spins_K%d.npy" % k), bits.astype(np.float32))


def _load_profile(name):
    path = os.path.join(ROOT, "profiles", name)
    try:
        with open(path) as f:
            return json.load(f)
    except Exception:
        return None


def case_source_set(case):
    """The kernel-source set (build.KERNEL_SOURCE_SETS) a profiled case depends on."""
    return "shuffled" if "shuffled" in case else "colour"


def profiled_counters(built_sets):
    """``(counters, traffic, reason)``: the committed rocprofv3 summaries
    (profiles/sweep_counters.json, profiles/traffic.json; tools/gpu_profile_r4.sh) — but only the
    cases that were taken from THIS code.  Every case carries the fingerprint of the sources its
    kernel is built from (build.KERNEL_SOURCE_SETS: the kernel's file, the plan builder, their
    headers and the compiler flags) as it was when the case was measured; ``built_sets`` are the
    fingerprints recorded when the running library was built.  A case whose fingerprint differs
    says nothing about this binary and is dropped — its ``frac`` in the bench line is null instead
    of a number carried over from another kernel — and ``reason`` names what was dropped."""
    counters, traffic = _load_profile("sweep_counters.json"), _load_profile("traffic.json")
    if counters is None:
        return None, None, "profiles/sweep_counters.json missing or unreadable"
    if not built_sets:
        return None, None, "the running library has no build stamp to compare the counters with"

    def current(doc):
        kept, dropped = {}, []
        for case, entry in doc.get("cases", {}).items():
            name = entry.get("kernel_source_set") or case_source_set(case)
            have = entry.get("source_set_fingerprint")
            if have and have == built_sets.get(name):
                kept[case] = entry
            else:
                dropped.append(case)
        return kept, dropped

    kept, dropped = current(counters)
    reason = None
    if dropped:
        reason = ("stale counters dropped (their kernel's sources changed since they were measured; re-run "
                  "tools/gpu_profile_r4.sh for them): " + ", ".join(sorted(dropped)))
    if not kept:
        return None, None, reason
    counters = dict(counters, cases=kept)
    if traffic is not None:
        traffic = dict(traffic, cases=current(traffic)[0])
    return counters, traffic, reason


def issue_fraction(case, counters, flips_per_s):
    """VALU-issue fraction of one profiled case at a rate measured live: (VALU instructions per
    flip, PMC) x (SIMD cycles per instruction, on-chip probe) x flips/s over 1024 SIMDs x 2.4 GHz."""
    if not counters or case not in counters.get("cases", {}):
        return None
    per_flip = counters["cases"][case].get("valu_insts_per_flip")
    if per_flip is None or not flips_per_s:
        return None
    return per_flip * counters["cycles_per_valu_inst"] * flips_per_s / 1e9 / (NUM_SIMDS * CLOCK_GHZ)


def lane_utilisation(case, counters):
    """Of one profiled case: lanes with exec = 1 per VALU instruction (SQ_THREAD_CYCLES_VALU over
    SQ_ACTIVE_INST_VALU x 64, its own rocprofv3 pass) — what the hardware counters can see; the
    padding lanes and padding couplings of a block execute like real ones and are reported as
    `lane_fill` / `row_fill` by the library (shuffled sweep) or follow from the plan (colour sweep)."""
    if not counters or case not in counters.get("cases", {}):
        return None
    return counters["cases"][case].get("exec_lane_utilisation")


def shuffled_fill(lib, plan):
    lane, row = ctypes.c_double(0.0), ctypes.c_double(0.0)
    spins, wgs = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib.asp_sa_last_shuffled_fill(plan, ctypes.byref(lane), ctypes.byref(row))
    lib.asp_sa_last_shuffled_blocks(plan, ctypes.byref(spins), ctypes.byref(wgs))
    return {"spins_per_block": int(spins.value), "workgroups": int(wgs.value), "lane_fill": lane.value,
            "row_fill": row.value}


def usable_cores() -> int:
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            cores = max(1, min(cores, int(float(quota) / float(period))))
    except Exception:
        pass
    return cores


def cpu_baseline(J, field, cores, seconds):
    """Oracle sweep (OpenMP over chains) on the host: flips/s on a bounded sample."""
    import oracle
    from annealing_sign_problem_amd import annealer as sa, _lib

    info = _lib.SaInfo()
    m = J.tocsr()
    indptr = m.indptr.astype(np.int64)
    indices = m.indices.astype(np.int32)
    _lib.check(_lib.load().asp_sa_layout_host(
        m.shape[0], _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(m.data), _lib.ptr(field),
        ctypes.byref(info), None, None))
    k = m.shape[0]

    def run(reps, sweeps):
        betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, sweeps)
        t0 = time.perf_counter()
        oracle.sa_anneal(m, field, 12345, betas, reps, 0, None, info.energy_scale_exp,
                         num_threads=cores)
        return time.perf_counter() - t0

    reps = cores
    t_probe = run(reps, 4)
    rate = reps * 4 * k / max(t_probe, 1e-6)
    sweeps = int(max(8, min(4096, seconds * rate / (reps * k))))
    t = run(reps, sweeps)
    return {
        "value": reps * sweeps * k / t,
        "unit": "spin-flips/s",
        "cores": cores,
        "kind": "port",
        "sample": "oracle/sa_oracle.c (OpenMP over chains), K=%d cluster, %d chains x %d sweeps, %.1f s"
                  % (k, reps, sweeps, t),
    }


def bench_build(J, cores_unused, seconds=6.0):
    """Coupling build on the largest cluster: device-resident HIP vs the reference C."""
    import oracle
    from annealing_sign_problem_amd import _build_matrix, _lib, synthetic

    lib = _lib.load()
    keys, counts, psi, other, coeffs, other_counts, other_psi = synthetic.build_inputs_from_matrix(J)
    spins = _build_matrix.as_bits512(keys)
    others = _build_matrix.as_bits512(other)
    n, m = spins.shape[0], others.shape[0]
    handle = ctypes.c_void_p(lib.asp_build_create(n, m))
    if not handle:
        raise RuntimeError(_lib.last_error())
    _lib.check(lib.asp_build_upload(handle, _lib.ptr(spins), _lib.ptr(counts), _lib.ptr(psi),
                                    _lib.ptr(others), _lib.ptr(coeffs), _lib.ptr(other_counts),
                                    _lib.ptr(other_psi)))
    nnz = ctypes.c_uint64(0)
    times = []
    for _ in range(6):
        _lib.check(lib.asp_build_run(handle, ctypes.byref(nnz)))
        times.append(lib.asp_build_last_ms(handle))
    lib.asp_build_destroy(handle)
    ms = float(np.median(times[1:]))
    # the drop-in symbol itself, called through the C ABI with host pointers in and out (pinned
    # staging + key compaction by a team of host threads, PCIe both ways, kernels)
    row = np.empty(max(m, 1), np.uint32)
    col = np.empty(max(m, 1), np.uint32)
    el = np.empty(max(m, 1), np.float64)
    fld = np.empty(max(n, 1), np.float64)
    call_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        _build_matrix.lib.build_matrix(n, spins, counts, psi, others, coeffs, other_counts, other_psi,
                                       row, col, el, fld)
        call_ms.append((time.perf_counter() - t0) * 1e3)
    host_call_ms = float(np.median(call_ms[1:]))
    # reference C (serial: cbits/build_matrix.c has no OpenMP) on a prefix of the rows; the
    # key table must stay whole, so the remaining rows get other_counts = 0
    rows = max(1, min(n, int(n * 0.2)))
    cut = int(other_counts[:rows].sum())
    ref = oracle.ref_lib()
    cpu = None
    if ref is not None:
        row = np.zeros(max(cut, 1), np.uint32)
        col = np.zeros(max(cut, 1), np.uint32)
        el = np.zeros(max(cut, 1), np.float64)
        fld = np.zeros(n, np.float64)
        oc = other_counts.copy()
        oc[rows:] = 0
        t0 = time.perf_counter()
        ref.build_matrix(ctypes.c_uint64(n), _lib.ptr(spins), _lib.ptr(counts), _lib.ptr(psi),
                         _lib.ptr(others), _lib.ptr(coeffs), _lib.ptr(oc), _lib.ptr(other_psi),
                         _lib.ptr(row), _lib.ptr(col), _lib.ptr(el), _lib.ptr(fld))
        t = time.perf_counter() - t0
        cpu = {"value": cut / t, "unit": "connections/s", "cores": 1, "kind": "reference",
               "sample": "oracle/_ref (cbits/build_matrix.c, serial), first %d of %d rows, %.2f s"
                         % (rows, n, t)}
    # live path (common.make_ising_model's two numba kernels, 64-bit keys): device time of
    # scan + fused kernel, next to a numpy restatement of common.py:71-82,116-128 on one core
    from annealing_sign_problem_amd import common

    common.ising_elements(keys, psi, other, coeffs, other_counts)
    live_ms = []
    for _ in range(5):
        common.ising_elements(keys, psi, other, coeffs, other_counts)
        live_ms.append(lib.asp_ising_elements_last_ms())
    live = float(np.median(live_ms))
    t0 = time.perf_counter()
    idx = np.clip(np.searchsorted(keys, other), 0, n - 1)
    member = other == keys[idx]
    el = coeffs * np.abs(np.where(member, psi[idx], 0))
    el *= np.abs(psi[np.repeat(np.arange(n), other_counts)])
    t_np = time.perf_counter() - t0
    live_path = {
        "workload": "ising_elements K=%d, %d connections (64-bit keys)" % (n, m),
        "connections_per_s": m / (live * 1e-3), "ms": live,
        "algorithmic_GBps": m * 40 / (live * 1e-3) / 1e9,
        "cpu_baseline": {"value": m / t_np, "unit": "connections/s", "cores": 1, "kind": "port",
                         "sample": "numpy restatement of common.py:71-82,116-128, all %d connections, %.2f s" % (m, t_np)},
    }
    # action fused with the build (asp_operator_ising): 36-site kagome, 72 bonds, a 1e5-state
    # cluster; connections = what batched_apply would have materialised; CPU side = the numpy
    # operator + numpy/scipy restatement of the reference route on one core
    from annealing_sign_problem_amd import operators

    op = operators.Operator.from_config(synthetic.kagome_lattice())
    cluster = synthetic.grow_cluster(op, int("01" * 18, 2), 100000, seed=1)
    amp = np.ascontiguousarray(np.exp(synthetic.hashed_log_amplitudes(cluster)).real)
    amp /= np.linalg.norm(amp)
    dev = op.device()
    fused_ms, call_ms = [], []
    for _ in range(6):
        t0 = time.perf_counter()
        r_, c_, v_ = dev.ising(cluster, amp)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        fused_ms.append(dev.last_ms)
    fused = float(np.median(fused_ms[1:]))
    t0 = time.perf_counter()
    o_, co_, cn_ = op.batched_apply(cluster)
    o_ = o_[:, 0]
    ix_ = np.clip(np.searchsorted(cluster, o_), 0, cluster.size - 1)
    el_ = co_.real * np.abs(np.where(o_ == cluster[ix_], amp[ix_], 0))
    el_ *= np.abs(amp[np.repeat(np.arange(cluster.size), cn_)])
    import scipy.sparse
    m_ = scipy.sparse.csr_matrix((el_, ix_, np.concatenate([[0], np.cumsum(cn_)])),
                                 shape=(cluster.size,) * 2)
    m_ = 0.5 * (m_ + m_.T)
    m_.sort_indices()
    m_ = m_.tocoo()
    t_host = time.perf_counter() - t0
    if not (np.array_equal(m_.row, r_) and np.array_equal(m_.col, c_)
            and m_.data.tobytes() == v_.tobytes()):
        raise RuntimeError("fused coupling build disagrees with the reference route")
    conn = int(cn_.sum())
    fused_path = {
        "workload": "asp_operator_ising, kagome 36 sites / 72 bonds, K=%d, %d connections, nnz %d"
                    % (cluster.size, conn, v_.size),
        "connections_per_s": conn / (fused * 1e-3), "ms": fused,
        "host_pointer_call_ms": float(np.median(call_ms[1:])),
        "algorithmic_GBps": (cluster.size * 16 + v_.size * 16) / (fused * 1e-3) / 1e9,
        "cpu_baseline": {"value": conn / t_host, "unit": "connections/s", "cores": 1,
                         "kind": "port",
                         "sample": "numpy operator + numpy/scipy restatement of common.py:85-196, "
                                   "same cluster, %.2f s; outputs compared bit for bit" % t_host},
    }
    return {
        "fused_operator_path": fused_path,
        "live_path": live_path,
        "workload": "build_matrix K=%d, %d connections (512-bit keys)" % (n, m),
        "connections_per_s": m / (ms * 1e-3),
        "ms": ms,
        "host_pointer_call_ms": host_call_ms,
        "nnz": int(nnz.value),
        "algorithmic_GBps": m * 96 / (ms * 1e-3) / 1e9,
        "cpu_baseline": cpu,
    }


def bench_default_call():
    """The reference's default solve (common.py:236-239: 5120 sweeps, 64 repetitions) on one
    kagome_36-sized cluster: 64 chains cannot fill 256 CUs one workgroup each, so the launcher
    spreads every chain over a team of workgroups; timed next to the
    one-workgroup-per-chain kernel, same energies required."""
    from annealing_sign_problem_amd import _lib, synthetic
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    J, h, _ = synthetic.planted_cluster(100000, seed=1, mean_degree=8.0)
    ham = sa.Hamiltonian(J, h)
    sa.anneal(ham, seed=1, number_sweeps=16, repetitions=64, sweep_order="colour")  # warm-up
    out = {"workload": "anneal(number_sweeps=5120, repetitions=64), K=100000, dbar=8"}
    energies = []
    for name, team in (("team", -1), ("one_workgroup_per_chain", 0)):
        _lib.check(lib.asp_sa_set_team(ham.plan(), team))
        t0 = time.perf_counter()
        x, e = sa.anneal(ham, seed=12345, number_sweeps=5120, repetitions=64, sweep_order="colour")
        out[name + "_s"] = time.perf_counter() - t0
        out[name + "_flips_per_s"] = 100000 * 64 * 5120 / (lib.asp_sa_last_sweep_ms(ham.plan()) * 1e-3)
        energies.append(e)
    if energies[0] != energies[1]:
        raise RuntimeError("team sweep and single-workgroup sweep disagree")
    return out


def bench_large_cluster(replicas, sweeps, k=200000):
    """A cluster beyond the capacity of a byte per spin in LDS (~1.4e5 spins): four bits per spin,
    four chains per workgroup (layout 6), against a bit per spin and one chain per workgroup, the
    only choice before round 3.  The sampled-cluster pipeline's largest order-2 models."""
    from annealing_sign_problem_amd import _lib, synthetic
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    J, h, _ = synthetic.planted_cluster(k, seed=CLUSTER_SEED)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, sweeps)
    out = {"workload": "K=%d, dbar=%.1f, %d chains x %d sweeps" % (k, J.nnz / k, replicas, sweeps)}
    energies = []
    for name, packed in (("nibbles", 0), ("bits", 1)):
        _lib.check(lib.asp_sa_set_packed(ham.plan(), packed))
        sa.anneal_raw(ham, 1, betas[:4], replicas)  # warm-up
        _, es = sa.anneal_raw(ham, 12345, betas, replicas)
        out[name + "_layout"] = int(lib.asp_sa_last_layout(ham.plan()))
        out[name + "_kernel_flips_per_s"] = k * replicas * sweeps / (lib.asp_sa_last_sweep_ms(ham.plan()) * 1e-3)
        energies.append(es)
    if energies[0].tobytes() != energies[1].tobytes():
        raise RuntimeError("the 4-bit and the 1-bit layout disagree")
    return out


def bench_batched_clusters(num_problems=128, serial_every=8):
    """The reference's production shape (experiments/sampled_connected_components.py:764-767,
    common.py:236-239): many sampled clusters, each solved with 64 chains x 5120 sweeps.  A
    log-uniform mix of cluster sizes in [1e2, 1e4]; one asp_sa_anneal_batch call for all of them
    next to the per-cluster loop (timed on every `serial_every`-th problem), identical results
    required."""
    from annealing_sign_problem_amd import _lib, synthetic
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    rng = np.random.default_rng(CLUSTER_SEED)
    sizes = [int(round(np.exp(rng.uniform(np.log(1e2), np.log(1e4))))) for _ in range(num_problems)]
    hams = []
    for i, k in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(k, seed=CLUSTER_SEED + i)
        ham = sa.Hamiltonian(J, h)
        ham.info()  # plan resident before the timed region
        hams.append(ham)
    sweeps, reps = 5120, 64
    sa.anneal_batch(hams[:4], seed=1, number_sweeps=8, repetitions=reps, sweep_order="colour")  # warm-up
    t0 = time.perf_counter()
    batched = sa.anneal_batch(hams, seed=12345, number_sweeps=sweeps, repetitions=reps, sweep_order="colour")
    t_batched = time.perf_counter() - t0
    batched_kernel_ms = float(lib.asp_sa_batch_last_ms())
    subset = list(range(0, num_problems, serial_every))
    sa.anneal(hams[subset[0]], seed=1, number_sweeps=8, repetitions=reps, sweep_order="colour")  # warm-up
    t0 = time.perf_counter()
    serial = [sa.anneal(hams[i], seed=12345, number_sweeps=sweeps, repetitions=reps, sweep_order="colour")
              for i in subset]
    t_serial = time.perf_counter() - t0
    for i, (x, e) in zip(subset, serial):
        if not (np.array_equal(x, batched[i][0]) and e == batched[i][1]):
            raise RuntimeError("batched anneal disagrees with the per-cluster call")
    flips_all = float(sum(sizes)) * reps * sweeps
    flips_subset = float(sum(sizes[i] for i in subset)) * reps * sweeps
    # the same batch with the reference annealer's visiting order (ASP_SA_BATCH_SHUFFLED: the
    # problems share one order launch and one sweep launch per wavefront class and chunk)
    sa.anneal_batch(hams[:4], seed=1, number_sweeps=8, repetitions=reps, sweep_order="shuffled")  # warm-up
    t0 = time.perf_counter()
    shuffled = sa.anneal_batch(hams, seed=12345, number_sweeps=sweeps, repetitions=reps, sweep_order="shuffled")
    t_shuffled = time.perf_counter() - t0
    shuffled_kernel_ms = float(lib.asp_sa_batch_last_ms())
    # how the batch was cut: spins per block (lane packing below 64) -> problems, workgroups, fill
    shapes = {}
    for ham, k in zip(hams, sizes):
        f = shuffled_fill(lib, ham.plan())
        e = shapes.setdefault(f["spins_per_block"], {"problems": 0, "workgroups": 0, "spins": 0, "slots": 0.0,
                                                      "coupling_slots": 0.0, "couplings": 0.0})
        e["problems"] += 1
        e["workgroups"] += f["workgroups"]
        e["spins"] += k
        e["slots"] += k / f["lane_fill"] if f["lane_fill"] else 0.0
    for e in shapes.values():
        e["lane_fill"] = e["spins"] / e["slots"] if e["slots"] else None
        for key in ("slots", "coupling_slots", "couplings"):
            e.pop(key)
    x, e = sa.anneal(hams[subset[1]], seed=12345, number_sweeps=sweeps, repetitions=reps, sweep_order="shuffled")
    if not (np.array_equal(x, shuffled[subset[1]][0]) and e == shuffled[subset[1]][1]):
        raise RuntimeError("batched shuffled anneal disagrees with the per-cluster call")
    for ham in hams:
        ham.release()
    return {
        "workload": "%d planted clusters, K log-uniform in [1e2, 1e4] (sum K = %d), %d chains x %d "
                    "sweeps each" % (num_problems, sum(sizes), reps, sweeps),
        "batched_s": t_batched,
        "batched_sweep_kernels_ms": batched_kernel_ms,
        "batched_kernel_flips_per_s": flips_all / (batched_kernel_ms * 1e-3),
        "batched_flips_per_s": flips_all / t_batched,
        "batched_problems_per_s": num_problems / t_batched,
        "serial_sample": "every %dth problem (%d problems)" % (serial_every, len(subset)),
        "serial_s": t_serial,
        "serial_flips_per_s": flips_subset / t_serial,
        "serial_problems_per_s": len(subset) / t_serial,
        "speedup": (flips_all / t_batched) / (flips_subset / t_serial),
        "shuffled_order_batched_s": t_shuffled,
        "shuffled_order_batched_flips_per_s": flips_all / t_shuffled,
        "shuffled_order_batched_problems_per_s": num_problems / t_shuffled,
        "shuffled_order_batched_kernels_ms": shuffled_kernel_ms,
        "shuffled_order_batched_kernel_flips_per_s": flips_all / (shuffled_kernel_ms * 1e-3),
        "shuffled_order_blocks": {str(k): v for k, v in sorted(shapes.items())},
    }


def bench_real_kagome_36(replicas, sweeps, targets=(10_000, 30_000, 100_000), seeds=24, calls=5,
                         warmup=2, pipeline=True):
    """The headline step on REAL clusters of the 36-site kagome model, not planted ones: the
    ground state of heisenberg_kagome_36.yaml's symmetry sector is computed here (31.5 M
    representatives; enumeration, resident Hamiltonian and Lanczos on this GPU, sector_ed.py —
    the reference downloads it as SpinED output, Makefile:143-153), clusters are sampled and
    extended twice exactly as `make kagome_36` does (sampled_power 0.1, 50-1000 seed states,
    cutoff 1e-6), and the three whose sizes are closest to the planted K are annealed with the
    same 1024 chains x 128 sweeps.  Rank 0, N = 1 only."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, operators, sampled_components, sector_ed, synthetic

    t0 = time.perf_counter()
    op = operators.Operator.from_config(synthetic.load_models()["heisenberg_kagome_36"])
    energy, psi, reps, info = sector_ed.ground_state(op)
    op.basis.build(reps)
    ed_s = time.perf_counter() - t0
    state = np.random.get_state()
    np.random.seed(435834)
    try:
        clusters = sampled_components.generate_clusters(op, psi, seeds, 0.1, 50, 1000, 0.5)
    finally:
        np.random.set_state(state)
    log_psi = common.ground_state_to_log_coeff_fn(psi, op.basis)
    models = []
    t0 = time.perf_counter()
    for cluster in clusters:
        h = common.make_ising_model(cluster, op, log_psi_fn=log_psi)
        for _ in range(2):
            h = common.make_hamiltonian_extension(h, log_psi)
            h = common.sparsify_using_global_cutoff(h, 1e-6, cluster)
        models.append(h)
    build_s = time.perf_counter() - t0
    chosen = []
    for target in targets:
        rest = [m for m in models if all(m is not c for c in chosen)]
        chosen.append(min(rest, key=lambda m: abs(np.log(m.size / target))))
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    flips, flips_profiled, seconds, kernel_ms, shapes = 0, 0, 0.0, 0.0, []
    for m in chosen:
        ham = m.ising_hamiltonian
        hinfo = ham.info()
        betas = sa.make_schedule(hinfo.beta0_auto, hinfo.beta1_auto, sweeps)
        for _ in range(warmup):
            sa.anneal_raw(ham, 12345, betas, replicas)  # warm-up (plan upload, clocks)
        timed = []
        for _ in range(calls):
            t0 = time.perf_counter()
            sa.anneal_raw(ham, 12345, betas, replicas)
            timed.append((time.perf_counter() - t0, lib.asp_sa_last_sweep_ms(ham.plan())))
        # medians: an occasional host-side stall (50 ms once in ten calls) is not the workload
        seconds += float(np.median([c[0] for c in timed]))
        kernel_ms += float(np.median([c[1] for c in timed]))
        flips += m.size * replicas * sweeps
        flips_profiled += m.size * replicas * sweeps * (warmup + calls)
        j = ham.exchange
        shapes.append({"K": int(m.size), "dbar": float(j.nnz / j.shape[0]),
                       "colors": int(hinfo.num_colors), "max_degree": int(hinfo.max_degree),
                       "call_ms": [round(c[0] * 1e3, 2) for c in timed],
                       "sweep_kernel_ms": [round(c[1], 2) for c in timed]})
    return {
        # (not under the profiler's counter passes: its descent sweeps are k_sa_sweep launches too)
        "pipeline": bench_pipeline(op, psi, log_psi) if pipeline else None,
        "workload": "real heisenberg_kagome_36 clusters (order-2 extension, cutoff 1e-6) closest to "
                    "K = %s, %d chains x %d sweeps per call (median of %d calls each)" % (
                        "/".join(str(t) for t in targets), replicas, sweeps, calls),
        "flips_per_s": flips / seconds,
        "flips_profiled": flips_profiled,
        "kernel_flips_per_s": flips / (kernel_ms * 1e-3),
        "clusters": shapes,
        "sector_dimension": int(info["dimension"]),
        "ground_state_energy": energy,
        "ground_state_energy_per_site_S_dot_S": energy / 36.0 / 4.0,
        "lanczos_steps": int(info["iterations"]),
        "eigen_residual": float(info["residual"]),
        "ground_state_s": ed_s,
        "cluster_build_s": build_s,
        "clusters_built": len(models),
        "sizes_built": sorted(int(m.size) for m in models),
    }


def bench_pipeline(op, psi, log_psi, greedy_clusters=128, annealed_clusters=32, threads=16):
    """`make kagome_36`'s per-cluster pipeline on the real model (the caller's operator and ground
    state): clusters of 50-1000 seed states, orders 0-2, cutoff 1e-6 — coupling build, extension,
    cutoff, plan, greedy solver and metrics per order — with host threads, then the same with every
    model annealed (64 chains x 5120 sweeps, the reference's defaults) in one batched call."""
    from concurrent.futures import ThreadPoolExecutor

    from annealing_sign_problem_amd import sampled_components

    os.environ.setdefault("ASP_HOST_THREADS", "1")  # (as sampled_components.main does with --jobs > 1)
    state = np.random.get_state()
    np.random.seed(435834)
    try:
        t0 = time.perf_counter()
        clusters = sampled_components.generate_clusters(op, psi, greedy_clusters, 0.1, 50, 1000, 0.5)
        growth_s = time.perf_counter() - t0
    finally:
        np.random.set_state(state)

    def work(cluster):
        return sampled_components.process_cluster(cluster, op, psi, psi, log_psi, 2, 1e-6, False)

    work(clusters[0])  # warm-up
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        results = list(pool.map(work, clusters))
    greedy_s = time.perf_counter() - t0
    some = clusters[:annealed_clusters]
    t0 = time.perf_counter()
    staged = sampled_components.stage_clusters(some, op, psi, psi, log_psi, 2, 1e-6, threads)
    staged_s = time.perf_counter() - t0
    spins = sum(m.size for _, m, _, _, _ in staged)
    t0 = time.perf_counter()
    annealed = sampled_components.anneal_staged(staged, some, True)
    anneal_s = time.perf_counter() - t0
    return {
        "workload": "%d real kagome_36 clusters x orders 0-2 (cutoff 1e-6), greedy, %d host threads; "
                    "%d of them with 64 chains x 5120 sweeps per model" % (greedy_clusters, threads, annealed_clusters),
        "growth_ms_per_cluster": growth_s / greedy_clusters * 1e3,
        "greedy_ms_per_cluster": greedy_s / greedy_clusters * 1e3,
        "greedy_clusters_per_s": greedy_clusters / greedy_s,
        "median_order2_greedy_accuracy": float(np.median([r[2].greedy_accuracy for r in results])),
        "annealed_models": len(staged),
        "annealed_spins": int(spins),
        "annealed_build_s": staged_s,
        "annealed_sweep_order": "shuffled (the drop-in default: sampled_components --annealing)",
        "annealed_anneal_s": anneal_s,
        "annealed_flips_per_s": spins * 64 * 5120 / anneal_s,
        "median_order2_sa_accuracy": float(np.median([r[2].sa_accuracy for r in annealed])),
    }


def bench_shuffled_order(clusters, replicas, sweeps, offset, counters):
    """The reference annealer's visiting order — a fresh random permutation every sweep,
    ASP-SA-1S — on the headline workload: the same three planted clusters, the
    same chains and sweeps per call, through asp_sa_anneal_shuffled (orders built on the device
    beside the sweeps, csrc/sa_shuffled.hip); and the reference's default call, 64 repetitions x
    5120 sweeps (common.py:236-239), on the smallest of them.  Rates of whole calls (host wall
    clock) and of the kernels alone (HIP events on the launch stream, order kernels included)."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    out = {"workload": "asp_sa_anneal_shuffled on the headline clusters, %d chains x %d sweeps per call "
                       "(median of 3 calls)" % (replicas, sweeps), "clusters": []}
    flips = seconds = kernel_s = 0.0
    for c in clusters:
        k = c["J"].shape[0]
        sa.anneal_raw(c["ham"], 12345, c["betas"], replicas, offset, shuffled=True)  # warm-up (row quads resident)
        timed = []
        for _ in range(3):
            t0 = time.perf_counter()
            sa.anneal_raw(c["ham"], 12345, c["betas"], replicas, offset, shuffled=True)
            timed.append((time.perf_counter() - t0, lib.asp_sa_last_sweep_ms(c["ham"].plan()) * 1e-3))
        call_s = float(np.median([t[0] for t in timed]))
        kern_s = float(np.median([t[1] for t in timed]))
        levels = ctypes.c_uint32(0)
        lib.asp_sa_last_shuffled(c["ham"].plan(), ctypes.byref(levels), None)
        m, th, g = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        lib.asp_sa_last_launch(c["ham"].plan(), ctypes.byref(m), ctypes.byref(th), ctypes.byref(g))
        rate = k * replicas * sweeps / kern_s
        out["clusters"].append({
            "K": k, "levels_per_sweep_max": int(levels.value), "chains_per_group": m.value,
            "wavefronts": th.value // 64, "groups": g.value, "call_ms": call_s * 1e3,
            "kernels_ms": kern_s * 1e3, "kernel_flips_per_s": rate,
            "valu_issue_frac": issue_fraction("shuffled_%d" % k, counters, rate),
            "exec_lane_utilisation": lane_utilisation("shuffled_%d" % k, counters),
            "blocks": shuffled_fill(lib, c["ham"].plan())})
        flips += k * replicas * sweeps
        seconds += call_s
        kernel_s += kern_s
    out["flips_per_s"] = flips / seconds
    out["kernel_flips_per_s"] = flips / kernel_s
    # the reference's default call on the K = 1e4 cluster
    c = clusters[0]
    k = c["J"].shape[0]
    betas = sa.make_schedule(c["info"].beta0_auto, c["info"].beta1_auto, 5120)
    t0 = time.perf_counter()
    sa.anneal_raw(c["ham"], 12345, betas, 64, 0, shuffled=True)
    t = time.perf_counter() - t0
    kern = lib.asp_sa_last_sweep_ms(c["ham"].plan()) * 1e-3
    out["reference_default_call"] = {
        "workload": "64 chains x 5120 sweeps, K=%d" % k, "call_s": t, "flips_per_s": k * 64 * 5120 / t,
        "kernel_flips_per_s": k * 64 * 5120 / kern,
        "valu_issue_frac": issue_fraction("shuffled64_%d" % k, counters, k * 64 * 5120 / kern),
        "exec_lane_utilisation": lane_utilisation("shuffled64_%d" % k, counters),
        "blocks": shuffled_fill(lib, c["ham"].plan())}
    return out


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d" % args.gpus)

    import torch
    import torch.distributed as dist

    # Rehearsal knobs for a 1-GPU box (never set by the driver): all ranks on device 0 and a
    # gloo process group, which exercises everything but RCCL itself.
    backend = os.environ.get("ASP_BENCH_BACKEND", "nccl")
    if os.environ.get("ASP_BENCH_SINGLE_DEVICE") == "1":
        local_rank = 0
    # ASP_BENCH_FORCE_DIST=1: run the multi-rank code path (process group, RCCL gather of each
    # rank's best chain, max-over-ranks timing) at world size 1 — the rehearsal of the N > 1
    # path a one-GPU box allows (tests/test_gpu_rccl.py)
    use_dist = world > 1 or os.environ.get("ASP_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend)

    from annealing_sign_problem_amd import _lib, synthetic
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import distributed as asp_dist

    lib = _lib.load()
    _lib.require_gpu()
    _lib.check(lib.asp_set_device(local_rank))

    sizes = [int(s) for s in args.sizes.split(",") if s]
    clusters = []
    for k in sizes:
        J, field, _ = synthetic.planted_cluster(k, seed=CLUSTER_SEED)
        ham = sa.Hamiltonian(J, field)
        info = ham.info()  # builds the plan: couplings now resident in HBM
        if args.group or args.threads:
            _lib.check(lib.asp_sa_set_launch(ham.plan(), args.group, args.threads))
        betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, args.sweeps)
        dbar = J.nnz / J.shape[0]
        clusters.append(dict(J=J, field=field, ham=ham, info=info, betas=betas, dbar=dbar,
                             b_flip=12.0 * dbar + 16.0))

    replicas = args.replicas
    offset = rank * replicas
    sweep_ms = []
    accepted = []

    on_device = use_dist and backend == "nccl"
    if on_device:
        # per cluster: the chains' results land in device tensors (D2D from the kernel's
        # buffers), the best chain is picked there and gathered over RCCL: no host round trip
        for c in clusters:
            words = (c["J"].shape[0] + 63) // 64
            c["xs_t"] = torch.zeros((replicas, words), dtype=torch.int64, device="cuda")
            c["es_t"] = torch.zeros(replicas, dtype=torch.float64, device="cuda")

    def step(record):
        for c in clusters:
            if on_device:
                sa.anneal_raw_into(c["ham"], 12345, c["betas"], replicas, offset, None,
                                   c["xs_t"].data_ptr(), c["es_t"].data_ptr())
                best = torch.argmin(c["es_t"])
                mine = torch.cat([c["xs_t"][best], c["es_t"][best].view(1).view(torch.int64)])
                parts = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(parts, mine)
                torch.stack(parts).cpu()  # every rank ends up with all ranks' best chains
                # and, as at N = 1, with all of its own chains on the host (same work per rank)
                xs = c["xs_t"].cpu().numpy()
                es = c["es_t"].cpu().numpy()
            else:
                xs, es = sa.anneal_raw(c["ham"], 12345, c["betas"], replicas, offset)
                if use_dist:
                    best = int(np.argmin(es))
                    words = xs.shape[1]
                    payload = np.concatenate([xs[best].view(np.int64).reshape(1, words),
                                              np.array([[es[best]]]).view(np.int64)], axis=1)
                    asp_dist.all_gather_rows(payload, [1] * world)
            c["last"] = (xs, es)  # (for --dump-outputs)
            if record:
                sweep_ms.append((c, lib.asp_sa_last_sweep_ms(c["ham"].plan())))

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(False)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    fence()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    flips_per_step = sum(c["J"].shape[0] for c in clusters) * replicas * args.sweeps
    value = world * flips_per_step * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, clusters, replicas)
    if rank == 0:
        launch = []
        for c in clusters:
            m, th, g = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
            lib.asp_sa_last_launch(c["ham"].plan(), ctypes.byref(m), ctypes.byref(th), ctypes.byref(g))
            launch.append({"K": c["J"].shape[0], "colors": int(c["info"].num_colors),
                           "replicas_per_group": m.value, "threads": th.value, "groups": g.value,
                           "ell_padding": float(c["info"].ell_entries) / max(1, c["info"].nnz_offdiag)})
        alg_bytes = sum(c["J"].shape[0] * replicas * args.sweeps * c["b_flip"] for c, _ in sweep_ms)
        kernel_s = sum(ms for _, ms in sweep_ms) * 1e-3
        launches = max(1, len(sweep_ms))
        kernel_flips = flips_per_step * args.steps / kernel_s
        from annealing_sign_problem_amd import build as asp_build

        counters, traffic, stale = profiled_counters(asp_build.built_source_set_fingerprints())
        # every proposal evaluated: field cache and inert-block skipping off (results identical).
        # --full only, and left out under --no-build, the form the rocprofv3 passes use, so that
        # their per-launch averages cover the timed workload only.
        kernel_flips_no_skip = None
        if args.full and not args.no_build:
            no_skip_ms = 0.0
            for c in clusters:
                _lib.check(lib.asp_sa_set_field_cache(c["ham"].plan(), 0))
                sa.anneal_raw(c["ham"], 12345, c["betas"], replicas, offset)
                no_skip_ms += lib.asp_sa_last_sweep_ms(c["ham"].plan())
                _lib.check(lib.asp_sa_set_field_cache(c["ham"].plan(), 1))
            kernel_flips_no_skip = flips_per_step / (no_skip_ms * 1e-3)
        # The sweep kernel is bound by VALU ISSUE, not by HBM (couplings are L2/MALL-resident
        # and shared by the replicas of a workgroup; spins never leave LDS): achieved = SIMD
        # issue cycles its VALU instructions occupy per second = (instructions per flip, PMC, per
        # cluster size) x (cycles per instruction, on-chip probe) x (flips/s, measured live here).
        peak_issue = NUM_SIMDS * CLOCK_GHZ  # G SIMD-cycles/s
        per_size, issue_cycles, hbm_bytes, have_all = [], 0.0, 0.0, counters is not None
        for c in clusters:
            k = c["J"].shape[0]
            ms = [t for cc, t in sweep_ms if cc is c]
            rate = k * replicas * args.sweeps * len(ms) / (sum(ms) * 1e-3)
            case = "colour_%d" % k
            entry = counters["cases"].get(case) if counters else None
            frac = issue_fraction(case, counters, rate)
            per_flip_bytes = (traffic or {}).get("cases", {}).get(case, {}).get("hbm_bytes_per_flip")
            per_size.append({"K": k, "kernel_flips_per_s": rate, "avg_launch_ms": sum(ms) / len(ms),
                             "valu_insts_per_flip": entry.get("valu_insts_per_flip") if entry else None,
                             "frac": frac,
                             "hbm_measured_frac": (per_flip_bytes * rate / 1e9 / HBM_PEAK_GBS
                                                   if per_flip_bytes else None)})
            if frac is None:
                have_all = False
            else:
                # cycles this size's launches occupied = frac x peak x their time
                issue_cycles += frac * peak_issue * sum(ms) * 1e-3
            if per_flip_bytes:
                hbm_bytes += per_flip_bytes * k * replicas * args.sweeps * len(ms)
            else:
                hbm_bytes = float("nan")
        issue = issue_cycles / kernel_s if have_all else None
        hits = [(traffic or {}).get("cases", {}).get("colour_%d" % c["J"].shape[0], {}).get("l2_hit_rate")
                for c in clusters]
        l2_hit = sum(hits) / len(hits) if hits and all(h is not None for h in hits) else None
        hbm_per_launch = hbm_bytes / launches if hbm_bytes == hbm_bytes and traffic else None
        mean_offdiag = sum((c["dbar"] - 1.0) * c["J"].shape[0] for c in clusters) / sum(
            c["J"].shape[0] for c in clusters)
        clock = None
        if counters:
            clocks = [counters["cases"].get("colour_%d" % c["J"].shape[0], {}).get("clock_ghz") for c in clusters]
            if all(clocks):
                clock = sum(clocks) / len(clocks)
        roofline = {
            "bound": "valu",
            "kernel": "k_sa_sweep",
            "achieved": issue,
            "peak": peak_issue,
            "unit": "G SIMD issue cycles/s",
            "frac": issue / peak_issue if issue is not None else None,
            "frac_null_reason": stale if issue is None else None,
            "stale_counter_cases": stale if issue is not None else None,
            "counters_source_fingerprints": ({case: entry.get("source_set_fingerprint")
                                             for case, entry in counters["cases"].items()} if counters else None),
            "running_source_fingerprints": asp_build.built_source_set_fingerprints(),
            "running_library_fingerprint": asp_build.built_fingerprint(),
            "traffic": hbm_per_launch,
            "per_cluster_size": per_size,
            "cycles_per_valu_inst": counters.get("cycles_per_valu_inst") if counters else None,
            "measured_clock_ghz": clock,
            "frac_at_measured_clock": (issue / (NUM_SIMDS * clock) if issue is not None and clock else None),
            "hbm_measured_frac": (hbm_per_launch / (kernel_s / launches) / 1e9 / HBM_PEAK_GBS
                                  if hbm_per_launch else None),
            # SURVEY §8(d)'s contract figures as a sub-object of their own: the HBM roofline by the
            # letter (algorithmic bytes of a one-replica CPU sweep over the kernel's time: above 1
            # because a row is shared by the chains of a workgroup and by the workgroups through
            # L2), what the counters say really crossed the HBM interface, and the L2 hit rate.
            "hbm": {
                "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "algorithmic_achieved": alg_bytes / kernel_s / 1e9,
                "algorithmic_frac": alg_bytes / kernel_s / 1e9 / HBM_PEAK_GBS,
                "measured_achieved": (hbm_per_launch / (kernel_s / launches) / 1e9 if hbm_per_launch else None),
                "measured_frac": (hbm_per_launch / (kernel_s / launches) / 1e9 / HBM_PEAK_GBS
                                  if hbm_per_launch else None),
                "l2_hit_rate": l2_hit,
            },
            # the same fraction with every proposal evaluated (field cache and inert-block skipping
            # off; identical chains): the instructions per flip of the profiled run are those of the
            # skipping kernel, so this is frac scaled by the rate ratio — a LOWER bound of the
            # no-skip kernel's issue occupancy (it executes more instructions per flip, not fewer)
            "frac_no_skip_lower_bound": (issue / peak_issue * kernel_flips_no_skip / kernel_flips
                                         if issue is not None and kernel_flips_no_skip else None),
            "lane_utilisation": {
                "exec_mask": {("colour_%d" % c["J"].shape[0]): lane_utilisation("colour_%d" % c["J"].shape[0], counters)
                              for c in clusters},
                "slots": {str(c["J"].shape[0]): c["J"].shape[0] / (64.0 * c["info"].num_blocks) for c in clusters},
                "rows": {str(c["J"].shape[0]): float(c["info"].nnz_offdiag) / max(1, c["info"].ell_entries)
                         for c in clusters},
                "note": "exec_mask: lanes with exec = 1 per VALU instruction (PMC, own pass); slots: spins per "
                        "64-lane block slot of the colour classes; rows: couplings per ELL slot (a block is as "
                        "wide as its longest row).  A padding lane or coupling executes like a real one.",
            },
            "cycles_per_valu_inst_by_class": {
                "source": "profiles/r02_issue_rate_probe.txt (4 wavefronts per SIMD)",
                "v_fma_f64 / v_add_f64": 4.36, "v_mul_f64": 4.92, "v_or_b32_sdwa (sign, word layout)": 4.41,
                "v_lshl_or_b32 / v_bfi_b32 (VOP3)": 4.39, "v_mul_hi_u32 / v_mul_lo_u32 (Philox)": 4.34,
                "v_lshlrev_b32": 4.23, "v_xor_b32 / v_add_u32 / v_lshrrev_b32 (plain VOP2)": 2.54,
                "v_exp_f32": 8.27,
                "note": "the guide's 2 cycles per wave64 VOP2 is what the probe finds for xor / add / right shift "
                        "(2.5); every f64, SDWA, VOP3, left-shift and 32x32-multiply instruction issues at "
                        "4.2-4.4.  Of the colour kernel's 1.58 instructions per flip the integer ones that are "
                        "or could be plain VOP2 are the Philox xors and key adds (already VOP2) and the byte "
                        "layout's sign shift (v_lshrrev since round 2); the word layout's sign is one SDWA "
                        "instruction (4.4) for a shift + VOP3 pair (2.5 + 4.4), the rest is f64",
            },
            "f64_fma_frac": kernel_flips * mean_offdiag * 2.0 / 1e12 / F64_VALU_PEAK_TFLOPS,
            "algorithmic_GBps": alg_bytes / kernel_s / 1e9,
            "algorithmic_bytes_per_launch": alg_bytes / launches,
            "avg_launch_ms": kernel_s * 1e3 / launches,
            "kernel_flips_per_s": kernel_flips,
            "kernel_flips_per_s_no_skip": kernel_flips_no_skip,
            "note": "bound = VALU issue (DESIGN.md §6): algorithmic_GBps = B_flip x flips/s is the "
                    "traffic of a one-replica CPU sweep and exceeds the HBM peak because rows are "
                    "shared by the replicas of a workgroup and stay cache-resident; the HBM side "
                    "is hbm_measured_frac.  frac is computed from PMC counters committed under "
                    "profiles/ and is null when they were not measured on the running library",
        }
        out = {
            "metric": "SA spin-flips/sec, kagome_36-sized clusters",
            "value": value,
            "unit": "spin-flips/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": "heisenberg_kagome_36-sized planted clusters K=%s, dbar=24, %d chains/GPU, "
                            "%d sweeps/step (geometric beta ladder), Metropolis single-spin-flip"
                            % ("/".join(str(s) for s in sizes), replicas, args.sweeps),
                "replicas_per_gpu": replicas,
                "sweeps_per_step": args.sweeps,
                "launch": launch,
            },
            "roofline": roofline,
            "value_no_skip": (value * kernel_flips_no_skip / kernel_flips
                              if kernel_flips_no_skip else None),
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            cores = usable_cores()
            out["cpu_baseline"] = cpu_baseline(clusters[0]["J"], clusters[0]["field"], cores,
                                               args.cpu_seconds)
        if args.full and world == 1 and not args.no_build:
            out["build"] = bench_build(clusters[-1]["J"], 1)
            out["reference_default_call"] = bench_default_call()
            out["batched_small_clusters"] = bench_batched_clusters()
            out["large_cluster"] = bench_large_cluster(replicas, args.sweeps)
            out["large_cluster"]["valu_issue_frac"] = issue_fraction(
                "colour_200000", counters, out["large_cluster"]["nibbles_kernel_flips_per_s"])
            out["batched_small_clusters"]["valu_issue_frac"] = issue_fraction(
                "batch", counters, out["batched_small_clusters"]["batched_kernel_flips_per_s"])
            out["reference_default_call"]["team_valu_issue_frac"] = issue_fraction(
                "team", counters, out["reference_default_call"]["team_flips_per_s"])
            try:
                out["real_kagome_36_clusters"] = bench_real_kagome_36(replicas, args.sweeps)
                out["real_kagome_36_clusters"]["valu_issue_frac"] = issue_fraction(
                    "real_kagome_36", counters, out["real_kagome_36_clusters"]["kernel_flips_per_s"])
            except Exception as error:  # a secondary leg never costs the headline line
                out["real_kagome_36_clusters"] = {"error": "%s: %s" % (type(error).__name__, error)}
        if args.full and world == 1:
            # (also under --no-build: it is part of what the rocprofv3 passes of the bench see)
            out["shuffled_order"] = bench_shuffled_order(clusters, replicas, args.sweeps, offset, counters)
        print(json.dumps(out))

    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
