"""What a colour sweep costs outside its visits (development aid).

Fully frozen sweeps as tools/time_frozen.py runs them — the greedy minimum as x0, beta = 1e15, field
cache on, M = 4, 1024 threads — at K = 1e4, 3e4 and 1e5.  After the first sweeps every block is
clean and inert, so a sweep is the skip scan over its blocks, one barrier per colour and the sweep
end.  A least-squares line of the time per sweep against the skipped blocks per wavefront gives
  intercept = colour barriers + sweep end,   slope = one skipped block.
The first sweeps of a launch evaluate every block (the cache is entered, then the inert bytes are
set), so the frozen cost is the difference of a long and a short launch over the sweeps between."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from annealing_sign_problem_amd import _lib, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402

THREADS, M, GROUPS = 1024, 4, 256
SHORT, LONG, REPEAT = 64, 1088, 5
lib = _lib.load()
rows = []
for k in (10000, 30000, 100000):
    J, h, _ = synthetic.planted_cluster(k, seed=783494)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    x0, _ = sa.greedy_solve(ham)          # a local minimum: nothing flips at huge beta
    _lib.check(lib.asp_sa_set_field_cache(ham.plan(), 1))
    _lib.check(lib.asp_sa_set_launch(ham.plan(), M, THREADS))
    ms = {}
    for sweeps in (SHORT, LONG):
        betas = np.full(sweeps, 1e15)
        best = float("inf")
        for _ in range(REPEAT):
            sa.anneal_raw(ham, 1, betas, M * GROUPS, 0, x0)
            best = min(best, lib.asp_sa_last_sweep_ms(ham.plan()))
        ms[sweeps] = best
        acc = np.zeros(M * GROUPS, np.uint64)
        lib.asp_sa_last_stats(ham.plan(), M * GROUPS, None, _lib.ptr(acc))
        assert acc.sum() == 0, "the start is no local minimum: the sweeps are not frozen"
    us = (ms[LONG] - ms[SHORT]) / (LONG - SHORT) * 1e3
    skipped = info.num_blocks / (THREADS // 64)
    rows.append((skipped, us))
    print("K=%d blocks=%d colours=%d: %.3f us per frozen sweep, %.1f skipped blocks per wavefront "
          "(launches of %d / %d sweeps: %.3f / %.3f ms)"
          % (k, info.num_blocks, info.num_colors, us, skipped, SHORT, LONG, ms[SHORT], ms[LONG]), flush=True)
    ham.release()
x, y = np.array(rows).T
slope, intercept = np.polyfit(x, y, 1)
print("fit: intercept %.3f us per sweep (colour barriers + sweep end), slope %.4f us per skipped block"
      % (intercept, slope))
print("residuals (us):", " ".join("%.3f" % r for r in y - (slope * x + intercept)))
