"""Generate tests/golden/noise_stats.npz from the REFERENCE's postprocess_influence_of_noise
(annealing_sign_problem/common.py:906-937), loaded the way generate_golden.py loads that module.

    python tests/golden/generate_noise_golden.py

The input is a synthetic three-column table (eps, amplitude overlap, sign overlap) with empty bins,
bins of one row, values on bin edges and an amplitude overlap of exactly 0 (which no bin holds); the
file keeps the table and the four columns the reference wrote — arrays only."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from generate_golden import load_reference_common  # noqa: E402


def synthetic_table() -> np.ndarray:
    rng = np.random.default_rng(20260)
    n = 600
    amplitude = np.concatenate([rng.uniform(0.3, 1.0, n - 8), [0.0, 0.01, 0.02, 0.5, 0.5, 1.0, 1.0, 0.255]])
    sign = np.clip(amplitude[: n] ** 2 + rng.normal(scale=0.1, size=n), -1.0, 1.0)
    sign[-1] = 1.0
    eps = np.repeat(np.geomspace(1e-2, 1e2, n // 10), 10)
    return np.column_stack([eps, amplitude, np.abs(sign)])


def main() -> None:
    ref = load_reference_common()
    table = synthetic_table()
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, "noise.csv")
        with open(name, "w") as f:
            for row in table:
                f.write("{},{},{}\n".format(*row))
        ref.postprocess_influence_of_noise(name)
        stats = np.loadtxt(os.path.join(tmp, "noise_stats.csv"), delimiter=",", skiprows=1)
        with open(os.path.join(tmp, "noise_stats.csv")) as f:
            header = f.readline().strip()
    assert header == "amplitude_overlap,median,upper,lower"
    np.savez(os.path.join(HERE, "noise_stats.npz"), table=table, stats=stats)
    print("noise_stats.npz: table", table.shape, "stats", stats.shape)


if __name__ == "__main__":
    main()
