"""Generate tests/golden/field_kagome16_cluster.npz: a cluster of the 16-site kagome model, its one-hop
environment with signed amplitudes, and the `field` that the REFERENCE's cbits/build_matrix.c (compiled in
place into oracle/_ref by oracle/build_oracle.py) returns for them with counts = 1 — the miss branch that
specification ASP-FIELD-1 restates.

Run where the reference checkout and gcc are present:

    python tests/golden/generate_field_fixtures.py

The file holds inputs and outputs only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
import field_cases  # noqa: E402


def main() -> None:
    op = field_cases.model_operator("heisenberg_kagome_16")
    c = field_cases.make_case("fixture", op, field_cases.grow(op, 60, seed=2024), seed=2025)
    _, _, _, _, field = oracle.ref_build_matrix(
        c.keys, np.ones(c.keys.size, dtype=np.int64), c.psi, c.other, c.coeffs, c.counts,
        field_cases.other_psi(c.other, c.env_keys, c.env_psi))
    law, unresolved = c.law(scale=1.0)
    assert unresolved == 0 and field_cases.same_bits(law, field)
    out = os.path.join(HERE, "field_kagome16_cluster.npz")
    np.savez_compressed(out, keys=c.keys, psi=c.psi, env_keys=c.env_keys, env_psi=c.env_psi, field=field)
    print(out, os.path.getsize(out), "bytes; K =", c.keys.size, "E =", c.env_keys.size)


if __name__ == "__main__":
    main()
