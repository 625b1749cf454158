#!/usr/bin/env python3
"""The regime the colour sweep's tail sweeps work in, on the CPU: no GPU needed.

A statistical simulation of the bench ladder — synthetic.planted_cluster(K, seed=783494), the colours
and the order of oracle.sa_layout, the plan's automatic geometric ladder of 128 sweeps, four chains
as one workgroup, numpy random numbers.  It does not reproduce the device's chains; it measures how
many rows a sweep has to evaluate at all.  A row needs no evaluation when no neighbour has flipped in
any of the four chains since its last evaluation and all four proposals were certain rejections then
(beta * dE >= 23).  Per sweep: the flips of the group, the share of rows that need an evaluation, and
the share of 64-row blocks that hold at least one such row.

    python tools/tail_regime.py [--sizes 10000,30000] [--sweeps 128] [--every 8] [--seed 1]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import oracle  # noqa: E402
from annealing_sign_problem_amd import _lib, synthetic  # noqa: E402
from annealing_sign_problem_amd import annealer as sa  # noqa: E402


def auto_ladder(J, field, sweeps):
    n = J.shape[0]
    info = _lib.SaInfo()
    colors = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(
        n, _lib.ptr(np.ascontiguousarray(J.indptr, np.int64)), _lib.ptr(np.ascontiguousarray(J.indices, np.int32)),
        _lib.ptr(np.ascontiguousarray(J.data, np.float64)), _lib.ptr(np.ascontiguousarray(field, np.float64)),
        ctypes.byref(info), _lib.ptr(colors), _lib.ptr(position)))
    return sa.make_schedule(info.beta0_auto, info.beta1_auto, sweeps)


def regime(k, sweeps, seed, chains=4):
    """Per sweep: (flips of the group, share of rows needed, share of blocks needed)."""
    J, field, _ = synthetic.planted_cluster(k, seed=783494)
    J = scipy.sparse.csr_matrix(J)
    betas = auto_ladder(J, field, sweeps)
    A = scipy.sparse.csr_matrix(J + J.T)
    A.setdiag(0)
    A.eliminate_zeros()
    pattern = scipy.sparse.csr_matrix((np.ones(A.nnz, np.float32), A.indices, A.indptr), shape=A.shape)
    colors, order, num_colors = oracle.sa_layout(J)[:3]
    # block of every spin: a colour's spins in the plan's order, 64 to a block, every colour on blocks of its own
    block = np.zeros(k, np.int64)
    first = 0
    rows_of = []
    for c in range(num_colors):
        members = order[colors[order] == c]
        rows_of.append(members)
        block[members] = first + np.arange(members.size) // 64
        first += (members.size + 63) // 64
    rng = np.random.default_rng(seed)
    s = np.where(rng.random((k, chains)) < 0.5, -1.0, 1.0)
    stale = np.ones(k, bool)
    was_open = np.ones(k, bool)
    out = []
    for beta in betas:
        flips = 0
        needed = np.zeros(k, bool)
        for members in rows_of:
            needed[members] = stale[members] | was_open[members]
            g = A[members] @ s + field[members][:, None]
            de = -2.0 * s[members] * g
            x = beta * de
            accept = (de <= 0.0) | (rng.random(x.shape) < np.exp(-np.clip(x, 0.0, 700.0)))
            accept &= x < 23.0
            s[members] = np.where(accept, -s[members], s[members])
            stale[members] = False
            was_open[members] = (x < 23.0).any(axis=1)
            flipped = members[accept.any(axis=1)]
            flips += int(accept.sum())
            if flipped.size:
                mark = np.zeros(k, np.float32)
                mark[flipped] = 1.0
                stale |= (pattern @ mark) > 0.0
        out.append((flips, needed.mean(), np.unique(block[needed]).size / first))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="10000,30000")
    ap.add_argument("--sweeps", type=int, default=128)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",")]
    tables = {k: regime(k, args.sweeps, args.seed) for k in sizes}
    print("| t | " + " | ".join("K = %g flips | K = %g rows needed | K = %g blocks needed" % (k, k, k) for k in sizes) + " |")
    print("|---|" + "---|" * (3 * len(sizes)))
    for t in range(args.sweeps // 2, args.sweeps, args.every):
        cells = []
        for k in sizes:
            flips, rows, blocks = tables[k][t]
            cells += ["%d" % flips, "%.3g" % rows, "%.2f" % blocks]
        print("| %d | " % t + " | ".join(cells) + " |")
    for k in sizes:
        rows = np.array([r for _, r, _ in tables[k]])
        print("K = %g: rows needed over the whole ladder %.3f of all rows" % (k, rows.mean()))


if __name__ == "__main__":
    main()
