#!/usr/bin/env python3
"""What the colour sweep's k-loop evaluates and the result does not need, counted
on the CPU from the host plan: no GPU needed.

Per plan — the three bench clusters synthetic.planted_cluster(K, seed=783494) and one sparse model
(mean_degree = 8.0):
  * the padding terms every lane of a block shares: sum over blocks of (width rounded to whole quads -
    longest row), per row (64 rows to a block, dummy lanes included: a visit evaluates them), per real
    spin and as a share of the ELL slots;
  * the share of blocks with an even quad count (> 0), whose visit prefetched one quad past the block;
  * the quads and the quads' loads (three per quad) of a sweep over every block, with and without the
    over-read.

    python tools/kloop_padding.py [--sizes 10000,30000,100000] [--sparse 100000]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from annealing_sign_problem_amd import _lib, synthetic  # noqa: E402


def block_widths(J, field):
    """(longest row of every block, number of spins): the plan's blocks from asp_sa_layout_host."""
    Jc = scipy.sparse.csr_matrix(J)
    n = Jc.shape[0]
    info = _lib.SaInfo()
    colour = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(
        n, _lib.ptr(np.ascontiguousarray(Jc.indptr, np.int64)), _lib.ptr(np.ascontiguousarray(Jc.indices, np.int32)),
        _lib.ptr(np.ascontiguousarray(Jc.data, np.float64)), _lib.ptr(np.ascontiguousarray(field, np.float64)),
        ctypes.byref(info), _lib.ptr(colour), _lib.ptr(position)))
    pattern = scipy.sparse.csr_matrix((np.ones_like(Jc.data), Jc.indices, Jc.indptr), shape=Jc.shape)
    pattern = (pattern + pattern.T).tolil()
    pattern.setdiag(0)
    pattern = pattern.tocsr()
    pattern.eliminate_zeros()
    degree = np.diff(pattern.indptr)
    longest = np.zeros(info.num_blocks, np.int64)
    np.maximum.at(longest, position // 64, degree)
    return longest, n, int(degree.sum())


def report(name, J, field):
    longest, n, nnz = block_widths(J, field)
    rounded = (longest + 3) // 4 * 4
    quads = rounded // 4
    blocks = longest.size
    removable = int((rounded - longest).sum())
    even = int(((quads % 2 == 0) & (quads > 0)).sum())
    slots = int(rounded.sum()) * 64
    loads_old = 3 * int((quads + (quads % 2 == 0)).sum())  # quads = 0 loaded one quad as well
    loads_new = 3 * int(quads.sum())
    print("%-22s spins %7d blocks %5d  mean degree %.2f  ELL slots / nnz %.3f" % (name, n, blocks, nnz / n, slots / nnz))
    print("    removable terms (rounded width - longest row): %d = %.3f per row of a block, %.3f per spin, "
          "%.2f %% of the ELL slots" % (removable, removable / blocks, removable * 64 / n, 100.0 * removable * 64 / slots))
    print("    remainder of the longest row mod 4 (0,1,2,3): %s blocks" % np.bincount(longest % 4, minlength=4).tolist())
    print("    blocks with an even quad count: %d of %d = %.1f %%; vector loads per sweep over every block "
          "%d -> %d (-%.2f %%)" % (even, blocks, 100.0 * even / blocks, loads_old, loads_new,
                                  100.0 * (loads_old - loads_new) / loads_old))
    print("    mean quads per block %.2f; terms evaluated per row %.2f -> %.2f (-%.2f %%)"
          % (quads.mean(), rounded.mean(), longest.mean(), 100.0 * removable / rounded.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,30000,100000")
    ap.add_argument("--sparse", type=int, default=100000)
    args = ap.parse_args()
    for k in [int(s) for s in args.sizes.split(",") if s]:
        J, h, _ = synthetic.planted_cluster(k, seed=783494)
        report("bench K=%d" % k, J, h)
    if args.sparse:
        J, h, _ = synthetic.planted_cluster(args.sparse, seed=1, mean_degree=8.0)
        report("sparse d=8 K=%d" % args.sparse, J, h)


if __name__ == "__main__":
    main()
