"""The models of tests/test_kloop_tail_cases.py and tests/test_gpu_kloop_tail.py: 300 to 600 spins whose
plans put every END of a block in front of the colour sweep's k-loop (csrc/sa_sweep.hip, block_row_sums:
the loop ends on the last real term of the block's longest row) — every remainder of the longest row
modulo 4, one to four quads, a block of width 1, blocks without couplings, a colour's last block with
dummy lanes, and blocks whose longest row belongs to a single lane.  What a model is built for is read
back from asp_sa_layout_host (`blocks`) and asserted in test_kloop_tail_cases.py, so that a change of a
generator or of the plan cannot silently empty a class."""
import ctypes

import numpy as np
import scipy.sparse

SWEEPS_HOT, SWEEPS_FROZEN = 14, 8  # a hot-to-cold ladder, then sweeps that accept nothing uphill


def _symmetric(n, lo, hi, w):
    J = scipy.sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))),
                                shape=(n, n)).tocsr()
    J.sum_duplicates()
    J.sort_indices()
    return J


def _circulants(degrees, sides=2):
    """`sides` bipartite 32 + 32 circulant components per degree d (row i of one side meets rows
    i .. i + d - 1 mod 32 of the other): with two colours each holds 32 * sides rows of every degree.
    Returns (lo, hi, number of spins); component c of degree number k starts at (k * sides + c) * 64."""
    lo, hi = [], []
    base = 0
    for d in degrees:
        for _ in range(sides):
            i = np.repeat(np.arange(32), d)
            k = np.tile(np.arange(d), 32)
            lo.append(base + i)
            hi.append(base + 32 + (i + k) % 32)
            base += 64
    return np.concatenate(lo), np.concatenate(hi), base


def _finish(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)  # spins in no particular order: the plan's permutation does the work
    w = rng.normal(size=lo.shape[0])
    field = rng.normal(size=n) * 0.3  # (nowhere 0: an isolated spin is not flipped for nothing)
    return _symmetric(n, perm[lo], perm[hi], w), field


def ladder():
    """Blocks of 64 rows of degree 16, 11, 6 and 1 in either colour — four quads with remainder 0, three
    with 3, two with 2, one with 1 (a block of width 1) — and 66 isolated spins: a block of width 0 and a
    last block of two rows and 62 dummy lanes.  578 spins."""
    lo, hi, n = _circulants((16, 11, 6, 1))
    return _finish(n + 66, lo, hi, 31)


def short_rows():
    """Blocks of 64 rows of degree 8, 5, 4 and 3: two quads with remainders 0 and 1, one quad with
    remainders 0 and 3 — the quads that end a block on its first or on its only load.  512 spins."""
    lo, hi, n = _circulants((8, 5, 4, 3))
    return _finish(n, lo, hi, 37)


def single_lane():
    """Degrees 13 and 2, one more coupling between a row of one degree-13 component and a row of the
    other, and a coupled pair of spins: in either colour one row of degree 14 (four quads, remainder 2) is
    the only longest row of its block, in front of 63 rows of degree 13; then a block of degree 2; and the
    colour ends with a block of one row of degree 1 and 63 dummy lanes.  258 spins."""
    lo, hi, n = _circulants((13, 2))
    lo = np.concatenate([lo, [5, n]])
    hi = np.concatenate([hi, [64 + 32 + 9, n + 1]])
    return _finish(n + 2, lo, hi, 41)


CASES = {"ladder": ladder, "short_rows": short_rows, "single_lane": single_lane}


def blocks(J, field):
    """Per block of the host plan: (longest row, lanes that hold a row of that length, live lanes), and the
    plan's summary.  The degree of a row: its off-diagonal entries in J + J^T."""
    from annealing_sign_problem_amd import _lib

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
    block = (position // 64).astype(np.int64)
    longest = np.zeros(info.num_blocks, np.int64)
    np.maximum.at(longest, block, degree)
    holders = np.bincount(block[degree == longest[block]], minlength=info.num_blocks)
    live = np.bincount(block, minlength=info.num_blocks)
    # the last block of every colour (a colour's blocks are consecutive, colours in ascending order)
    last_of_colour = np.zeros(info.num_blocks, bool)
    for c in range(info.num_colors):
        last_of_colour[block[colour == c].max()] = True
    return longest, holders, live, last_of_colour, info


def classes(longest, holders, live, last_of_colour):
    """The classes of block ends a plan covers, as a set of names."""
    seen = set()
    for width, lanes, rows, last in zip(longest, holders, live, last_of_colour):
        if width == 0:
            seen.add("width 0")
            if rows < 64:
                seen.add("width 0 with dummy lanes")
            continue
        seen.add("remainder %d" % (width % 4))
        seen.add("%d quads" % ((width + 3) // 4))
        if width == 1:
            seen.add("width 1")
        if last and rows < 64:
            seen.add("last block of a colour with dummy lanes")
        if lanes == 1 and rows > 1:
            seen.add("one lane holds the longest row")
    return seen


REQUIRED = {"remainder 0", "remainder 1", "remainder 2", "remainder 3", "1 quads", "2 quads", "3 quads", "4 quads",
            "width 1", "last block of a colour with dummy lanes", "one lane holds the longest row", "width 0"}


def betas_of(info):
    """SWEEPS_HOT sweeps down the plan's automatic ladder — nearly every proposal accepted at first — and
    SWEEPS_FROZEN at a beta that accepts nothing uphill: the chains fall into a local minimum, the sweeps'
    flips go to zero, and the field cache or tail mode (a sweep with fewer flips than a threshold of at
    least one) is entered for the last sweeps."""
    from annealing_sign_problem_amd import annealer as sa

    hot = sa.make_schedule(info.beta0_auto, info.beta1_auto, SWEEPS_HOT)
    return np.concatenate([hot, np.full(SWEEPS_FROZEN, 1e12)])
