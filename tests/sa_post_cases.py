"""The clusters of tests/test_sa_post_cases.py and tests/test_gpu_sa_post.py: the smallest ones that
put every shape of block in front of the pass after the sweeps (k_sa_post) — a single spin, blocks with dummy lanes,
a full block, every quad count from 0 to 5 and a partial-sum tree of two levels.  The structure each
case is named for is read back from asp_sa_layout_host (`layout`) and asserted in
test_sa_post_cases.py, so a change of a generator or of the plan cannot silently empty a case."""
import ctypes

import numpy as np
import scipy.sparse

SMALL_SIZES = (1, 63, 64, 65, 130)
LADDER_DEGREES = (3, 7, 11, 15, 19)  # rows per block: largest degree in 1-4, 5-8, ..., 17-20
LADDER_ISOLATED = 70                 # more than a block of isolated spins: one block of width 0
LARGE_SPINS, LARGE_DEGREE, LARGE_SEED = 4200, 6.0, 77
COUNTS = (1, 7, 8, 9, 11, 64)        # configurations per energies() call
CHAINS = (8, 11)
SWEEPS = 8


def _symmetric(n, lo, hi, w, diagonal):
    J = scipy.sparse.coo_matrix((np.concatenate([w, w, diagonal]),
                                 (np.concatenate([lo, hi, np.arange(n)]), np.concatenate([hi, lo, np.arange(n)]))),
                                shape=(n, n)).tocsr()
    J.sum_duplicates()
    J.sort_indices()
    return J


def small(n):
    """K = 1 and 64, 65: no couplings (one colour: one block of one live lane, one full block, a full
    block and one of a single live lane); K = 63: a path (two colours, dummy lanes in both blocks);
    K = 130: a ring with chords (several colours and blocks).  Diagonal entries and a field everywhere."""
    rng = np.random.default_rng(1000 + n)
    if n == 63:
        lo = np.arange(n - 1)
        hi = lo + 1
    elif n == 130:
        lo = np.concatenate([np.arange(n), np.arange(0, n, 3)])
        hi = np.concatenate([(np.arange(n) + 1) % n, (np.arange(0, n, 3) + 16) % n])
    else:
        lo = hi = np.zeros(0, np.int64)
    w = rng.normal(size=lo.shape[0])
    return _symmetric(n, lo, hi, w, rng.normal(size=n)), rng.normal(size=n)


def width_ladder():
    """Two 32 + 32 circulant bipartite components per degree d in LADDER_DEGREES (row i of one side
    meets rows i .. i + d - 1 mod 32 of the other), so that each of the two colours holds exactly 64 rows
    of every degree — one block of width d rounded up to 4 —, and LADDER_ISOLATED isolated spins, which
    end the first colour with a block of width 0."""
    rng = np.random.default_rng(2024)
    lo, hi = [], []
    base = 0
    for d in LADDER_DEGREES:
        for _ in range(2):
            i = np.repeat(np.arange(32), d)
            k = np.tile(np.arange(d), 32)
            lo.append(base + i)
            hi.append(base + 32 + (i + k) % 32)
            base += 64
    n = base + LADDER_ISOLATED
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    perm = rng.permutation(n)  # spins in no particular order: the plan's permutation does the work
    w = rng.normal(size=lo.shape[0])
    diagonal = np.where(rng.random(n) < 0.5, rng.normal(size=n), 0.0)
    return _symmetric(n, perm[lo], perm[hi], w, diagonal), rng.normal(size=n) * 0.3


def large():
    """A planted cluster of LARGE_SPINS spins with mean degree LARGE_DEGREE: more than 64 blocks, so the
    fold of the partial sums has a second level, whose last group of 64 is not full."""
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(LARGE_SPINS, mean_degree=LARGE_DEGREE, max_degree=14, seed=LARGE_SEED)
    return J.tocsr(), np.random.default_rng(LARGE_SEED).normal(size=LARGE_SPINS) * 1e-3


CASES = {("K%d" % n): (lambda n=n: small(n)) for n in SMALL_SIZES}
CASES["ladder"] = width_ladder
CASES["large"] = large


def layout(J, field):
    """(colour[K], position[K], width[num_blocks], info) of the host plan: the block of a spin is
    position // 64, the width of a block the largest off-diagonal degree of its rows in J + J^T, rounded
    up to whole quads."""
    from annealing_sign_problem_amd import _lib

    Jc = scipy.sparse.csr_matrix(J)
    n = Jc.shape[0]
    indptr = np.ascontiguousarray(Jc.indptr, np.int64)
    indices = np.ascontiguousarray(Jc.indices, np.int32)
    data = np.ascontiguousarray(Jc.data, np.float64)
    info = _lib.SaInfo()
    colour = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(n, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                              _lib.ptr(np.ascontiguousarray(field, np.float64)),
                                              ctypes.byref(info), _lib.ptr(colour), _lib.ptr(position)))
    pattern = scipy.sparse.csr_matrix((np.ones_like(Jc.data), Jc.indices, Jc.indptr), shape=Jc.shape)
    pattern = (pattern + pattern.T).tolil()
    pattern.setdiag(0)
    pattern = pattern.tocsr()
    pattern.eliminate_zeros()
    degree = np.diff(pattern.indptr)
    width = np.zeros(info.num_blocks, np.int64)
    np.maximum.at(width, position // 64, degree)
    return colour, position, (width + 3) // 4 * 4, info


def configurations(n, count, seed=5):
    """`count` packed configurations of n spins: all up, all down, then random ones."""
    from annealing_sign_problem_amd import annealer as sa

    rng = np.random.default_rng(seed)
    rows = [np.ones(n), -np.ones(n)] + [rng.choice([-1.0, 1.0], size=n) for _ in range(max(count - 2, 0))]
    return np.stack([sa.signs_to_bits(r) for r in rows[:count]])
