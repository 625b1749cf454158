"""Law ASP-ICM-1 restated in plain Python — the checker of tests/test_cluster_move_abi.py
and tests/test_gpu_cluster_move.py, never imported by the package.

Python floats are IEEE doubles with one rounding per operation, so the row sums below are the device's
``fma(A_ij, +-1.0, acc)`` (the product is exact) and ``oracle.philox4x32_10`` restates its random words.
Configurations are packed as everywhere (bit = +1, 64 spins per word, original order); a state is the
dict of ``Chains.state()``.
"""
import numpy as np
import scipy.sparse

import oracle

DRAW_WORD = 0xFFFFFFFB  # word 2 of the Philox counter: proposals and starts have < 2^30 there, the
                        # priorities 0xFFFFFFFE, the resampling 0xFFFFFFFD, the exchange 0xFFFFFFFC


def couplings(J):
    """§4.2: A = offdiag(J + J^T), exact zeros dropped, as a canonical CSR."""
    m = scipy.sparse.csr_matrix(J, dtype=np.float64)
    a = scipy.sparse.csr_matrix(m + m.T)
    a.setdiag(0.0)
    a.eliminate_zeros()
    a.sort_indices()
    return a


def bits(x, K):
    """A packed configuration as a bool array of K spins (True = +1)."""
    x = np.ascontiguousarray(x, dtype="<u8").reshape(-1)
    return np.unpackbits(x.view(np.uint8), bitorder="little")[:K].astype(bool)


def pack(up):
    up = np.asarray(up, dtype=bool)
    K = up.shape[0]
    words = (K + 63) // 64
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:K] = up
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def draw_word(seed, a, sweeps_done, draw):
    """Step 2: word 0 of Philox4x32-10(counter (a, sweeps_done, 0xFFFFFFFB, draw), key seed)."""
    seed = int(seed) & (2 ** 64 - 1)
    return int(oracle.philox4x32_10([int(a), int(sweeps_done), DRAW_WORD, int(draw)],
                                    [seed & 0xFFFFFFFF, seed >> 32])[0])


def seed_index(v, n):
    """Step 2: U = floor(v n / 2^32)."""
    return (int(v) * int(n)) >> 32


def component(A, d, i0):
    """Step 3: the connected component of i0 in A's graph induced on {d = 1}, by a hand search."""
    inside = np.zeros(d.shape[0], dtype=bool)
    inside[i0] = True
    todo = [i0]
    while todo:
        i = todo.pop()
        for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
            if d[j] and not inside[j]:
                inside[j] = True
                todo.append(int(j))
    return inside


def delta(A, h, S, up_a, d, inside):
    """Step 4: Q = sum over C of rint(dE_i 2^S), the row sums over the neighbours with d = 0 in
    ascending column."""
    Q = 0
    scale = 2.0 ** S
    for i in np.flatnonzero(inside):
        acc = 0.0
        for k in range(A.indptr[i], A.indptr[i + 1]):
            j = A.indices[k]
            if d[j]:
                continue
            acc = acc + (float(A.data[k]) if up_a[j] else -float(A.data[k]))
        g = acc + float(h[i])
        de = -2.0 * g if up_a[i] else 2.0 * g
        Q += int(np.rint(de * scale))
    return Q


def pair_move(A, h, S, K, xa, xb, v):
    """Steps 1-5 for one pair with the random word v: (new xa, new xb, n, size, Q)."""
    up_a, up_b = bits(xa, K), bits(xb, K)
    d = up_a ^ up_b
    n = int(d.sum())
    if n == 0:
        return np.array(xa, dtype=np.uint64), np.array(xb, dtype=np.uint64), 0, 0, 0
    i0 = int(np.flatnonzero(d)[seed_index(v, n)])
    inside = component(A, d, i0)
    Q = delta(A, h, S, up_a, d, inside)
    return pack(up_a ^ inside), pack(up_b ^ inside), n, int(inside.sum()), Q


def move(J, h, S, state, seed, pairs, draw, words=None):
    """The whole law on a ``Chains.state()`` dict: (new state, differing uint32[P], sizes uint32[P],
    deltas int64[P]).  ``words``: {a: v} to replace the Philox words (for the tests of the law itself)."""
    A = couplings(J)
    K = A.shape[0]
    new = {name: np.array(value, copy=True) for name, value in state.items()}
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert np.unique(pairs).size == pairs.size
    differing = np.zeros(len(pairs), dtype=np.uint32)
    sizes = np.zeros(len(pairs), dtype=np.uint32)
    deltas = np.zeros(len(pairs), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        v = words[a] if words is not None else draw_word(seed, a, state["sweeps_done"], draw)
        xa, xb, n, size, Q = pair_move(A, h, S, K, state["x_current"][a], state["x_current"][b], v)
        differing[p], sizes[p], deltas[p] = n, size, Q
        if n == 0:
            continue
        new["x_current"][a], new["x_current"][b] = xa, xb
        new["tracked_current"][a] += Q
        new["tracked_current"][b] -= Q
        for r in (a, b):  # step 6
            if new["tracked_current"][r] < new["tracked_best"][r]:
                new["tracked_best"][r] = new["tracked_current"][r]
                new["x_best"][r] = new["x_current"][r]
    return new, differing, sizes, deltas


def energy(J, h, up):
    """s^T J s + h^T s of a bool configuration, in plain numpy."""
    s = np.where(up, 1.0, -1.0)
    return float(s @ (scipy.sparse.csr_matrix(J) @ s) + np.dot(h, s))
