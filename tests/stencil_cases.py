"""ASP-STENCIL-1 (include/asp.h) restated in numpy from connection lists, for
tests/test_gpu_stencil.py to compare the device with and for tests/test_stencil_cases.py to keep honest
against scipy's ``0.5 * (M + M.T)`` on hand-built matrices.

A connection list is CSR-like: row ``i``'s connections are ``targets[offsets[i]:offsets[i + 1]]`` (the
index of the target among the keys, ``-1`` for a target outside the cluster) with ``coeffs`` beside
them, in connection order.  Python floats are IEEE doubles and every ``*`` and ``+`` below rounds on its
own, which is all the law asks for."""
import numpy as np
import scipy.sparse


def resolve(keys, other_keys):
    """Indices of ``other_keys`` among the sorted unique ``keys``, -1 where absent."""
    keys = np.asarray(keys, dtype=np.uint64)
    other_keys = np.asarray(other_keys, dtype=np.uint64)
    if keys.shape[0] == 0:
        return np.full(other_keys.shape, -1, dtype=np.int64)
    at = np.minimum(np.searchsorted(keys, other_keys), keys.shape[0] - 1)
    return np.where(keys[at] == other_keys, at, -1).astype(np.int64)


def folds(offsets, targets, coeffs, psi):
    """``{(i, j): Mhat_ij}``: per (row, target) group the fold from +0.0 of ``(c * |psi_j|) * |psi_i|`` in
    connection order.  A pair without a connection has no key."""
    mhat = {}
    magnitude = [abs(float(x)) for x in psi]
    for i in range(len(offsets) - 1):
        for c in range(int(offsets[i]), int(offsets[i + 1])):
            j = int(targets[c])
            if j < 0:
                continue
            element = (float(coeffs[c]) * magnitude[j]) * magnitude[i]
            mhat[(i, j)] = mhat.get((i, j), 0.0) + element
    return mhat


def pair_sum(mhat, i, j):
    """``Mhat_ij + Mhat_ji``, a side without a connection contributing +0.0."""
    return mhat.get((i, j), 0.0) + mhat.get((j, i), 0.0)


def couplings(offsets, targets, coeffs, psi):
    """The canonical CSR ``(indptr, indices, data)`` of J: entry (i, j) exists iff the pair's sum is
    non-zero, and holds half of it."""
    mhat = folds(offsets, targets, coeffs, psi)
    n = len(offsets) - 1
    pairs = set(mhat) | {(j, i) for i, j in mhat}
    rows = [[] for _ in range(n)]
    for i, j in sorted(pairs):
        total = pair_sum(mhat, i, j)
        if total != 0.0:
            rows[i].append((j, 0.5 * total))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    indices = np.array([j for r in rows for j, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return indptr, indices, data


def values(offsets, targets, coeffs, psi, indptr, indices):
    """``(data, changed)`` on a GIVEN pattern: the stored pairs' values in pattern order, and whether a
    stored pair sums to exactly 0 or a silent pair (a connection, no entry) does not."""
    mhat = folds(offsets, targets, coeffs, psi)
    n = len(offsets) - 1
    stored = set()
    data = np.zeros(len(indices), dtype=np.float64)
    changed = False
    for i in range(n):
        for k in range(int(indptr[i]), int(indptr[i + 1])):
            j = int(indices[k])
            stored.add((i, j))
            total = pair_sum(mhat, i, j)
            data[k] = 0.5 * total
            changed = changed or total == 0.0
    for i, j in mhat:
        if (i, j) not in stored and (j, i) not in stored and pair_sum(mhat, i, j) != 0.0:
            changed = True
    return data, changed


def silent_pairs(offsets, targets, indptr, indices):
    """The unordered pairs with a connection and no entry."""
    n = len(offsets) - 1
    stored = {(i, int(indices[k])) for i in range(n) for k in range(int(indptr[i]), int(indptr[i + 1]))}
    silent = set()
    for i in range(n):
        for c in range(int(offsets[i]), int(offsets[i + 1])):
            j = int(targets[c])
            if j >= 0 and (i, j) not in stored and (j, i) not in stored:
                silent.add((min(i, j), max(i, j)))
    return silent


def scipy_couplings(offsets, targets, coeffs, psi):
    """make_ising_model's host route: the elements as a CSR matrix with its duplicates, unsorted columns
    and explicit zeros (targets outside the cluster: column clipped to 0, value 0), then scipy's
    ``0.5 * (M + M.T)`` with sorted indices."""
    n = len(offsets) - 1
    magnitude = np.abs(np.asarray(psi, dtype=np.float64))
    targets = np.asarray(targets, dtype=np.int64)
    inside = targets >= 0
    cols = np.where(inside, targets, 0)
    rows = np.repeat(np.arange(n), np.diff(offsets))
    elements = np.where(inside, (np.asarray(coeffs, dtype=np.float64) * magnitude[cols]) * magnitude[rows], 0.0)
    matrix = scipy.sparse.csr_matrix((elements, cols.astype(np.int32), np.asarray(offsets, dtype=np.int32)),
                                     shape=(n, n))
    matrix = 0.5 * (matrix + matrix.T)
    matrix = scipy.sparse.csr_matrix(matrix)
    matrix.sort_indices()
    return matrix.indptr.astype(np.int64), matrix.indices.astype(np.int32), matrix.data


# ---- hand-built connection lists ------------------------------------------------------------------------
def _list(rows):
    """rows: per row a list of (target, coefficient)."""
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    targets = np.array([t for r in rows for t, _ in r], dtype=np.int64)
    coeffs = np.array([c for r in rows for _, c in r], dtype=np.float64)
    return offsets, targets, coeffs


TINY = 5e-324  # the smallest subnormal: half of it rounds to 0

HAND_BUILT = {
    "plain symmetric": _list([[(0, 1.0), (1, 2.0)], [(1, -1.0), (0, 2.0)]]),
    "duplicate columns": _list([[(0, 0.5), (1, 1.0), (1, 0.25), (2, 3.0)], [(1, 1.0), (0, 1.25)],
                                [(2, 0.0), (0, 3.0), (0, -1.0), (0, 1.0)]]),
    "explicit zeros": _list([[(0, 0.0), (1, 0.0)], [(1, 2.0), (0, 0.0), (2, 1.0)], [(2, 0.0), (1, 1.0)]]),
    "one-sided": _list([[(0, 1.0), (1, 4.0), (2, -3.0)], [(1, 1.0)], [(2, 1.0), (1, 0.5)]]),
    "duplicate of the diagonal": _list([[(0, 1.0), (1, 2.0), (0, 0.125), (0, -3.0)], [(1, 0.0), (0, 2.0), (1, 7.0)]]),
    "order-dependent": _list([[(0, 1.0), (1, 1e16), (1, 1.0), (1, -1e16)], [(1, 1.0), (0, 3.0), (0, 1e16), (0, -1e16)],
                              [(2, 1e16), (2, 1.0), (2, -1e16)]]),
    "cancelling pair": _list([[(0, 1.0), (1, 0.75)], [(1, 1.0), (0, -0.75)]]),
    "minus zero": _list([[(0, -0.0), (1, -0.0), (2, 1.0)], [(1, 2.0), (0, -0.0)], [(2, -0.0), (0, -1.0)]]),
    "subnormals": _list([[(0, TINY), (1, TINY), (2, 3 * TINY)], [(1, 2 * TINY), (0, TINY), (2, TINY)],
                         [(2, TINY), (0, 2e-310)]]),
    "large and small": _list([[(0, 2.0 ** 500), (1, 2.0 ** 500), (2, 2.0 ** -500)],
                              [(1, -2.0 ** -500), (0, 2.0 ** 500), (2, 2.0 ** 500)],
                              [(2, 2.0 ** 500), (0, 2.0 ** -500), (1, -2.0 ** 500), (1, 2.0 ** -500)]]),
    "targets outside": _list([[(0, 1.0), (-1, 5.0), (1, 2.0), (-1, 1.0)], [(1, 1.0), (-1, 2.0), (0, 2.0)]]),
    "empty rows": _list([[], [(1, 1.0)], []]),
}
