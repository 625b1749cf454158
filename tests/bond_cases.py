"""Named inputs for the bond statistics (specification ASP-BONDS-1) and the law itself,
restated sequentially in numpy: a loop over the rows, np.searchsorted for the bins.  Nothing here
imports the package's bond code; tests/test_bond_cases.py checks the restatement against the reference's
own formulas, tests/test_gpu_bonds.py the device against the restatement.

A case is ``(indptr i64, indices i32, data f64, bits u64)``.  ``VARIANTS`` names eight plausible wrong
readings of the law; ``bond_law(..., variant=name)`` computes that reading, so that a test can show
which case tells it from the law."""
import functools

import numpy as np

VARIANTS = ("ge_zero", "diagonal_counted", "signed_argmax", "tie_largest_col", "right_open_last",
            "le_inner", "bit_is_minus", "row_sign_only")


def pack(signs):
    """bit i of word i // 64 set iff signs[i] > 0 (annealer.signs_to_bits' convention)."""
    signs = np.asarray(signs)
    words = np.zeros((signs.shape[0] + 63) // 64, dtype=np.uint64)
    for i in np.flatnonzero(signs > 0):
        words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return words


def unpack(bits, count):
    bits = np.asarray(bits, dtype=np.uint64)
    return np.array([1 if (int(bits[i // 64]) >> (i % 64)) & 1 else -1 for i in range(count)], dtype=np.int64)


def bond_law(indptr, indices, data, bits, variant=None):
    """The law of §1, row by row.  Returns a dict: the summary's fields; ``strongest``,
    ``strongest_col``, ``strongest_frustrated_rows`` per row; ``magnitude`` and ``is_frustrated`` of all
    bonds in storage order (for the histogram and the sorted magnitudes)."""
    assert variant is None or variant in VARIANTS
    n = len(indptr) - 1
    signs = unpack(bits, n)
    if variant == "bit_is_minus":
        signs = -signs
    strongest = np.zeros(n)
    strongest_col = np.full(n, -1, dtype=np.int32)
    strongest_frustrated = np.zeros(n, dtype=bool)
    magnitude, is_frustrated = [], []
    extra_frustrated = 0
    for i in range(n):
        cols = np.asarray(indices[indptr[i]:indptr[i + 1]], dtype=np.int64)
        x = np.asarray(data[indptr[i]:indptr[i + 1]], dtype=np.float64)
        bond = x != 0
        if variant != "diagonal_counted":
            bond &= cols != i
        same = signs[cols] == signs[i]
        if variant == "row_sign_only":
            same = np.full(cols.shape, signs[i] > 0)
        frustrated = same == (x > 0)
        if variant == "ge_zero":  # frustration decided with >= and before the zeros are dropped
            extra_frustrated += int(np.count_nonzero((same == (x >= 0)) & (cols != i) & ~bond))
        cols, x, frustrated = cols[bond], x[bond], frustrated[bond]
        magnitude.append(np.abs(x))
        is_frustrated.append(frustrated)
        if x.size:
            key = x if variant == "signed_argmax" else np.abs(x)
            top = np.flatnonzero(key == key.max())
            pick = top[np.argmax(cols[top])] if variant == "tie_largest_col" else top[np.argmin(cols[top])]
            strongest[i] = abs(x[pick])
            strongest_col[i] = cols[pick]
            strongest_frustrated[i] = frustrated[pick]
    magnitude = np.concatenate(magnitude) if magnitude else np.zeros(0)
    is_frustrated = np.concatenate(is_frustrated) if is_frustrated else np.zeros(0, dtype=bool)
    bonds = magnitude.shape[0]
    return {
        "num_spins": n, "stored": int(indptr[-1]), "bonds": bonds,
        "frustrated": int(np.count_nonzero(is_frustrated)) + extra_frustrated,
        "rows_with_bonds": int(np.count_nonzero(strongest_col >= 0)),
        "strongest_frustrated": int(np.count_nonzero(strongest_frustrated)),
        "max_abs": float(magnitude.max()) if bonds else 0.0,
        "min_abs": float(magnitude.min()) if bonds else 0.0,
        "strongest": strongest, "strongest_col": strongest_col, "strongest_frustrated_rows": strongest_frustrated,
        "magnitude": magnitude, "is_frustrated": is_frustrated,
    }


def histogram_law(law, edges, variant=None):
    """``(normal u64[nb], frustrated u64[nb], below, above)``: bin k holds edges[k] <= |J| < edges[k+1],
    the last bin is closed on the right (np.histogram's rule)."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.shape[0] - 1
    m = law["magnitude"]
    if variant == "le_inner":
        position = np.searchsorted(edges, m, side="left")   # edges[k] < m <= edges[k+1] -> k + 1
        position = np.where(m == edges[0], 1, position)
    else:
        position = np.searchsorted(edges, m, side="right")  # number of edges <= m
        if variant != "right_open_last":
            position = np.where(m == edges[-1], nb, position)
    inside = (position >= 1) & (position <= nb)
    bins = position[inside] - 1
    flagged = law["is_frustrated"][inside]
    normal = np.bincount(bins[~flagged], minlength=nb).astype(np.uint64)
    frustrated = np.bincount(bins[flagged], minlength=nb).astype(np.uint64)
    return normal, frustrated, int(np.count_nonzero(position < 1)), int(np.count_nonzero(position > nb))


def magnitudes_law(law):
    return np.sort(law["magnitude"])[::-1]


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------

def _grid(rng, size):
    """Couplings m / 64, m = 1 .. 192, of either sign: many repeated values, and many that lie exactly on
    the dyadic edges of HISTOGRAMS."""
    return rng.integers(1, 193, size=size) / 64.0 * rng.choice([-1.0, 1.0], size=size)


def _from_rows(n, rows):
    """rows: {row: (columns, values)}, kept in the order given (unsorted columns stay unsorted)."""
    indptr = np.zeros(n + 1, dtype=np.int64)
    indices, data = [], []
    for i in range(n):
        cols, vals = rows.get(i, ((), ()))
        assert len(set(cols)) == len(cols) == len(vals)
        indices.extend(cols)
        data.extend(vals)
        indptr[i + 1] = len(indices)
    return indptr, np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=np.float64)


def _random_rows(n, seed, longest=9):
    """Every row a random number of entries in random (unsorted) unique columns, the diagonal among
    them now and then; not symmetric."""
    rng = np.random.default_rng(seed)
    rows = {}
    for i in range(n):
        length = int(rng.integers(0, min(longest, n) + 1))
        cols = rng.permutation(n)[:length]
        rows[i] = (cols.tolist(), _grid(rng, length).tolist())
    return _from_rows(n, rows)


def _random_signs(n, seed):
    return np.random.default_rng(seed).choice([-1, 1], size=n)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (indptr, indices, data, bits)}; read-only arrays, built once."""
    out = {}
    out["k0"] = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0, dtype=np.uint64))
    out["k1_diagonal_only"] = _from_rows(1, {0: ([0], [2.5])}) + (pack([1]),)
    for n in (63, 64, 65, 129):  # the tail of the sign words and the word boundary
        out["k%d" % n] = _random_rows(n, seed=n) + (pack(_random_signs(n, 1000 + n)),)
    out["k129_all_plus"] = _random_rows(129, seed=129) + (pack(np.ones(129)),)
    out["k129_alternating"] = _random_rows(129, seed=129) + (pack(1 - 2 * (np.arange(129) % 2)),)
    # rows of 0, 1, 63, 64, 65, 129 and 300 entries: less than, exactly and more than one trip of the lanes
    rng = np.random.default_rng(7)
    n, rows = 301, {}
    for i, length in enumerate((0, 1, 63, 64, 65, 129, 300)):
        rows[i] = (rng.permutation(n)[:length].tolist(), _grid(rng, length).tolist())
    rows[9] = ([9], [-1.25])  # a row that holds only its diagonal
    # values on the first, an inner and the last edge of every histogram of HISTOGRAMS, below and above
    planted = [0.5, -2.03125, 1.0, -2.0, 1.5, -1.25, 0.25, -2.75]
    long_cols, long_vals = rows[6]
    off_diagonal = [k for k, c in enumerate(long_cols) if c != 6][:len(planted)]
    for k, value in zip(off_diagonal, planted):
        long_vals[k] = value
    out["row_lengths"] = _from_rows(n, rows) + (pack(_random_signs(n, 8)),)
    # stored zeros of both signs beside real bonds; equal signs on (0, 1), (0, 2), opposite on (0, 3)
    out["stored_zeros"] = _from_rows(5, {0: ([1, 2, 3, 4], [0.0, -0.0, 0.0, 1.0]), 1: ([0, 1], [-0.0, 0.0]),
                                        3: ([4, 0], [2.0, 0.0])}) + (pack([1, 1, 1, -1, -1]),)
    tiny = np.nextafter(0.0, 1.0)
    out["subnormal"] = _from_rows(4, {0: ([1, 2, 3], [tiny, -3 * tiny, 1e-310]), 1: ([0], [-tiny]),
                                     2: ([3, 0], [2e-308, -1e-320]), 3: ([3], [tiny])}) + (pack([1, -1, 1, -1]),)
    out["non_symmetric"] = _from_rows(4, {0: ([1], [1.0]), 1: ([0, 2], [-2.0, 0.5]), 2: ([3], [0.25]),
                                         3: ([0], [-4.0])}) + (pack([1, -1, -1, 1]),)
    # +1.5 at column 5 and -1.5 at column 2: the tie goes to the smallest column
    out["tie"] = _from_rows(6, {0: ([5, 2, 3], [1.5, -1.5, 1.0]), 1: ([4, 0], [-0.5, 0.5]),
                                3: ([3, 1, 2], [9.0, 2.0, 2.0])}) + (pack([1, 1, -1, 1, -1, -1]),)
    # the strongest bond is negative, the signed maximum is another entry
    out["negative_strongest"] = _from_rows(5, {0: ([1, 4], [-3.0, 2.0]), 2: ([3, 0, 1], [0.5, -0.75, 0.25]),
                                              4: ([0], [-1.0])}) + (pack([1, 1, -1, 1, -1]),)
    # the diagonal is the largest entry of its row and would be frustrated if it counted
    out["diagonal"] = _from_rows(3, {0: ([0, 1], [5.0, -1.0]), 1: ([1, 0], [-7.0, 1.0]), 2: ([2], [1.0])}) + (pack([1, -1, 1]),)
    out["big"] = _big()
    for arrays in out.values():
        for a in arrays:
            a.flags.writeable = False
    return out


def _big():
    """About 70 000 rows and more than 2^20 stored entries (the scan's tiles, the histogram's flush of
    several workgroups), symmetric, columns sorted, the diagonal stored on every third row."""
    import scipy.sparse

    from annealing_sign_problem_amd import synthetic

    n = 70001
    rng = np.random.default_rng(20240)
    lo, hi = synthetic.random_symmetric_graph(n, 17.0, 40, rng)
    w = _grid(rng, lo.shape[0])
    diagonal = np.arange(0, n, 3)
    rows = np.concatenate([lo, hi, diagonal])
    cols = np.concatenate([hi, lo, diagonal])
    vals = np.concatenate([w, w, _grid(rng, diagonal.shape[0])])
    matrix = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    matrix.sort_indices()
    return (matrix.indptr.astype(np.int64), matrix.indices.astype(np.int32), matrix.data.astype(np.float64),
            pack(_random_signs(n, 5)))


# cases that claim mixed signs: their frustrated share must lie in 10-90 % (test_bond_cases.py)
MIXED = ("k63", "k64", "k65", "k129", "k129_alternating", "row_lengths", "big")

# (name, case, edges): nb = 1, 49 and 4096; dyadic edges, so that the grid's values fall exactly on the
# first, on inner and on the last edge, and below and above them
HISTOGRAMS = (
    ("one_bin", "k129", np.array([1.0, 2.0])),
    ("one_bin_rows", "row_lengths", np.array([1.0, 2.0])),
    ("bins49", "k129", 0.5 + np.arange(50) / 32.0),
    ("bins49_rows", "row_lengths", 0.5 + np.arange(50) / 32.0),
    ("bins49_big", "big", 0.5 + np.arange(50) / 32.0),
    ("bins4096", "row_lengths", 1.0 + np.arange(4097) / 4096.0),
    ("bins4096_big", "big", 1.0 + np.arange(4097) / 4096.0),
)


@functools.lru_cache(maxsize=None)
def law(name):
    """bond_law of a named case, computed once."""
    return bond_law(*cases()[name])
