"""Named synthetic inputs for the sector route of the bond statistics (asp_sector_bonds_create,
BondStatistics.from_sector; DESIGN.md §3.6, "The whole sector") and its law, restated twice: vectorised
in numpy (`sector_law`) and as a plain double loop written from the header's text (`sector_law_rows`).
Nothing here imports the package's bond code; tests/test_sector_bond_cases.py checks the two restatements
against each other and shows which case tells each wrong reading from the law,
tests/test_gpu_sector_bonds.py the device against the restatement.

A case is ``(idx u32[width, n], val f64[width, n], psi f64[n])``, slot-major as asp_sector_rows writes
it: slot k of row i at ``[k, i]``, an unused slot holds ``(i, 0.0)``.  ``VARIANTS`` names plausible wrong
readings of the law; ``sector_law_rows(..., variant=name)`` and ``sector_signs(..., variant=name)``
compute that reading."""
import collections.abc
import functools

import numpy as np

# the first nine are wrong; the last two are symmetries of the law (no input can tell them apart)
VARIANTS = ("first_slot_only", "adjacent_dedupe", "symmetric_assumed", "hji_from_first_slot", "other_association",
            "sum_then_scale", "diagonal_kept", "cancel_kept", "tie_largest_col", "zero_row_kept", "sign_gt")
SYMMETRIES = ("zero_row_kept", "sign_gt")


def sector_law(idx, val, psi):
    """CSR ``(indptr, indices, data)`` of the sector's Ising model, columns ascending.
    H_ij = sum in slot order, from +0.0, of val over the slots of row i with idx == j;
    M_ij = (H_ij |psi_j|) |psi_i|; J_ij = 0.5 (M_ij + M_ji); kept iff J_ij != 0, j != i.
    The device stores a row's entries in the order of their first slot, this restatement by ascending
    column: no statistic of the handle sees the order within a row (counts, extrema, the tie rule by
    column, a histogram and a sorted copy), so the two are compared through the statistics."""
    width, n = idx.shape
    if n == 0 or width == 0:
        return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)
    rows = np.repeat(np.arange(n, dtype=np.int64), width)
    cols = idx.T.astype(np.int64).ravel()     # row i's slots, in slot order
    vals = val.T.ravel()
    key = rows * n + cols
    order = np.argsort(key, kind="stable")    # (slot order survives within a pair)
    key, vals = key[order], vals[order]
    pairs, start, count = np.unique(key, return_index=True, return_counts=True)
    group = np.repeat(np.arange(pairs.shape[0]), count)
    rank = np.arange(key.shape[0]) - start[group]
    h = np.zeros(pairs.shape[0])              # +0.0
    for r in range(int(count.max())):         # one addition per pair and pass: strictly in slot order
        now = rank == r
        h[group[now]] = h[group[now]] + vals[now]
    i, j = pairs // n, pairs % n
    off = i != j
    pairs, i, j, h_ij = pairs[off], i[off], j[off], h[off]
    if pairs.shape[0] == 0:
        return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)
    at = np.searchsorted(pairs, j * n + i)
    found = (at < pairs.shape[0]) & (pairs[np.minimum(at, pairs.shape[0] - 1)] == j * n + i)
    h_ji = np.where(found, h_ij[np.minimum(at, pairs.shape[0] - 1)], 0.0)
    a = np.abs(psi)
    m_ij = (h_ij * a[j]) * a[i]
    m_ji = (h_ji * a[i]) * a[j]
    coupling = 0.5 * (m_ij + m_ji)
    keep = coupling != 0
    indptr = np.concatenate([[0], np.cumsum(np.bincount(i[keep], minlength=n))]).astype(np.int64)
    return indptr, j[keep].astype(np.int32), coupling[keep]


def sector_law_rows(idx, val, psi, variant=None):
    """The same law as a double loop over rows and slots (include/asp.h); a row's entries
    in the order of their first slot.  ``variant``: one of VARIANTS, that reading instead
    (`tie_largest_col` and `sign_gt` do not touch the matrix: bond_cases.bond_law and `sector_signs` take
    them)."""
    assert variant is None or variant in VARIANTS
    width, n = idx.shape
    slots = [[int(idx[k, i]) for k in range(width)] for i in range(n)]
    values = [[float(val[k, i]) for k in range(width)] for i in range(n)]
    amplitude = [abs(float(x)) for x in psi]
    half = np.float64(0.5)

    def gathered(row, target, first=0, only_first=False):
        total = np.float64(0.0)
        for e in range(first, width):
            if slots[row][e] == target:
                total = total + np.float64(values[row][e])
                if only_first:
                    break
        return total

    indptr, indices, data = [0], [], []
    for i in range(n):
        mine = np.float64(amplitude[i])
        if mine == 0 and variant != "zero_row_kept":
            indptr.append(len(indices))
            continue
        for k in range(width):
            j = slots[i][k]
            if j == i and variant != "diagonal_kept":
                continue
            if variant == "adjacent_dedupe":
                seen = k > 0 and slots[i][k - 1] == j
            else:
                seen = j in slots[i][:k]
            if seen:
                continue
            theirs = np.float64(amplitude[j])
            if theirs == 0 and variant != "zero_row_kept":
                continue
            only_first = variant == "first_slot_only"
            h_ij = gathered(i, j, first=k, only_first=only_first)
            if variant == "symmetric_assumed":
                h_ji = h_ij
            else:
                h_ji = gathered(j, i, first=k if variant == "hji_from_first_slot" else 0, only_first=only_first)
            if variant == "other_association":
                m_ij = h_ij * (theirs * mine)
                m_ji = h_ji * (mine * theirs)
                coupling = half * (m_ij + m_ji)
            elif variant == "sum_then_scale":
                coupling = ((half * (h_ij + h_ji)) * theirs) * mine
            else:
                m_ij = (h_ij * theirs) * mine
                m_ji = (h_ji * mine) * theirs
                coupling = half * (m_ij + m_ji)
            if coupling != 0 or variant == "cancel_kept":
                indices.append(j)
                data.append(float(coupling))
        indptr.append(len(indices))
    return (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32),
            np.asarray(data, dtype=np.float64))


def sector_signs(psi, variant=None):
    """+1 / -1 per state: s_i = +1 iff psi_i >= 0, so both zeros are +1 (`sign_gt`: psi_i > 0)."""
    psi = np.asarray(psi)
    return np.where(psi > 0 if variant == "sign_gt" else psi >= 0, 1, -1)


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------

def _ell(n, width, rows):
    """rows: per row a list of (target, value) slots, kept in the order given; the rest is padding."""
    idx = np.tile(np.arange(n, dtype=np.uint32), (width, 1))
    val = np.zeros((width, n))
    for i, row in enumerate(rows):
        assert len(row) <= width
        for k, (j, v) in enumerate(row):
            assert 0 <= j < n
            idx[k, i] = j
            val[k, i] = v
    return idx, val


def _random_psi(rng, n):
    """Standard normal, about 15 % exact zeros of both signs."""
    psi = rng.standard_normal(n)
    zero = rng.random(n) < 0.15
    psi[zero] = np.where(rng.random(n) < 0.5, 0.0, -0.0)[zero]
    return psi


def _random_ell(n, seed, width=7, fill=0.7, second_slot=0.3, one_sided=None):
    """Random pairs until about ``fill`` of the slots are used; a pair gets a second slot on either side
    with probability ``second_slot``; ``one_sided``: the share of pairs present in one row only (default:
    none on even n, half on odd n); one row in eight gets a diagonal slot with a value; then padding
    ``(i, 0.0)`` up to the width and a permutation of every row's slots, so that padding and other
    targets sit between the slots of a pair."""
    rng = np.random.default_rng(seed)
    if one_sided is None:
        one_sided = 0.5 if n % 2 else 0.0
    rows = [[] for _ in range(n)]
    for i in np.flatnonzero(rng.random(n) < 0.125):
        rows[i].append((int(i), float(rng.standard_normal())))
    used, target = sum(len(r) for r in rows), int(fill * n * width)
    for _ in range(20 * n * width):
        if used >= target:
            break
        i, j = (int(x) for x in rng.integers(0, n, size=2))
        sides = [(i, j)] if rng.random() < one_sided else [(i, j), (j, i)]
        need = [1 + int(rng.random() < second_slot) for _ in sides]
        if i == j or any(len(rows[a]) + c > width for (a, _), c in zip(sides, need)):
            continue
        for (a, b), c in zip(sides, need):
            for _ in range(c):
                rows[a].append((b, float(rng.standard_normal())))
                used += 1
    for i in range(n):
        rows[i] += [(i, 0.0)] * (width - len(rows[i]))
        rows[i] = [rows[i][k] for k in rng.permutation(width)]
    return _ell(n, width, rows) + (_random_psi(rng, n),)


def _order():
    """Row 0 reaches state 1 through slots 0, 2 and 4 with 1e16, 1, -1e16: in slot order the sum is 0
    (1e16 + 1 rounds to 1e16), with the two large values first it is 1, the first slot alone is 1e16.
    Rows 1, 2 and 3 reach a target through non-adjacent slots with padding or another target between; no
    Ĥ_ij equals its Ĥ_ji; row 1's first slot towards 0 is slot 3, and row 0 holds slots towards 1
    before that."""
    rows = [
        [(1, 1e16), (2, 0.7), (1, 1.0), (3, 0.3), (1, -1e16)],
        [(2, 0.11), (1, 0.0), (3, -0.23), (0, 0.37), (2, 0.05)],
        [(0, -0.9), (1, 0.13), (2, 0.0), (1, -0.021), (3, 0.6)],
        [(3, 0.0), (1, 0.77), (0, -0.45), (2, 0.31), (0, 0.19)],
    ]
    return _ell(4, 5, rows) + (np.array([0.83, -0.41, 0.29, -0.67]),)


def _tie():
    """Row 0 holds +1 towards state 2 in slot 0 and +1 towards state 1 in slot 1; the amplitudes are
    0.5 everywhere, so the two couplings are 0.25 bit for bit.  s_0 = s_1 = +1, s_2 = -1: the bond to
    1 is frustrated, the bond to 2 is not.  The tie goes to the smallest column, 1, which sits in the
    LATER slot."""
    rows = [[(2, 1.0), (1, 1.0)], [(0, 1.0)], [(0, 1.0)], [(3, 0.0)]]
    return _ell(4, 2, rows) + (np.array([0.5, 0.5, -0.5, 0.5]),)


def _one_sided(n=9, seed=77):
    """Every coupling in one row only: Ĥ_ji = 0 and row j has no entry towards i."""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(n)]
    for i in range(n):
        for j in rng.permutation(n)[:3]:
            j = int(j)
            if j != i and all(t != i for t, _ in rows[j]) and all(t != j for t, _ in rows[i]):
                rows[i].append((j, float(rng.standard_normal())))
    psi = rng.standard_normal(n)
    return _ell(n, 3, rows) + (psi,)


def _all_zero_psi():
    idx, val, _ = _random_ell(65, seed=1065)
    return idx, val, np.where(np.arange(65) % 3 == 0, -0.0, 0.0)


_BUILDERS = {
    "n0": lambda: (np.zeros((0, 0), dtype=np.uint32), np.zeros((0, 0)), np.zeros(0)),
    "n1": lambda: _ell(1, 1, [[(0, 2.5)]]) + (np.array([-0.7]),),
    "n2": lambda: _ell(2, 1, [[(1, 0.75)], [(0, -1.25)]]) + (np.array([0.6, -0.8]),),
    "width0": lambda: (np.zeros((0, 65), dtype=np.uint32), np.zeros((0, 65)),
                       _random_psi(np.random.default_rng(65), 65)),
    "all_zero_psi": _all_zero_psi,
    # wavefront, workgroup and (2048) the scan's tile
    "n63": lambda: _random_ell(63, seed=63),
    "n64": lambda: _random_ell(64, seed=64),
    "n65": lambda: _random_ell(65, seed=65),
    "n255": lambda: _random_ell(255, seed=255),
    "n256": lambda: _random_ell(256, seed=256),
    "n257": lambda: _random_ell(257, seed=257),
    "n2049": lambda: _random_ell(2049, seed=2049),
    # a row wider than a wavefront; a third of the used slots repeat their pair
    "wide": lambda: _random_ell(130, seed=130, width=70, second_slot=0.5),
    "one_sided": _one_sided,
    "order": _order,
    # the two products are +0.18 and -0.18 bit for bit: J = 0, no entry
    "cancel": lambda: _ell(2, 1, [[(1, 0.5)], [(0, -0.5)]]) + (np.array([0.6, -0.6]),),
    # (1 * 1e-200) * 1e-200 = 0: no entry
    "underflow": lambda: _ell(3, 2, [[(1, 1.0), (2, 1.0)], [(0, 1.0), (2, 1.0)], [(0, 1.0), (1, 1.0)]])
    + (np.array([1e-200, -1e-200, 1e-200]),),
    # (3 * 1.1e-160) * 1.5e-160 is subnormal and not 0: kept
    "subnormal": lambda: _ell(2, 1, [[(1, 3.0)], [(0, 3.0)]]) + (np.array([1.5e-160, -1.1e-160]),),
    "tie": _tie,
    # more rows than 16 workgroups of four wavefronts on each of 256 CUs: the row pass strides
    "large": lambda: _random_ell(20000, seed=20000, width=5),
}


class _Cases(collections.abc.Mapping):
    """name -> (idx, val, psi); read-only arrays, each case built on first use."""

    def __init__(self, builders):
        self._builders, self._built = builders, {}

    def __getitem__(self, name):
        if name not in self._built:
            arrays = self._builders[name]()
            for a in arrays:
                a.flags.writeable = False
            self._built[name] = arrays
        return self._built[name]

    def __iter__(self):
        return iter(self._builders)

    def __len__(self):
        return len(self._builders)


CASES = _Cases(_BUILDERS)
RANDOM = ("n63", "n64", "n65", "n255", "n256", "n257", "n2049", "wide")
LARGE = ("large",)  # the vectorised law only
SMALL = tuple(name for name in CASES if name not in LARGE)


@functools.lru_cache(maxsize=None)
def law(name):
    """sector_law of a named case, computed once."""
    out = sector_law(*CASES[name])
    for a in out:
        a.flags.writeable = False
    return out


def histogram_edges(bonds, log_edges):
    """The 50 edges of the reference's log-space histogram (``log_edges``: bonds.log_edges, handed in so
    that this module imports nothing of the package) for a bond_cases.bond_law result with bonds.  Where
    the magnitudes span fewer doubles than edges, neighbours coincide: the handle wants strictly
    ascending edges, so duplicates are dropped, and a single edge gets its successor as a second."""
    hi = np.log(bonds["max_abs"])
    edges = np.unique(log_edges(max(hi - 20.0, np.log(bonds["min_abs"])), hi, 50))
    if edges.shape[0] < 2:
        edges = np.append(edges, np.nextafter(edges[-1], np.inf))
    return edges
