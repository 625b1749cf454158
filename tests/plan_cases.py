"""Shared cases and numpy restatements for asp_sa_plan_create_segments (law ASP-PLAN-SEG-1, DESIGN.md
§4.15).  A SEGMENT is (indptr i64, indices i32, data f64, field f64) of one canonical CSR matrix; a ROUND
is a list of segments; `concatenate` gives the call's arguments.  `plan_front` restates the front of the
law (A = offdiag(J + J^T) as CSR, the stored diagonals, the row statistics, whether a mirror is missing),
`plan_scales` the fold of the row statistics, `plan_blocks` the block structure that follows from the
colours and positions, `plan_fill` the quad-interleaved fill of the arrays a plan holds."""
import functools
import math

import numpy as np

DUMMY = 0xFFFFFFFF  # spin_of_pos of a padding lane
TAIL_SLABS = 8      # zero slabs behind the last block
ARRAYS = ("color_block_start", "block_width", "ell_off", "ell_col", "ell_col4", "ell_val", "spin_of_pos",
          "pos_of_spin", "field_pos")


def segment(n, rows, cols, vals, field=None):
    """Canonical CSR of the given entries (no duplicates expected; explicit zeros are kept)."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n)) if n else 0
    field = np.zeros(n) if field is None else np.asarray(field, dtype=np.float64)
    return indptr, cols[order].astype(np.int32), vals[order].copy(), field.copy()


def symmetric(n, edges, weights, field=None, diagonal=None):
    """J_ij = J_ji = w for every edge (i, j), optionally a stored diagonal (dict spin -> value)."""
    i, j = (np.array(edges, dtype=np.int64).reshape(-1, 2).T if len(edges) else (np.empty(0, np.int64),) * 2)
    w = np.asarray(weights, dtype=np.float64)
    rows, cols, vals = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([w, w])
    if diagonal:
        d = np.array(sorted(diagonal), dtype=np.int64)
        rows, cols = np.concatenate([rows, d]), np.concatenate([cols, d])
        vals = np.concatenate([vals, [diagonal[k] for k in d]])
    return segment(n, rows, cols, vals, field)


def empty():
    return np.zeros(1, dtype=np.int64), np.empty(0, dtype=np.int32), np.empty(0), np.empty(0)


def isolated(n, seed=0):
    """n spins without couplings: one colour, width-0 blocks, padding lanes."""
    return symmetric(n, [], [], field=np.random.default_rng(seed).normal(size=n))


def matching(pairs, seed=1):
    """`pairs` disjoint edges (i, i + pairs): two colour classes of exactly `pairs` members."""
    rng = np.random.default_rng(seed)
    return symmetric(2 * pairs, [(i, i + pairs) for i in range(pairs)], rng.normal(size=pairs))


def cliques(sizes, seed=2):
    """Disjoint cliques: rows of degree size - 1."""
    rng = np.random.default_rng(seed)
    edges, first = [], 0
    for size in sizes:
        edges += [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]
        first += size
    return symmetric(first, edges, rng.normal(size=len(edges)), field=rng.normal(size=first) * 0.1)


def hub(leaves=300, seed=3):
    rng = np.random.default_rng(seed)
    return symmetric(leaves + 1, [(0, k) for k in range(1, leaves + 1)], rng.normal(size=leaves))


def random_sparse(n, seed, mean_degree=3.0, diagonal=True):
    rng = np.random.default_rng(seed)
    count = int(n * mean_degree / 2)
    pairs = {tuple(sorted(p)) for p in rng.integers(0, n, size=(count, 2)).tolist() if p[0] != p[1]}
    edges = sorted(pairs)
    diag = {int(k): float(rng.normal()) for k in range(n) if diagonal and rng.random() < 0.3}
    return symmetric(n, edges, rng.normal(size=len(edges)), field=rng.normal(size=n) * 0.2, diagonal=diag)


def cubic(n):
    """A ring with its diameters: every spin has degree 3 (n even)."""
    edges = [(i, (i + 1) % n) for i in range(n)] + [(i, i + n // 2) for i in range(n // 2)]
    edges = [tuple(sorted(e)) for e in edges]
    w = np.random.default_rng(5).normal(size=len(edges))
    return symmetric(n, edges, w)


def planted(n, mean_degree, seed=783494):
    from annealing_sign_problem_amd import synthetic

    matrix, field, _ = synthetic.planted_cluster(n, mean_degree=mean_degree, seed=seed)
    matrix = matrix.tocsr()
    matrix.sort_indices()
    return (matrix.indptr.astype(np.int64), matrix.indices.astype(np.int32), matrix.data.astype(np.float64),
            np.asarray(field, dtype=np.float64))


# ---- the value edges, one small segment each -------------------------------------------------------

def with_diagonal():
    return symmetric(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1.0, -2.0, 0.5, 0.25], diagonal={0: 0.5, 3: -1.5, 4: 0.0})


def without_diagonal():
    return symmetric(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1.0, -2.0, 0.5, 0.25])


def zeros_and_cancelling():
    """Stored +0.0 pair, stored -0.0 pair (-0.0 + -0.0 = -0.0 == 0: dropped), J_ij = -J_ji (dropped), and
    two couplings that stay."""
    rows = [0, 1, 1, 2, 2, 3, 3, 4, 0, 4]
    cols = [1, 0, 2, 1, 3, 2, 4, 3, 4, 0]
    vals = [0.0, 0.0, -0.0, -0.0, 0.75, -0.75, 1.5, 1.5, -2.0, -2.0]
    return segment(5, rows, cols, vals)


def subnormal():
    tiny = 5e-324
    return symmetric(4, [(0, 1), (1, 2), (2, 3)], [tiny, 3 * tiny, 1e-310], field=[0.0, tiny, 0.0, 0.0])


def value_asymmetric():
    """The pattern is symmetric, the values are not: A_ij = J_ij + J_ji, one rounded sum."""
    rows = [0, 1, 1, 2, 0, 2]
    cols = [1, 0, 2, 1, 2, 0]
    vals = [0.1, 0.2, 1e16, 1.0, -3.0, 0.3]
    return segment(3, rows, cols, vals, field=[0.5, -0.5, 0.25])


def upper_triangular():
    return segment(4, [0, 0, 1, 2, 1], [1, 3, 2, 3, 1], [1.0, -0.5, 2.0, 0.25, 7.0])


def one_missing_mirror():
    ip, ix, dv, h = symmetric(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [1.0, 2.0, -1.0, 0.5, 3.0])
    at = int(ip[5])  # the only entry of row 5: (5, 4) goes, (4, 5) stays
    ip = ip.copy()
    ip[6] -= 1
    return ip, np.delete(ix, at), np.delete(dv, at), h


def with_field():
    return symmetric(4, [(0, 1), (2, 3)], [1.0, -1.0], field=[0.3, -0.7, 0.0, 1e-3])


def value_edge():
    """Everything above in one connected segment (the use tests run on it)."""
    rows = [0, 1, 1, 2, 2, 3, 3, 4, 0, 4, 5, 4, 5, 6, 6, 0, 2, 7, 6]
    cols = [1, 0, 2, 1, 3, 2, 4, 3, 4, 0, 4, 5, 6, 5, 0, 6, 2, 6, 7]
    vals = [0.0, 0.0, -0.0, -0.0, 0.75, -0.75, 1.5, 1.25, -2.0, -2.0, 5e-324, 5e-324, 0.5, 0.5, 1e-3, 2e-3, 0.5, 4.0,
            1.0]
    return segment(8, rows, cols, vals, field=[0.1, 0.0, -0.2, 0.0, 0.0, 1e-300, 0.0, 0.3])


VALUE_SEGMENTS = {
    "diagonal": with_diagonal, "no_diagonal": without_diagonal, "zeros": zeros_and_cancelling,
    "subnormal": subnormal, "value_asymmetric": value_asymmetric, "upper_triangular": upper_triangular,
    "missing_mirror": one_missing_mirror, "field": with_field, "value_edge": value_edge,
}
HOST_FRONT = {"upper_triangular", "missing_mirror"}


@functools.lru_cache(maxsize=None)
def rounds():
    """name -> list of segments.  Built once and shared; nobody writes into them."""
    out = {
        "empty_first_middle_last": [empty(), random_sparse(9, 11), empty(), empty(), random_sparse(70, 12), empty()],
        "only_empty": [empty(), empty()],
        "one_spin": [isolated(1), symmetric(1, [], [], field=[0.0], diagonal={0: 2.5})],
        "isolated": [isolated(63, 1), isolated(64, 2), isolated(65, 3), isolated(130, 4)],
        "class_of_64": [matching(64)],
        "class_of_65": [matching(65)],
        "widths": [cliques([2, 5, 6, 9, 10])],
        "hub_300": [hub(300)],
        "values": [VALUE_SEGMENTS[name]() for name in VALUE_SEGMENTS],
        "round_of_1": [random_sparse(150, 21)],
        "round_of_3": [random_sparse(33, 22), random_sparse(400, 23, mean_degree=5.0), random_sparse(7, 24)],
        "round_of_128": [random_sparse(1 + (7 * g) % 40, 100 + g, diagonal=g % 3 == 0) for g in range(128)],
        "planted_20000": [planted(20000, 6.0)],
        "cubic_45000": [cubic(45000)],
    }
    for segments in out.values():
        for seg in segments:
            for array in seg:
                array.flags.writeable = False
    return out


def concatenate(segments):
    """(offsets u64, indptr, indices, data, field) of a round, the call's conventions."""
    offsets = np.zeros(len(segments) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([s[0].size - 1 for s in segments], dtype=np.uint64)
    indptr, entries = [np.zeros(1, dtype=np.int64)], 0
    for ip, _, _, _ in segments:
        indptr.append(ip[1:] + entries)
        entries += int(ip[-1])
    return (offsets, np.concatenate(indptr), np.concatenate([s[1] for s in segments]).astype(np.int32),
            np.concatenate([s[2] for s in segments]).astype(np.float64),
            np.concatenate([s[3] for s in segments]).astype(np.float64))


# ---- restatements ------------------------------------------------------------------------------------

def _sequential_sum(values):
    total = 0.0
    for v in values:
        total = total + v  # plain f64 adds, left to right
    return total


def plan_front(indptr, indices, data, field):
    """The front of the law for one segment: A = offdiag(J + J^T) with exact zeros dropped (x + y with x
    = J_ij or +0.0 and y = J_ji or +0.0), as CSR in ascending column order; the stored diagonal; per row
    sum_k |A_ik| added left to right and the smallest non-zero 2 |A_ik| (inf: none); and whether some stored
    off-diagonal entry has no stored mirror (the segment then takes the host's front)."""
    n = indptr.size - 1
    if n == 0:
        return {"a_ptr": np.zeros(1, dtype=np.int64), "a_col": np.empty(0, np.int32), "a_val": np.empty(0),
                "diagonal": np.empty(0), "has_diagonal": np.empty(0, bool), "row_sum": np.empty(0),
                "row_min": np.empty(0), "host_front": False, "dropped": 0}
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices.astype(np.int64)
    keys = rows * n + cols          # ascending: the CSR is canonical
    mirror = cols * n + rows
    off = rows != cols

    def lookup(wanted):
        """(found, value or +0.0) of the stored entries with the keys `wanted`."""
        values = np.zeros(wanted.size)
        if keys.size == 0:
            return np.zeros(wanted.size, dtype=bool), values
        where = np.minimum(np.searchsorted(keys, wanted), keys.size - 1)
        ok = keys[where] == wanted
        values[ok] = data[where[ok]]
        return ok, values

    host_front = bool(np.any(off & ~lookup(mirror)[0]))
    every = np.union1d(keys[off], mirror[off])  # the pattern of J + J^T off the diagonal, row-major
    x = lookup(every)[1]
    y = lookup((every % n) * n + every // n)[1]
    with np.errstate(over="ignore"):
        v = x + y
    keep = v != 0.0
    a_rows, a_col, a_val = (every // n)[keep], (every % n)[keep].astype(np.int32), v[keep]
    a_ptr = np.zeros(n + 1, dtype=np.int64)
    a_ptr[1:] = np.cumsum(np.bincount(a_rows, minlength=n))
    diagonal, has_diagonal = np.zeros(n), np.zeros(n, dtype=bool)
    diagonal[rows[~off]] = data[~off]
    has_diagonal[rows[~off]] = True
    row_sum, row_min = np.zeros(n), np.full(n, np.inf)
    magnitude = np.abs(a_val)
    for i in range(n):
        mine = magnitude[a_ptr[i]:a_ptr[i + 1]]
        row_sum[i] = _sequential_sum(mine.tolist())
        if np.any(mine > 0.0):
            row_min[i] = 2.0 * mine[mine > 0.0].min()
    return {"a_ptr": a_ptr, "a_col": a_col, "a_val": a_val, "diagonal": diagonal, "has_diagonal": has_diagonal,
            "row_sum": row_sum, "row_min": row_min, "host_front": host_front,
            "dropped": int(np.count_nonzero(~keep))}


def plan_scales(front, field):
    """diag_sum, energy_scale_exp, beta0_auto, beta1_auto from the row statistics, folded in row order."""
    diag = 0.0
    for d, has in zip(front["diagonal"].tolist(), front["has_diagonal"].tolist()):
        if has:
            diag = diag + d
    bound, max_delta, min_delta = 0.0, 0.0, math.inf
    for row, least, h in zip(front["row_sum"].tolist(), front["row_min"].tolist(), np.abs(field).tolist()):
        min_delta = min(min_delta, least)
        if h > 0.0:
            min_delta = min(min_delta, 2.0 * h)
        bound += 0.5 * row + h
        max_delta = max(max_delta, 2.0 * (row + h))
    exponent = 0
    if bound > 0.0:
        exponent = max(-1000, min(1000, min(60 - math.frexp(2.0 * bound)[1], 50 - math.frexp(max_delta)[1])))
    if max_delta > 0.0 and math.isfinite(min_delta):
        beta0, beta1 = math.log(2.0) / max_delta, math.log(100.0) / min_delta
    else:
        beta0 = beta1 = 1.0
    return {"diag_sum": diag, "energy_scale_exp": exponent, "beta0_auto": beta0, "beta1_auto": beta1}


def plan_blocks(a_ptr, colors, positions):
    """The block structure that follows from the colours and positions of the host layout: 64-row blocks,
    a colour class a run of blocks, widths the largest degree of the block rounded up to 4."""
    n = a_ptr.size - 1
    if n == 0:
        return {"num_blocks": 0, "num_colors": 0, "color_block_start": np.zeros(1, np.uint32),
                "block_width": np.empty(0, np.uint32), "ell_off": np.zeros(1, np.uint64),
                "spin_of_pos": np.empty(0, np.uint32)}
    degree = np.diff(a_ptr)
    num_blocks = int(positions.max()) // 64 + 1
    num_colors = int(colors.max()) + 1
    spin_of_pos = np.full(num_blocks * 64, DUMMY, dtype=np.uint32)
    spin_of_pos[positions] = np.arange(n, dtype=np.uint32)
    widest = np.zeros(num_blocks, dtype=np.int64)
    np.maximum.at(widest, positions // 64, degree)
    block_width = ((widest + 3) // 4 * 4).astype(np.uint32)
    ell_off = np.zeros(num_blocks + 1, dtype=np.uint64)
    ell_off[1:] = np.cumsum(block_width, dtype=np.uint64)
    first_block = np.full(num_colors + 1, num_blocks, dtype=np.uint32)
    np.minimum.at(first_block, colors, (positions // 64).astype(np.uint32))
    return {"num_blocks": num_blocks, "num_colors": num_colors, "color_block_start": first_block,
            "block_width": block_width, "ell_off": ell_off, "spin_of_pos": spin_of_pos}


def plan_fill(A, positions, block_width, ell_off, field):
    """The arrays a plan holds besides the structure, in the quad-interleaved layout: entry k of the lane
    at position b * 64 + l lies in quad Q = (ell_off[b] + k) // 4, j = k % 4, at
    ell_col[(Q * 64 + l) * 4 + j] and ell_val[((Q * 2 + j // 2) * 64 + l) * 2 + j % 2]; columns are
    POSITIONS; padding entries carry the lane's own position and +0.0; TAIL_SLABS slabs of zeros follow."""
    a_ptr, a_col, a_val = A["a_ptr"], A["a_col"], A["a_val"]
    n = a_ptr.size - 1
    num_blocks = block_width.size
    if n == 0:
        return {"ell_col": np.empty(0, np.uint32), "ell_col4": np.empty(0, np.uint32), "ell_val": np.empty(0),
                "field_pos": np.empty(0), "pos_of_spin": np.empty(0, np.uint32)}
    slabs = int(ell_off[num_blocks])
    ell_col = np.zeros((slabs + TAIL_SLABS) * 64, dtype=np.uint32)
    ell_val = np.zeros((slabs + TAIL_SLABS) * 64, dtype=np.float64)
    field_pos = np.zeros(num_blocks * 64)
    field_pos[positions] = field
    # padding first: every slot (b, l, k) of every block holds the lane's own position
    pos = np.arange(num_blocks * 64, dtype=np.int64)
    b, lane = pos // 64, pos % 64
    for k in range(int(block_width.max()) if num_blocks else 0):
        wide = block_width[b] > k
        quad = (ell_off[b].astype(np.int64) + k) // 4
        ell_col[((quad * 64 + lane) * 4 + k % 4)[wide]] = pos[wide]
    # the entries of A
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(a_ptr))
    k = np.arange(a_col.size, dtype=np.int64) - a_ptr[rows]
    p = positions[rows].astype(np.int64)
    quad = (ell_off[p // 64].astype(np.int64) + k) // 4
    j = k % 4
    ell_col[(quad * 64 + p % 64) * 4 + j] = positions[a_col]
    ell_val[((quad * 2 + j // 2) * 64 + p % 64) * 2 + j % 2] = a_val
    return {"ell_col": ell_col, "ell_col4": ell_col * np.uint32(4), "ell_val": ell_val, "field_pos": field_pos,
            "pos_of_spin": positions.astype(np.uint32)}


# ---- errors ---------------------------------------------------------------------------------------------

def _good():
    return random_sparse(12, 31)


def _broken(change):
    ip, ix, dv, h = (a.copy() for a in random_sparse(12, 32))
    change(ip, ix, dv, h)
    return ip, ix, dv, h


def _set(which, position, value):
    def change(ip, ix, dv, h):
        (ip, ix, dv, h)[which][position] = value
    return change


def _unsorted(ip, ix, dv, h):
    row = int(np.argmax(np.diff(ip) >= 2))
    ix[ip[row]], ix[ip[row] + 1] = ix[ip[row] + 1], ix[ip[row]]


def _duplicate(ip, ix, dv, h):
    row = int(np.argmax(np.diff(ip) >= 2))
    ix[ip[row] + 1] = ix[ip[row]]


def _overflow(ip, ix, dv, h):
    dv[:] = np.where(dv < 0, -8e307, 8e307)  # finite, symmetric; the bound is not


CONTENT_ERRORS = {
    "column_too_large": _set(1, 3, 12), "column_negative": _set(1, 0, -1), "unsorted_row": _unsorted,
    "duplicate_column": _duplicate, "nan_coupling": _set(2, 5, np.nan), "inf_coupling": _set(2, 1, np.inf),
    "nan_field": _set(3, 7, np.nan), "inf_field": _set(3, 0, -np.inf), "overflowing_bound": _overflow,
}


def content_error_round(name):
    """The error in the second of three segments."""
    return [_good(), _broken(CONTENT_ERRORS[name]), _good()]
