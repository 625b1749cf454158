"""The cases of tests/test_gpu_prep_edges.py and tests/test_prep_cases.py: inputs for the small integer
kernels that prepare a cluster before it is annealed — csrc/sparsify.hip, csrc/ising_elements.hip,
csrc/key_table.hip and the device-wide exclusive scan of csrc/asp_common.hip — at the sizes and
values where such kernels go wrong: a second 64-lane step of a row loop, a scan tile edge (2048),
the second chunk of the scan of the tile totals (more than 256 tiles: n > 524288), a second
grid-stride step of k_abs_max (more than 2^20 non-zeros), keys with bit 63 set, empty rows, needles
outside the key range.

A helper module like tests/sector_cases.py: no fixtures, no files, nothing compiled.  The right
answers are plain numpy restatements written here (`ising_elements`, `table_index`) and, for the
sparsification, oracle.sparsify_component.  Next to each stand named WRONG variants, a few lines
apart from the right one; tests/test_prep_cases.py asserts on the CPU that every one of them is
told apart by a named case, so that the GPU comparison cannot pass a kernel with that mistake.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np
import scipy.sparse
from scipy.sparse.csgraph import connected_components

SCAN_TILE = 2048                   # kScanThreads * kScanItems
SCAN_TOTALS_CHUNK = 256 * 2048     # k_scan_totals takes a second step above this many items
ABS_MAX_STRIDE = 4096 * 256        # k_abs_max: at most 4096 blocks of 256 threads
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable[[], object]     # -> SparsifyInput | IsingInput | TableInput
    reaches: Tuple[str, ...]       # the kernel paths this case is there for


# ==================================================================================================
# asp_ising_elements
# ==================================================================================================
def ising_elements(keys, psi, other_keys, other_coeffs, other_counts, *, signed=False, side="left",
                   first_of_equal_offsets=False, other_association=False):
    """``(other_indices i64[N], member bool[N], elements f64[N], offsets i64[K+1])`` of
    common.ising_elements.  The keyword arguments switch on the WRONG variants."""
    keys = np.asarray(keys, dtype=np.uint64)
    needles = np.asarray(other_keys, dtype=np.uint64)
    psi = np.asarray(psi, dtype=np.float64)
    coeffs = np.asarray(other_coeffs, dtype=np.float64)
    counts = np.asarray(other_counts, dtype=np.int64)
    k, n = keys.shape[0], needles.shape[0]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.float64), offsets
    if signed:      # WRONG: the keys compared as int64
        at = np.searchsorted(keys.view(np.int64), needles.view(np.int64), side=side)
    else:
        at = np.searchsorted(keys, needles, side=side)
    index = np.clip(at, 0, k - 1).astype(np.int64)
    member = keys[index] == needles
    if first_of_equal_offsets:   # WRONG: lower bound of e among the row starts — an empty row's
        e = np.arange(n, dtype=np.int64)            # start equals the next row's
        row = np.searchsorted(offsets[:-1], e, side="left")
        row = row - ((row == k) | (offsets[np.minimum(row, k - 1)] != e))
    else:
        row = np.repeat(np.arange(k), counts)
    other = np.where(member, psi[index], 0.0)
    if other_association:        # WRONG: coeff * (|other| * |psi_row|)
        elements = coeffs * (np.abs(other) * np.abs(psi[row]))
    else:
        elements = (coeffs * np.abs(other)) * np.abs(psi[row])
    return index, member, elements, offsets


ISING_VARIANTS = {
    "signed key comparison": dict(signed=True),
    'side="right"': dict(side="right"),
    "empty rows mishandled in the row lookup": dict(first_of_equal_offsets=True),
    "the other association of the two products": dict(other_association=True),
}


@dataclass(frozen=True)
class IsingInput:
    keys: np.ndarray
    psi: np.ndarray
    other_keys: np.ndarray
    other_coeffs: np.ndarray
    other_counts: np.ndarray

    @property
    def args(self):
        return self.keys, self.psi, self.other_keys, self.other_coeffs, self.other_counts


def _amplitudes(rng, k):
    """Both signs, exact zeros, magnitudes over eight decades (far from the subnormals, so that no
    product of three factors leaves the normal range)."""
    psi = rng.choice([-1.0, 1.0], size=k) * 10.0 ** rng.uniform(-8.0, 0.0, size=k)
    psi[rng.random(k) < 0.1] = 0.0
    return psi


def _needles(rng, keys, n):
    """Present keys, absent values between keys and next to keys, and the ends of the range."""
    k = keys.shape[0]
    needles = rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)   # absent, between
    kind = rng.integers(0, 10, size=n)
    at = rng.integers(0, k, size=n)
    needles[kind < 5] = keys[at[kind < 5]]                                        # present
    needles[kind == 5] = keys[at[kind == 5]] + np.uint64(1)                       # just above a key
    needles[kind == 6] = keys[at[kind == 6]] - np.uint64(1)                       # just below a key
    special = [np.uint64(0), U64_MAX, keys[0], keys[-1], keys[k // 2], keys[0] - np.uint64(1),
               keys[-1] + np.uint64(1)]
    where = rng.permutation(n)[:len(special)]
    needles[where] = np.array(special, dtype=np.uint64)[:where.shape[0]]
    return needles


def make_ising(k, seed, counts=None, per_row=3):
    """``k`` sorted keys from the full uint64 range with one repeated key; a fifth of the rows,
    the first and the last are empty, one row has about 700 connections, N is no multiple of 256.
    ``counts`` overrides the row lengths (the degenerate sizes)."""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.integers(1 << 20, (1 << 64) - (1 << 20), size=k, dtype=np.uint64))
    if k >= 3:
        keys[k // 2 + 1] = keys[k // 2]          # the entry point accepts non-strictly sorted keys
    if counts is None:
        counts = rng.integers(1, per_row + 1, size=k).astype(np.int64)
        counts[rng.random(k) < 0.2] = 0
        counts[2 * k // 3] = 700
        counts[[0, 1, k - 1]] = [0, 0, 0]        # (two empty rows in a row at the start)
        if int(counts.sum()) % 256 == 0:
            counts[2 * k // 3] += 1
    counts = np.asarray(counts, dtype=np.int64)
    n = int(counts.sum())
    needles = _needles(rng, keys, n) if k else np.zeros(0, np.uint64)
    coeffs = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.1, 3.0, size=n)
    return IsingInput(keys, _amplitudes(rng, k), needles, coeffs, counts)


def _ising_case(k, seed, why, **kwargs):
    return Case("ising K=%d%s" % (k, "".join(" %s=%s" % kv for kv in sorted(kwargs.items()))),
                lambda: _ising_input(k, seed, tuple(sorted(kwargs.items()))), why)


@functools.lru_cache(maxsize=None)
def _ising_input(k, seed, kwargs):
    kwargs = dict(kwargs)
    if "counts" in kwargs:
        kwargs["counts"] = list(kwargs["counts"])
    return make_ising(k, seed, **kwargs)


ISING_CASES = (
    _ising_case(0, 1, ("K = N = 0: k_scan_empty, no launch of k_ising_elements",), counts=()),
    _ising_case(1, 2, ("N = 0 with K > 0: the scan alone",), counts=(0,)),
    _ising_case(1, 3, ("K = 1: every needle clipped to index 0, hi = 1 in both bisections",), counts=(7,)),
    _ising_case(2, 5, ("K = 2, first row empty: connection 0 belongs to row 1, whose amplitude differs",),
                counts=(0, 5)),
    _ising_case(2, 4, ("K = 2, last row empty",), counts=(5, 0)),
    _ising_case(255, 6, ("K = 255: one scan tile, last thread of the apply kernel partly filled",)),
    _ising_case(256, 7, ("K = 256: threads 0 .. 31 of k_scan_apply own eight items each, the others none; "
                          "every thread of k_scan_tile_totals adds one item",)),
    _ising_case(257, 8, ("K = 257",)),
    _ising_case(2047, 9, ("K = 2047: one item short of a scan tile",)),
    _ising_case(2048, 10, ("K = 2048: exactly one scan tile, out[n] written by its last block",)),
    _ising_case(2049, 11, ("K = 2049: a second tile of one item, tile base from k_scan_totals",)),
    _ising_case(70001, 12, ("K about 70 000 (a production cluster): 35 tiles, 17 probes per bisection",)),
    _ising_case(SCAN_TOTALS_CHUNK + 713, 13, (
        "K > 524288: k_scan_totals takes a second step of 256 tiles and carries (int64_t input)",
        "about one connection per row: row_of bisects half a million offsets"), per_row=1),
)


# ==================================================================================================
# asp_table_index
# ==================================================================================================
def table_index(keys, queries, *, signed=False, insertion_index=False):
    """Position of every query in the strictly ascending ``keys``, -1 when absent."""
    keys = np.asarray(keys, dtype=np.uint64)
    queries = np.asarray(queries, dtype=np.uint64)
    n = keys.shape[0]
    if n == 0:
        return np.full(queries.shape[0], -1, dtype=np.int64)
    if signed:        # WRONG: the keys compared as int64
        at = np.searchsorted(keys.view(np.int64), queries.view(np.int64))
    else:
        at = np.searchsorted(keys, queries)
    found = keys[np.minimum(at, n - 1)] == queries
    if insertion_index:   # WRONG: what np.searchsorted alone gives
        return at.astype(np.int64)
    return np.where(found, at, -1).astype(np.int64)


TABLE_VARIANTS = {
    "signed key comparison": dict(signed=True),
    "insertion index for absent keys": dict(insertion_index=True),
}

TABLE_SIZES = (0, 1, 2, 3, 1000, 300_000)
TABLE_QUERIES = (1, 255, 256, 257)


@dataclass(frozen=True)
class TableInput:
    keys: np.ndarray
    queries: Tuple[np.ndarray, ...]      # one array per entry of TABLE_QUERIES


@functools.lru_cache(maxsize=None)
def make_table(n, seed):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1 << 20, (1 << 64) - (1 << 20), size=n, dtype=np.uint64))
    assert keys.shape[0] == n
    queries = []
    for which, m in enumerate(TABLE_QUERIES):
        q = rng.integers(0, 1 << 64, size=m + 16, dtype=np.uint64)                # between keys
        if n:
            present = rng.random(q.shape[0]) < 0.5
            q[present] = keys[rng.integers(0, n, size=int(present.sum()))]
            special = [keys[0] - np.uint64(1), keys[-1] + np.uint64(1), keys[0], keys[-1],
                       np.uint64(0), U64_MAX, keys[n // 2] + np.uint64(1)]
        else:
            special = [np.uint64(0), U64_MAX, np.uint64(1) << np.uint64(63)]
        # the special probes lead, rotated so that the single query of m = 1 differs from size to size
        special = np.roll(np.array(special, dtype=np.uint64), -(TABLE_SIZES.index(n) + which))
        q[:special.shape[0]] = special
        queries.append(q[:m])
    return TableInput(keys, tuple(queries))


TABLE_CASES = tuple(
    Case("table n=%d" % n, lambda n=n: make_table(n, 100 + n), (
        {0: "n = 0: the bisection never starts and nothing is read",
         1: "n = 1: the loop body never runs", 2: "n = 2: one step", 3: "n = 3: odd split"}.get(
             n, "n = %d: %d probes per query" % (n, int(np.ceil(np.log2(max(n, 2)))))),
        "m = 1, 255, 256, 257: a partly filled, a full and a second workgroup",
        "queries below the first key, above the last, between keys, 0 and 2^64 - 1"))
    for n in TABLE_SIZES)


# ==================================================================================================
# asp_sparsify_component
# ==================================================================================================
def sparsify_keep(matrix, is_frozen, reltol, anchor, *, frozen_pairs_survive=True, link="sum",
                  strict=True, check=True):
    """``keep bool[K]`` as oracle.sparsify_component gives it (tests/test_prep_cases.py asserts
    that on every case); the keyword arguments switch on the WRONG variants.  Raises
    AssertionError when a frozen spin falls outside the anchor's component, unless ``check`` is
    off."""
    full = scipy.sparse.csr_matrix(matrix)
    frozen = np.asarray(is_frozen, dtype=bool)
    rows = np.repeat(np.arange(full.shape[0]), np.diff(full.indptr))
    data = full.data.astype(np.float64)
    if data.size:
        threshold = reltol * np.max(np.abs(data))
        weak = np.abs(data) < threshold if strict else np.abs(data) <= threshold   # WRONG: <=
        if frozen_pairs_survive:       # WRONG without: both ends frozen -> never pruned
            weak &= ~(frozen[rows] & frozen[full.indices])
        data[weak] = 0.0
    pruned = scipy.sparse.csr_matrix((data, full.indices, full.indptr), shape=full.shape)
    if link == "sum":
        graph = 0.5 * (pruned + pruned.transpose())
    else:                              # WRONG: a link whenever either direction survives
        graph = abs(pruned) + abs(pruned).transpose()
    graph = scipy.sparse.csr_matrix(graph)
    graph.eliminate_zeros()
    _, component = connected_components(graph, directed=False)
    if check:
        assert np.all(component[frozen] == component[anchor])
    return component == component[anchor]


SPARSIFY_VARIANTS = {
    "two frozen ends are pruned like any others": dict(frozen_pairs_survive=False),
    "a link whenever either direction survives": dict(link="either"),
    "<= in the cutoff": dict(strict=False),
}


def block_of(matrix, keep):
    """``(indptr, indices, data)`` of the rows and columns ``keep`` of a canonical CSR matrix, stored
    zeros included, columns renumbered — exchange[mask][:, mask] written out."""
    m = scipy.sparse.csr_matrix(matrix)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    live = keep[rows] & keep[m.indices]
    new_index = np.cumsum(keep) - 1
    counts = np.bincount(new_index[rows[live]], minlength=int(keep.sum()))
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return indptr, new_index[m.indices[live]].astype(np.int32), m.data[live]


@dataclass(frozen=True)
class SparsifyInput:
    matrix: scipy.sparse.csr_matrix     # canonical: sorted rows, no duplicates, stored zeros kept
    frozen: np.ndarray
    anchor: int
    reltols: Tuple[float, ...]
    cutting: Tuple[float, ...] = ()     # the reltols at which the case is about the cut


def _csr(k, rows, cols, vals):
    """Canonical CSR from distinct (row, col) pairs; stored zeros stay stored."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])), "duplicate entry"
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=k))])
    m = scipy.sparse.csr_matrix((vals, cols.astype(np.int32), indptr.astype(np.int32)), shape=(k, k))
    m.has_sorted_indices = True
    return m


def _both_ways(pairs, vals):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    vals = np.asarray(vals, dtype=np.float64)
    return (np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]]),
            np.concatenate([vals, vals]))


def frozen_bridges():
    """Twelve islands of eight spins (strong rings), joined in a row by weak couplings only.  The
    first spin of islands 0..5 is frozen and carries the bridge to the next island: bridges 0-1 ..
    4-5 join two frozen spins and survive the cutoff; bridge 5-6 joins a frozen and a free spin,
    bridges 6-7 .. 10-11 two free spins, and are cut.  The candidate frozen spin of island 8 falls
    outside the anchor's component under the correct law and leaves the frozen set."""
    rng = np.random.default_rng(21)
    islands, size = 12, 8
    k = islands * size
    label = rng.permutation(k)                       # spins in random order
    first = [label[i * size] for i in range(islands)]
    pairs, vals = [], []
    for i in range(islands):
        for t in range(size):
            pairs.append((label[i * size + t], label[i * size + (t + 1) % size]))
            vals.append(float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.0)))
    for i in range(islands - 1):
        far = first[i + 1] if i + 1 <= 5 else label[(i + 1) * size + 3]
        near = first[i] if i <= 5 else label[i * size + 5]
        pairs.append((near, far))
        vals.append(float(rng.choice([-1.0, 1.0]) * rng.uniform(1e-6, 1e-5)))
    matrix = _csr(k, *_both_ways(pairs, vals))
    frozen = np.zeros(k, dtype=bool)
    frozen[first[:6] + [first[8]]] = True
    anchor = int(first[0])
    while True:     # drop the frozen spins the correct law leaves outside, until none is
        keep = sparsify_keep(matrix, frozen, 1e-3, anchor, check=False)
        if not np.any(frozen & ~keep):
            break
        frozen &= keep
    return SparsifyInput(matrix, frozen, anchor, (1e-3,), (1e-3,))


PAIR_KINDS = ("(v, -v)", "(v, weak)", "(weak, -weak)", "(v, absent)", "|v| = reltol * max")


def directed_pairs():
    """200 backbone spins in a strong ring, each with one leaf; the leaf's link is of kind
    PAIR_KINDS[i % 5], stored as (M[backbone, leaf], M[leaf, backbone]) or the other way round:
    exact cancellation (no edge), one side pruned (edge), two weak ones that cancel (no edge at
    any reltol), one direction absent (edge) and |v| exactly reltol * max for reltol = 1e-3 and
    0.5 in turn (kept under `<`, so an edge at that reltol).  The diagonal entry of spin 0 is the
    largest element; leaves are joined to each other by stored zeros and one -0.0, which never
    make an edge but belong to the kept block."""
    rng = np.random.default_rng(22)
    m = 200
    k = 2 * m
    label = rng.permutation(k)
    back, leaf = label[:m], label[m:]
    largest = 8.0
    rows, cols, vals = [int(label[0])], [int(label[0])], [largest]
    r, c, v = _both_ways([(back[i], back[(i + 1) % m]) for i in range(m)], rng.uniform(5.0, 7.0, size=m))
    rows += r.tolist(); cols += c.tolist(); vals += v.tolist()
    for i in range(m):
        a, b = (back[i], leaf[i]) if (i // 5) % 2 == 0 else (leaf[i], back[i])
        strong = float(rng.choice([-1.0, 1.0]) * rng.uniform(5.0, 7.0))
        weak = float(rng.uniform(1e-6, 1e-5))
        edge = (1e-3 if (i // 5) % 2 == 0 else 0.5) * largest        # numpy's reltol * max
        forward, backward = {0: (strong, -strong), 1: (strong, weak), 2: (weak, -weak),
                             3: (strong, None), 4: (edge, None if i % 2 else -edge * 0.25)}[i % 5]
        rows.append(int(a)); cols.append(int(b)); vals.append(forward)
        if backward is not None:
            rows.append(int(b)); cols.append(int(a)); vals.append(backward)
    for i in range(m - 1):           # stored zeros between neighbouring leaves, one of them -0.0
        rows.append(int(leaf[i])); cols.append(int(leaf[i + 1])); vals.append(-0.0 if i == 7 else 0.0)
    frozen = np.zeros(k, dtype=bool)
    frozen[back[0]] = True
    return SparsifyInput(_csr(k, rows, cols, vals), frozen, int(back[0]), (0.0, 1e-3, 0.5), (0.0, 1e-3, 0.5))


HUB_DEGREES = (63, 64, 65, 127, 128, 129, 300)


def hub_rows():
    """Seven hubs whose rows hold exactly 63 .. 300 non-zeros: each hub has its own leaves, in random
    index order, and nothing else.  A leaf is tied strongly or weakly in an irregular pattern, so
    that every 64-lane chunk of a hub's row keeps a different number of columns.  The hubs hang
    together through leaves: the first leaf of a hub is tied strongly to the second leaf of the
    next one (both strongly tied to their hubs), so no hub's row grows.  At reltol 0 everything is
    kept: full ballots."""
    rng = np.random.default_rng(23)
    k = len(HUB_DEGREES) + sum(HUB_DEGREES)
    label = rng.permutation(k)
    hubs = label[:len(HUB_DEGREES)]
    pairs, vals, linking = [], [], []
    at = len(hubs)
    for h, degree in zip(hubs, HUB_DEGREES):
        leaves = label[at:at + degree]
        at += degree
        strong = rng.random(degree) < 0.6
        strong[:2] = True
        linking.append((leaves[0], leaves[1]))
        for leaf, s in zip(leaves, strong):
            pairs.append((h, leaf))
            vals.append(float(rng.choice([-1.0, 1.0]) * (rng.uniform(0.5, 2.0) if s else rng.uniform(1e-5, 1e-4))))
    for (out, _), (_, into) in zip(linking[:-1], linking[1:]):
        pairs.append((out, into))
        vals.append(float(rng.uniform(1.0, 2.0)))
    frozen = np.zeros(k, dtype=bool)
    frozen[hubs[0]] = True
    return SparsifyInput(_csr(k, *_both_ways(pairs, vals)), frozen, int(hubs[0]), (0.0, 1e-3))


def tile_edge(k):
    """A strong ring over the spins i with i % 3 != 2; every spin with i % 3 == 2 hangs on its
    predecessor by a weak coupling.  At reltol 1e-3 two thirds are kept (the scan of
    `keep` adds zeros and ones up to the last item), at reltol 0 all K are (the scan of the kept
    rows' lengths then runs over K items as well)."""
    rng = np.random.default_rng(1000 + k)
    if k == 1:
        return SparsifyInput(_csr(1, [0], [0], [-1.5]), np.array([True]), 0, (0.0, 1e-3))
    ring = np.array([i for i in range(k) if i % 3 != 2])
    pairs = [(ring[i], ring[i + 1]) for i in range(len(ring) - 1)]
    if len(ring) > 2:
        pairs.append((ring[-1], ring[0]))
    vals = (rng.choice([-1.0, 1.0], size=len(pairs)) * rng.uniform(0.5, 1.0, size=len(pairs))).tolist()
    for i in range(2, k, 3):
        pairs.append((i - 1, i))
        vals.append(float(rng.uniform(1e-5, 1e-4)))
    frozen = np.zeros(k, dtype=bool)
    frozen[0] = True
    return SparsifyInput(_csr(k, *_both_ways(pairs, vals)), frozen, 0, (0.0, 1e-3))


LARGE_K = SCAN_TOTALS_CHUNK + 5712      # 530 000


def large():
    """530 000 spins in a random recursive tree (spin i hangs on a random earlier spin: depth about
    2 ln K, shallow) plus K / 4 random chords, stored both ways: 1.3 million non-zeros.  One link in
    three is weak.  The largest element is the fourth from the end of `data`.  At reltol 0 every
    spin is kept (K > 524288: both scans carry across chunks of 256 tiles); at 1e-2 the weak links
    cut the tree."""
    rng = np.random.default_rng(24)
    k = LARGE_K
    child = np.arange(1, k)
    parent = (rng.random(k - 1) * child).astype(np.int64)
    a = rng.integers(0, k, size=k // 4)
    b = rng.integers(0, k, size=k // 4)
    lo, hi = np.concatenate([parent, np.minimum(a, b)]), np.concatenate([child, np.maximum(a, b)])
    code = np.unique(lo[lo != hi] * k + hi[lo != hi])
    lo, hi = code // k, code % k
    vals = rng.choice([-1.0, 1.0], size=lo.shape[0]) * rng.uniform(0.5, 1.0, size=lo.shape[0])
    weak = rng.random(lo.shape[0]) < 1.0 / 3.0
    vals[weak] *= 1e-4
    matrix = _csr(k, *_both_ways(np.stack([lo, hi], axis=1), vals))
    matrix.data[-4] = -2.0
    frozen = np.zeros(k, dtype=bool)
    frozen[0] = True
    return SparsifyInput(matrix, frozen, 0, (0.0, 1e-2), (1e-2,))


def _cached(fn, *args):
    return lambda: _sparsify_input(fn, args)


@functools.lru_cache(maxsize=None)
def _sparsify_input(fn, args):
    return fn(*args)


SPARSIFY_CASES = (
    Case("frozen bridges", _cached(frozen_bridges), (
        "pruned(): both ends frozen, so the coupling is never pruned",
        "pruned(): one end frozen is pruned like any other")),
    Case("directed pairs", _cached(directed_pairs), (
        "k_hook_edges: 0.5 * (M'_ij + M'_ji) cancels to zero with both directions alive",
        "pruned_transposed(): element absent; element present but pruned",
        "pruned(): |v| == threshold is kept (`<`)",
        "k_abs_max: the maximum on the diagonal; -0.0 and stored zeros in the block")),
    Case("hub rows", _cached(hub_rows), (
        "k_hook_edges, k_slice_rows: a second, third .. fifth 64-lane step of the row loop",
        "k_slice_rows<emit>: `out += here` across chunks that each keep a different count",
        "rows of exactly 63, 64, 65, 127, 128, 129 and 300 non-zeros: a last chunk of 63 lanes, full "
        "chunks after which the loop must stop (64, 128), one lane after one and after two full chunks")),
) + tuple(
    Case("tile edge K=%d" % k, _cached(tile_edge, k), (
        "exclusive_scan<uint32_t> over %d items of `keep` and over the kept rows' lengths" % k,))
    for k in (1, 2, 2047, 2048, 2049, 4097)
) + (
    Case("large", _cached(large), (
        "k_scan_totals with more than 256 tiles (uint32_t input): keep (530 000) and row lengths",
        "k_abs_max: a second grid-stride step, the maximum found in it",
        "union-find over half a million spins, hub-free and shallow")),
)


@functools.lru_cache(maxsize=None)
def _sparsify_oracle(name, reltol):
    import oracle

    case = {c.name: c for c in SPARSIFY_CASES}[name].make()
    keep, block = oracle.sparsify_component(case.matrix, case.frozen, reltol, case.anchor)
    block = scipy.sparse.csr_matrix(block)
    block.sort_indices()
    return keep, block


def sparsify_oracle(case, reltol):
    """oracle.sparsify_component on the case: ``(keep, block with sorted indices)``, computed on
    first use, shared by every test, never modified."""
    return _sparsify_oracle(case.name, float(reltol))
