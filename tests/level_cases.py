"""The cases of tests/test_level_cases.py and tests/test_gpu_level_batch.py: the cutoff and the extension of many
clusters in one call, specifications ASP-SPARSIFY-SEG-1 and ASP-EXTEND-SEG-1 (DESIGN.md §3.9, §3.10;
csrc/level_segments.hip), and their sequential numpy laws.

A helper module like tests/ising_segment_cases.py: no fixtures, no files, nothing compiled, no GPU.  The sparsify
tables are concatenations of tests/prep_cases.py inputs (never "large"), the law is prep_cases.sparsify_keep /
block_of segment by segment; the extend tables come from tests/eloc_cases.py and tests/operator_cases.py, the law
is operator_cases.extend (in a symmetry sector: the representatives of the raw targets, without the orbits of norm
0) segment by segment.  The keyword arguments of the laws switch on the WRONG variants.  A case and its law are
computed once and shared.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import scipy.sparse
from scipy.sparse.csgraph import connected_components

import eloc_cases
import operator_cases
import prep_cases
from field_cases import grow, model_operator
from symmetry_cases import plain_twin

U64 = np.uint64
ROWS_PER_BLOCK = 4            # kWaves of level_segments.hip: one wavefront per row
SCAN_TILE = prep_cases.SCAN_TILE


# ==================================================================================================
# asp_sparsify_component_segments
# ==================================================================================================
@dataclass(frozen=True)
class Segment:
    matrix: object           # canonical csr_matrix (n x n) or None for an empty segment
    frozen: np.ndarray       # bool[n]
    anchor: int              # local

    @property
    def size(self):
        return 0 if self.matrix is None else self.matrix.shape[0]


EMPTY = Segment(None, np.zeros(0, dtype=bool), 0)


@dataclass
class SparsifyTable:
    name: str
    segments: Tuple[Segment, ...]
    reltol: float
    offsets: np.ndarray      # u64[G + 1]
    indptr: np.ndarray       # i64[T + 1], global
    indices: np.ndarray      # i32, segment-local
    data: np.ndarray         # f64
    frozen: np.ndarray       # bool[T]
    anchors: np.ndarray      # u64[G]

    def law(self, **switches):
        return _shared_sparsify_law(self.name) if not switches else sparsify_segments_law(self, **switches)


def table_of(name, segments, reltol):
    segments = tuple(segments)
    sizes = [s.size for s in segments]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(U64)
    indptr, base = [np.zeros(1, dtype=np.int64)], 0
    for s in segments:
        if s.size:
            assert s.matrix.has_sorted_indices
            indptr.append(s.matrix.indptr[1:].astype(np.int64) + base)
            base += int(s.matrix.indptr[-1])
    live = [s for s in segments if s.size]
    indices = np.concatenate([s.matrix.indices for s in live]).astype(np.int32) if live else np.zeros(0, np.int32)
    data = np.concatenate([s.matrix.data for s in live]).astype(np.float64) if live else np.zeros(0)
    frozen = np.concatenate([s.frozen for s in segments]).astype(bool) if segments else np.zeros(0, dtype=bool)
    return SparsifyTable(name, segments, float(reltol), offsets, np.concatenate(indptr), indices, data, frozen,
                         np.array([s.anchor for s in segments], dtype=U64))


def keep_with_threshold(matrix, frozen, threshold, anchor):
    """prep_cases.sparsify_keep with the threshold handed in (tests/test_level_cases.py asserts that they agree
    at `reltol * max|data|`): what the WRONG variant with one threshold for the whole table needs."""
    full = scipy.sparse.csr_matrix(matrix)
    rows = np.repeat(np.arange(full.shape[0]), np.diff(full.indptr))
    data = full.data.astype(np.float64)
    weak = (np.abs(data) < threshold) & ~(frozen[rows] & frozen[full.indices])
    data[weak] = 0.0
    pruned = scipy.sparse.csr_matrix((data, full.indices, full.indptr), shape=full.shape)
    graph = scipy.sparse.csr_matrix(0.5 * (pruned + pruned.transpose()))
    graph.eliminate_zeros()
    _, component = connected_components(graph, directed=False)
    return component == component[anchor]


class Stray(AssertionError):
    """A frozen spin outside its anchor's component: `segment` (None: the check was made table-wide), `count`."""

    def __init__(self, segment, count):
        super().__init__("segment {}: {} stray frozen spins".format(segment, count))
        self.segment, self.count = segment, count


def sparsify_segments_law(table, *, shared_threshold=False, global_anchor=False, table_columns=False,
                          table_wide_stray=False):
    """``(keep bool[T], kept_offsets u64[G + 1], out_indptr i64, out_indices i32, out_data f64)`` of
    ASP-SPARSIFY-SEG-1, segment by segment; raises :class:`Stray`.  The keyword arguments switch on the WRONG
    variants."""
    whole_max = float(np.max(np.abs(table.data))) if table.data.size else 0.0
    keeps, blocks, strays = [], [], []
    for g, s in enumerate(table.segments):
        if s.size == 0:
            keeps.append(np.zeros(0, dtype=bool))
            blocks.append((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)))
            strays.append(0)
            continue
        if shared_threshold:           # WRONG: reltol * max|data of the TABLE|
            keep = keep_with_threshold(s.matrix, s.frozen, table.reltol * whole_max, s.anchor)
        else:
            keep = prep_cases.sparsify_keep(s.matrix, s.frozen, table.reltol, s.anchor, check=False)
        if global_anchor:              # WRONG: anchors[g] read as an index into the table
            first, last = int(table.offsets[g]), int(table.offsets[g + 1])
            if not first <= s.anchor < last:
                keep = np.zeros(s.size, dtype=bool)   # the anchor's component lies in another segment
            elif first:
                keep = prep_cases.sparsify_keep(s.matrix, s.frozen, table.reltol, s.anchor - first, check=False)
        keeps.append(keep)
        strays.append(int(np.count_nonzero(s.frozen & ~keep)))
        blocks.append(prep_cases.block_of(s.matrix, keep))
    if table_wide_stray and sum(strays):   # WRONG: one counter for the table
        raise Stray(None, sum(strays))
    for g, count in enumerate(strays):
        if count:
            raise Stray(g, count)
    kept_offsets = np.concatenate([[0], np.cumsum([int(k.sum()) for k in keeps])]).astype(U64)
    out_indptr, base = [np.zeros(1, dtype=np.int64)], 0
    for ip, _, _ in blocks:
        out_indptr.append(ip[1:].astype(np.int64) + base)
        base += int(ip[-1])
    columns = [c.astype(np.int64) + (int(kept_offsets[g]) if table_columns else 0)   # WRONG: table-wide numbering
               for g, (_, c, _) in enumerate(blocks)]
    return (np.concatenate(keeps) if keeps else np.zeros(0, dtype=bool), kept_offsets, np.concatenate(out_indptr),
            np.concatenate(columns).astype(np.int32) if columns else np.zeros(0, np.int32),
            np.concatenate([v for _, _, v in blocks]) if blocks else np.zeros(0))


SPARSIFY_VARIANTS = {
    "one threshold for the table": dict(shared_threshold=True),
    "the anchor read as a global index": dict(global_anchor=True),
    "columns renumbered over the table": dict(table_columns=True),
    "the stray-frozen check made table-wide": dict(table_wide_stray=True),
}


def rebased(result, offsets, g):
    """Segment g of a law's or a call's result: ``(keep_g, indptr, indices, data)`` of its own."""
    keep, kept_offsets, out_indptr, out_indices, out_data = result
    first, last = int(kept_offsets[g]), int(kept_offsets[g + 1])
    begin, end = int(out_indptr[first]), int(out_indptr[last])
    return (keep[int(offsets[g]):int(offsets[g + 1])], out_indptr[first:last + 1] - begin, out_indices[begin:end],
            out_data[begin:end])


def same_result(got, want):
    """Integers equal, the doubles as bytes."""
    return bool(all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[:4], want[:4]))
                and np.asarray(got[4], dtype=np.float64).tobytes() == np.asarray(want[4], dtype=np.float64).tobytes())


def _of(inp):
    return Segment(inp.matrix, inp.frozen, inp.anchor)


def _prep(name):
    return {c.name: c for c in prep_cases.SPARSIFY_CASES}[name].make()


def _scaled(inp, factor):
    m = inp.matrix.copy()
    m.data = m.data * factor      # a power of two: every product, comparison and sum scales exactly
    m.has_sorted_indices = True
    return Segment(m, inp.frozen, inp.anchor)


SCALED = ("directed pairs", "frozen bridges", "hub rows", "tile edge K=2049")
SCALES = (2.0 ** -30, 1.0, 2.0 ** 30)


def _scaled_copies(name):
    inp = _prep(name)
    return table_of("scaled: " + name, [_scaled(inp, f) for f in SCALES], 1e-3)


def _tile(k):
    return _of(prep_cases.tile_edge(k)) if k else EMPTY


SIZES = (0, 1, 2, 3, 63, 64, 65, 257)


def _sizes():
    """Segments of 0 ... 257 spins, empty ones first, in the middle (two in a row) and last."""
    return table_of("sizes 0 1 2 3 63 64 65 257", [_tile(k) for k in (0, 1, 2, 3, 0, 0, 63, 64, 65, 257, 0)], 1e-3)


WORKGROUP_SIZES = (1, 2, 3, 2, 3, 1, 4, 3)


def _workgroup_boundaries():
    """Boundaries at rows 1, 3, 6, 8, 11, 12, 16: at 1, 2, 3 and 0 modulo the four rows of a workgroup."""
    return table_of("boundaries in a workgroup", [_tile(k) for k in WORKGROUP_SIZES], 1e-3)


def _scan_tile_boundaries():
    """Boundaries at 2047, 2048 and 2049 of the device scan's tile; the cut keeps two spins in three."""
    return table_of("boundaries at the scan tile", [_tile(2047), _tile(1), _tile(1), _tile(65)], 1e-3)


def _many_small():
    return table_of("4097 segments of 1-3 spins", [_tile(1 + g % 3) for g in range(4097)], 1e-3)


def _two_anchors():
    """The frozen-bridges matrix twice: with its own frozen spins and anchor, and with one free spin of a part
    that the cutoff separates as the anchor and the only frozen spin."""
    inp = _prep("frozen bridges")
    keep = prep_cases.sparsify_keep(inp.matrix, inp.frozen, 1e-3, inp.anchor)
    other = int(np.nonzero(~keep)[0][5])
    frozen = np.zeros_like(inp.frozen)
    frozen[other] = True
    return table_of("one matrix, two anchors", [_of(inp), Segment(inp.matrix, frozen, other)], 1e-3)


def _no_couplings():
    """A segment without non-zeros (threshold reltol * 0) whose only frozen spin is the anchor, between two others."""
    none = scipy.sparse.csr_matrix((5, 5), dtype=np.float64)
    none.has_sorted_indices = True
    frozen = np.zeros(5, dtype=bool)
    frozen[2] = True
    zeros = prep_cases._csr(3, [0, 1, 1, 2], [1, 0, 2, 1], [0.0, 0.0, -0.0, 0.0])   # stored zeros only
    return table_of("no non-zeros", [_tile(3), Segment(none, frozen, 2), Segment(zeros, np.array([True, False, False]), 0),
                                     _tile(2)], 1e-3)


def _all_cut():
    """Everything but the anchor is cut: the anchor's diagonal element is the maximum, its couplings are weak."""
    k = 70
    rows, cols, vals = prep_cases._both_ways([(0, j) for j in range(1, k)], np.full(k - 1, 1e-6))
    m = prep_cases._csr(k, np.concatenate([[0], rows]), np.concatenate([[0], cols]), np.concatenate([[8.0], vals]))
    frozen = np.zeros(k, dtype=bool)
    frozen[0] = True
    return table_of("all but the anchor cut", [_tile(3), Segment(m, frozen, 0), _tile(2)], 1e-3)


def _stray():
    """Three copies of the frozen bridges; in the second ONE free spin outside the anchor's component is frozen
    again, in the third two are: the first such segment is 1 and its count 1, the table's count 3."""
    inp = _prep("frozen bridges")
    keep = prep_cases.sparsify_keep(inp.matrix, inp.frozen, 1e-3, inp.anchor)
    outside = np.nonzero(~keep)[0]
    one, two = inp.frozen.copy(), inp.frozen.copy()
    one[outside[3]] = True
    two[outside[[1, 9]]] = True
    return table_of("stray frozen spins", [_of(inp), Segment(inp.matrix, one, inp.anchor),
                                           Segment(inp.matrix, two, inp.anchor)], 1e-3)


SPARSIFY_BUILDERS = {"scaled: " + name: functools.partial(_scaled_copies, name) for name in SCALED}
SPARSIFY_BUILDERS.update({
    "sizes 0 1 2 3 63 64 65 257": _sizes,
    "boundaries in a workgroup": _workgroup_boundaries,
    "boundaries at the scan tile": _scan_tile_boundaries,
    "4097 segments of 1-3 spins": _many_small,
    "one matrix, two anchors": _two_anchors,
    "no non-zeros": _no_couplings,
    "all but the anchor cut": _all_cut,
})
SPARSIFY_NAMES = tuple(SPARSIFY_BUILDERS)
STRAY = "stray frozen spins"          # no result: the call is refused
SPARSIFY_BUILDERS[STRAY] = _stray


@functools.lru_cache(maxsize=None)
def sparsify_table(name):
    t = SPARSIFY_BUILDERS[name]()
    assert t.name == name
    return t


@functools.lru_cache(maxsize=None)
def _shared_sparsify_law(name):
    return sparsify_segments_law(sparsify_table(name))


# ==================================================================================================
# asp_operator_extend_segments
# ==================================================================================================
@dataclass
class ExtendTable:
    name: str
    operator: object
    keys: np.ndarray         # u64[T]: the segments one after the other, any order, repeats allowed
    offsets: np.ndarray      # u64[G + 1]

    def law(self, **switches):
        return _shared_extend_law(self.name) if not switches else extend_segments_law(self, **switches)

    @property
    def segments(self):
        return self.offsets.size - 1

    def segment(self, g):
        return self.keys[int(self.offsets[g]):int(self.offsets[g + 1])]


def no_state(op):
    """What stands for a target of norm 0 before the sort: all sites up."""
    n = op.basis.number_spins
    return U64((1 << n) - 1)


def drops(op):
    group = getattr(op.basis, "group", None)
    return group is not None and group.spin_inversion < 0


def targets(op, keys):
    """Every target of every key, in connection order, repeats kept; in a symmetry sector the representatives,
    a target of norm 0 as :func:`no_state`."""
    raw = operator_cases.action(plain_twin(op), keys)[0]
    group = getattr(op.basis, "group", None)
    if group is None or raw.size == 0:
        return raw
    rep, _, norm = group.state_info(raw)
    return np.where(norm > 0, rep, no_state(op)).astype(U64)


def extend_one(op, keys):
    """asp_operator_extend's law for one key set: operator_cases.extend, in a sector on the representatives."""
    keys = np.asarray(keys, dtype=U64)
    if getattr(op.basis, "group", None) is None:
        return operator_cases.extend(op, keys, op.basis.number_spins)
    out = np.unique(targets(op, keys))
    return out[out != no_state(op)] if drops(op) else out


def extend_segments_law(table, *, flag_across_boundary=False, one_sort=False, dropped_at_table_end=False):
    """``(states u64, out_offsets u64[G + 1])`` of ASP-EXTEND-SEG-1 as the device computes it: the targets of every
    segment sorted, the first of every run flagged — a segment's first connection always —, the "no state" value
    left out, the flags counted per segment.  The keyword arguments switch on the WRONG variants."""
    op = table.operator
    lists = [targets(op, table.segment(g)) for g in range(table.segments)]
    sizes = np.array([x.size for x in lists], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    if one_sort:                       # WRONG: one sort over the table, cut at the connection offsets
        cat = np.sort(np.concatenate(lists)) if lists else np.zeros(0, U64)
    else:
        cat = np.concatenate([np.sort(x) for x in lists]) if lists else np.zeros(0, U64)
    first = np.ones(cat.size, dtype=bool)
    first[1:] = cat[1:] != cat[:-1]
    if not flag_across_boundary:       # WRONG without: a repeat of the PREVIOUS segment's last state is dropped
        first[starts[:-1][sizes > 0]] = True
    gone = np.zeros(cat.size, dtype=bool)
    if drops(op):
        gone = cat == no_state(op)
        if dropped_at_table_end:       # WRONG: only the run at the table's end is left out
            tail = cat.size
            while tail > 0 and gone[tail - 1]:
                tail -= 1
            gone[:tail] = False
    flag = first & ~gone
    position = np.concatenate([[0], np.cumsum(flag)])
    return cat[flag], position[starts].astype(U64)


EXTEND_VARIANTS = {
    "the first-flag looks across a boundary": dict(flag_across_boundary=True),
    "one sort over the table": dict(one_sort=True),
    "norm 0 dropped only at the table's end": dict(dropped_at_table_end=True),
}


def same_extension(got, want):
    return bool(np.array_equal(np.asarray(got[0], dtype=U64), want[0])
                and np.array_equal(np.asarray(got[1], dtype=U64), want[1]))


def _cut(name, op, segments):
    segments = [np.asarray(s, dtype=U64) for s in segments]
    offsets = np.concatenate([[0], np.cumsum([s.size for s in segments])]).astype(U64)
    return ExtendTable(name, op, np.concatenate(segments) if segments else np.zeros(0, U64), offsets)


def _from_eloc(name):
    t = eloc_cases.table(name)
    return ExtendTable(name, t.operator, t.keys, t.offsets)


def _key_counts():
    """Segments of 0, 1, 2, 63, 64 and 65 kagome16 keys, each shuffled, one key in four twice."""
    op, _ = eloc_cases.kagome16_basis()
    rng = np.random.default_rng(65)
    whole = grow(op, 200, 66)
    segments, at = [], 0
    for n in (0, 1, 2, 63, 0, 64, 65):
        own = whole[at:at + n]
        at += n
        segments.append(rng.permutation(np.concatenate([own, own[::4]])) if n > 2 else own)
    return _cut("segments of 0 1 2 63 64 65 keys", op, segments)


def _same_single_key():
    """Neighbouring segments that hold the same single key, whose only target is itself (all sites down on the
    exchange ring): the last sorted target of one segment EQUALS the first of the next, which is no repeat.  Then
    an empty segment, the key twice in one segment, and a key with neighbours."""
    op = operator_cases.ring(16, 400)
    key = np.zeros(1, dtype=U64)
    return _cut("two segments with the same single key", op, [key, key, np.zeros(0, U64), key, np.concatenate([key, key]),
                                                             np.array([5], dtype=U64)])


def _unsorted():
    x = operator_cases.extension_unsorted()
    keys = x.extend_keys
    return _cut("unsorted with repeats", x.operator, [keys[:120], keys[120:121], keys[121:]])


def _kagome18_minus():
    """kagome_18 in the sector with inversion -1 (the dropping pass is on; these clusters reach no orbit of norm 0)."""
    op = model_operator("heisenberg_kagome_18", -1)
    return _cut("kagome18 inversion -1, four clusters", op, [grow(op, 40, 19), grow(op, 7, 20), grow(op, 65, 21),
                                                           grow(op, 1, 22)])


def _ring22_minus():
    """The 22-site ring in the sector with inversion -1, whose connections DO reach orbits of norm 0: the "no
    state" value ends up at the end of the sorted targets of the first three segments, and not of the last."""
    import symmetry_cases

    e = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    k = e.keys
    return _cut("ring22 inversion -1, norm-0 targets", e.operator, [k[:20], k[20:27], k[27:60][::-1], k[60:61]])


def _ring64():
    """64 sites, keys with bit 63 set and clear: no segment number fits above the key.  Overlapping segments, one
    of them descending."""
    t = eloc_cases.table("ring64 bit 63")
    return _cut("ring64 bit 63", t.operator, [t.keys[:20], t.keys[10:][::-1], t.keys[-1:], t.keys[5:8]])


EXTEND_BUILDERS = {
    "segments of 0 1 2 63 64 65 keys": _key_counts,
    "unsorted with repeats": _unsorted,
    "two segments with the same single key": _same_single_key,
    "ring64 bit 63": _ring64,
    "4097 segments of 1-3 keys": functools.partial(_from_eloc, "4097 segments of 1-3 keys"),
    "empty segments": functools.partial(_from_eloc, "empty segments"),
    "kagome18 inversion -1, four clusters": _kagome18_minus,
    "ring22 inversion -1, norm-0 targets": _ring22_minus,
    "kagome18 inversion +1": functools.partial(_from_eloc, "kagome18 inversion +1"),
    "single-site flips": functools.partial(_from_eloc, "single-site flips"),
}
EXTEND_NAMES = tuple(EXTEND_BUILDERS)


@functools.lru_cache(maxsize=None)
def extend_table(name):
    t = EXTEND_BUILDERS[name]()
    t.name = name
    return t


@functools.lru_cache(maxsize=None)
def _shared_extend_law(name):
    return extend_segments_law(extend_table(name))
