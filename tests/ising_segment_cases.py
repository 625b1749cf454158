"""The cases of tests/test_ising_segment_cases.py and tests/test_gpu_ising_segments.py: the coupling build of many
clusters in one call, specification ASP-ISING-SEG-1 (csrc/operator_ising_segments.hip), and its law.

A helper module like tests/eloc_cases.py, whose segmented tables and operators it uses: no fixtures, no files,
nothing compiled, no GPU.  The law is, per segment, `helpers.reference_route_ising` — the reference's own numpy/scipy
arithmetic on the host action — as canonical CSR, concatenated as the specification says: ONE global indptr from 0,
columns local to their segment.  A case and its law are computed once and shared.
"""
import functools
from dataclasses import dataclass

import numpy as np

import eloc_cases
from field_cases import awkward_amplitudes, grow, model_operator, same_bits
from helpers import random_operator, reference_route_ising

__all__ = ["awkward_amplitudes", "model_operator", "same_bits"]


# -- the law -------------------------------------------------------------------------------------------------
def segment_csr(op, keys, psi):
    """`(indptr i64[n + 1], col i32, val f64)` of one cluster: make_ising_model's J as canonical CSR."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.size == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    m = reference_route_ising(op, keys, np.ascontiguousarray(psi, dtype=np.float64))  # COO sorted by (row, col)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(m.row, minlength=keys.size))]).astype(np.int64)
    return indptr, m.col.astype(np.int32), np.ascontiguousarray(m.data, dtype=np.float64)


def concatenate(parts, sizes):
    """The per-segment CSR arrays as the specification lays them out: `indptr` global over all rows."""
    indptr = np.zeros(int(np.sum(sizes, dtype=np.int64)) + 1, dtype=np.int64)
    at, base = 0, 0
    for (ip, _, _), n in zip(parts, sizes):
        assert ip.shape == (n + 1,) and ip[0] == 0
        indptr[at:at + n + 1] = base + ip
        at, base = at + n, base + int(ip[-1])
    col = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int32)
    val = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=np.float64)
    return indptr, col.astype(np.int32), val.astype(np.float64)


def rebased(indptr, col, val, offsets, g):
    """Segment g of a concatenated result, as a CSR of its own."""
    first, last = int(offsets[g]), int(offsets[g + 1])
    begin, end = int(indptr[first]), int(indptr[last])
    return indptr[first:last + 1] - begin, col[begin:end], val[begin:end]


def ising_segments_law(op, keys, psi, offsets):
    offsets = np.asarray(offsets).astype(np.int64)
    parts = [segment_csr(op, keys[offsets[g]:offsets[g + 1]], psi[offsets[g]:offsets[g + 1]])
             for g in range(offsets.size - 1)]
    return concatenate(parts, np.diff(offsets))


def equal(got, want):
    """Indices equal, values as bits."""
    return bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2]))


# -- cases ---------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    operator: object
    keys: np.ndarray     # u64[T]: the segments one after the other, each ascending and unique
    psi: np.ndarray      # f64[T]: signed, unit norm over every non-empty segment
    offsets: np.ndarray  # u64[S + 1]

    def law(self, psi=None):
        if psi is None:
            return _shared_law(self.name)
        return ising_segments_law(self.operator, self.keys, psi, self.offsets)

    @property
    def segments(self):
        return self.offsets.size - 1


def normalised(psi, offsets):
    """Every segment's amplitudes divided by the segment's norm (what make_ising_model does per cluster)."""
    psi = np.array(psi, dtype=np.float64)
    for g in range(offsets.size - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        if hi > lo:
            psi[lo:hi] /= np.linalg.norm(psi[lo:hi])
    return psi


def _from_table(name):
    t = eloc_cases.table(name)
    return Case(name, t.operator, t.keys, normalised(t.phi, t.offsets), t.offsets)


def from_segments(name, op, segments, seed):
    t = eloc_cases.from_segments(name, op, segments, [], seed)
    return Case(name, op, t.keys, normalised(t.phi, t.offsets), t.offsets)


def _grown(count):
    """One connected cluster of `count` kagome16 states (the first seed whose cluster has a coupling: a single
    state's diagonal element can be 0)."""
    op, _ = eloc_cases.kagome16_basis()
    for seed in range(1000 + count, 1010 + count):
        c = from_segments("kagome16 grown K=%d" % count, op, [grow(op, count, seed)], count)
        if segment_csr(op, c.keys, c.psi)[2].size:
            return c
    raise AssertionError("no cluster with a coupling")


def _boundaries_in_a_workgroup():
    """Segments of 2, 3 and 5 keys (twice): their boundaries fall inside a workgroup of four rows."""
    op, _ = eloc_cases.kagome16_basis()
    whole = grow(op, 40, 77)
    return from_segments("segments of 2 3 5", op, [whole[:2], whole[2:5], whole[5:10], whole[11:13], whole[13:16],
                                                   whole[20:25]], 79)


def _one_way(kind):
    """An operator with m[dst][src] != 0 == m[src][dst]: a single key, an empty segment, then the cluster."""
    op, keys, _ = random_operator(11 if kind == "one_way" else 12, kind, number_spins=14, num_bonds=20, num_keys=120)
    return from_segments("one-directional, " + kind, op, [keys[:1], np.zeros(0, dtype=np.uint64), keys], 83)


WIDE_BONDS = 7


def _wide_rows():
    """Seven disjoint bonds whose only off-diagonal elements lead INTO the bond state 00 (m[0][src] != 0 ==
    m[src][0]): every row reaches at most one state per bond, so max_connections is 1 + 7, yet the row of the
    state 0 is reached from three states per bond and holds 1 + 21 couplings.  Rows reach distinct states (the
    bonds share no site).  Segments: the state 0 with everything that reaches it, and a part of it."""
    from annealing_sign_problem_amd import operators

    rng = np.random.default_rng(97)
    terms = []
    for b in range(WIDE_BONDS):
        m = np.zeros((4, 4))
        m[np.diag_indices(4)] = rng.normal(size=4)
        m[0, 1:] = rng.normal(size=3)
        terms.append(operators.Term(m, [(2 * b, 2 * b + 1)]))
    op = operators.Operator(operators.SpinBasis(2 * WIDE_BONDS), terms)
    near = sorted({0} | {x << (2 * b) for b in range(WIDE_BONDS) for x in (1, 2, 3)})
    far = sorted(set(near) | {(1 << (2 * b)) | (2 << (2 * c)) for b in range(3) for c in range(3, 6)})
    return from_segments("one-directional, wide rows", op, [near, near[:9], far], 89)


SIZES = (1, 2, 3, 5, 63, 64, 65, 301, 4097)
TABLES = ("kagome16 24 bonds", "j1j2 64 bonds", "sk16 first 65 bonds", "sk16 120 bonds", "ring64 bit 63",
          "ring4 full basis", "sk16 one row of 65 connections", "4097 segments of 1-3 keys", "empty segments",
          "one state in 300 segments", "three segments")
LISTED = eloc_cases.LISTED  # the duplicate-keeping variant: symmetry-adapted bases, single-site flips
BUILDERS = {name: functools.partial(_from_table, name) for name in TABLES + LISTED}
BUILDERS.update({"kagome16 grown K=%d" % k: functools.partial(_grown, k) for k in SIZES})
BUILDERS["segments of 2 3 5"] = _boundaries_in_a_workgroup
BUILDERS["one-directional, one_way"] = functools.partial(_one_way, "one_way")
BUILDERS["one-directional, wide rows"] = _wide_rows
PLAIN = tuple(name for name in BUILDERS if name not in LISTED)
NAMES = PLAIN + LISTED
# refused by the duplicate-keeping variant (no law on the device): not in NAMES
ONE_WAY_WITH_DUPLICATES = "one-directional, single_flip"
BUILDERS[ONE_WAY_WITH_DUPLICATES] = functools.partial(_one_way, "single_flip")


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.name = name
    return c


@functools.lru_cache(maxsize=None)
def _shared_law(name):
    c = case(name)
    return ising_segments_law(c.operator, c.keys, c.psi, c.offsets)


# -- the stored output of the reference function -------------------------------------------------------------------
GOLDEN = {"make_ising_kagome16_cluster.npz": lambda: model_operator("heisenberg_kagome_16"),
          "make_ising_sk16_cluster.npz": lambda: model_operator("sk_16_1"),
          "make_ising_ring4.npz": lambda: eloc_cases.plain_ring(4, 2)}


def golden_cluster(g):
    """`(keys, psi)` of a stored make_ising_model call: the amplitudes normalised as the function does."""
    from annealing_sign_problem_amd import common

    psi = np.ascontiguousarray(np.exp(g["log_psi"]).real)
    psi /= common.norm2(psi)
    return np.ascontiguousarray(g["spins"], dtype=np.uint64), psi
