"""The cases of tests/test_eloc_cases.py and tests/test_gpu_local_energy.py: local energies of signed amplitudes
over segmented tables, specification ASP-ELOC-1 (csrc/operator_local_energy.hip), and its
sequential restatement `eloc_law`.

A helper module like tests/field_cases.py, whose operator and cluster builders it uses: no fixtures, no files,
nothing compiled, no GPU.  The connections of a case come from the host `Operator.batched_apply` (the device action
equals it bit for bit: tests/test_gpu_operator.py, tests/test_gpu_symmetry_edges.py); a case and its law are computed
once and shared.
"""
import functools
from dataclasses import dataclass

import numpy as np

from field_cases import (awkward_amplitudes, case as field_case, first_bonds, grow, model_operator, num_bonds,
                         plain_ring, positions, same_bits)

__all__ = ["awkward_amplitudes", "first_bonds", "model_operator", "num_bonds", "plain_ring", "positions", "same_bits"]


# -- the law -------------------------------------------------------------------------------------------------
def connections(op, row_keys):
    """The host action on the distinct row keys: `(inverse, targets u64[M], coeffs f64[M], starts i64[U + 1])`,
    row r's entries at `starts[inverse[r]] ... starts[inverse[r] + 1]`, the diagonal entry first."""
    unique, inverse = np.unique(np.asarray(row_keys, dtype=np.uint64), return_inverse=True)
    other, coeffs, counts = op.batched_apply(unique)
    assert not np.any(coeffs.imag)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return inverse.reshape(-1), np.ascontiguousarray(other[:, 0]), np.ascontiguousarray(coeffs.real), starts


def segment_of(offsets, at):
    """The segment whose range holds table entry `at` (empty segments are skipped by the rule)."""
    return int(np.searchsorted(offsets, at, side="right")) - 1


def eloc_law(op, keys, phi, offsets=None, rows=None, with_terms=False):
    """ASP-ELOC-1 with Python floats (IEEE doubles, every operation rounded on its own, no contraction):
    `(hphi f64[N], eloc f64[N], missing u32[N])`.  Per row, over its connections in order, from +0.0: a target
    `keys[p]` with p in the row's segment adds `coeff * phi[p]`; any other target adds nothing and is counted
    when its coefficient is non-zero; `eloc = hphi / phi[rows[r]]`.  `with_terms`: also, per row, the number of
    connections n_r and `sum |coeff * phi[p]|` over the found ones (what the derived bounds are made of)."""
    keys = np.asarray(keys, dtype=np.uint64)
    phi = np.asarray(phi, dtype=np.float64)
    offsets = np.array([0, keys.size], dtype=np.int64) if offsets is None else np.asarray(offsets).astype(np.int64)
    rows = np.arange(keys.size, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    inverse, other, coeffs, starts = connections(op, keys[rows])
    hphi = np.zeros(rows.size, dtype=np.float64)
    missing = np.zeros(rows.size, dtype=np.uint32)
    count = np.zeros(rows.size, dtype=np.int64)
    magnitude = np.zeros(rows.size, dtype=np.float64)
    for r, at in enumerate(rows.tolist()):
        g = segment_of(offsets, at)
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        begin, end = int(starts[inverse[r]]), int(starts[inverse[r] + 1])
        where, found = positions(keys[lo:hi], other[begin:end])
        acc, lost, total = 0.0, 0, 0.0
        for e in range(end - begin):
            if found[e]:
                term = float(coeffs[begin + e]) * float(phi[lo + where[e]])
                acc = acc + term
                total += abs(term)
            elif coeffs[begin + e] != 0:
                lost += 1
        hphi[r], missing[r], count[r], magnitude[r] = acc, lost, end - begin, total
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        eloc = hphi / phi[rows]
    if with_terms:
        return hphi, eloc, missing, count, magnitude
    return hphi, eloc, missing


def derived_bound(count, magnitude):
    """`n_r * 2^-52 * sum_e |coeff_e * phi_e|`: both the law and a dense product sum the same n_r rounded
    products, each in its own order; either sum is within `(n_r - 1) * 2^-53 * sum|terms|` of the exact one
    (to first order), the products within `2^-53` each, and `n_r * 2^-52` leaves room for both and for
    the merging of equal targets in a matrix."""
    return np.asarray(count, dtype=np.float64) * 2.0 ** -52 * np.asarray(magnitude, dtype=np.float64)


def rayleigh_bound(phi, hphi, count, magnitude):
    """Both quotients are `sum_r phi_r (H phi)_r / sum phi^2` in floating point: each numerator is within
    `sum_r |phi_r| bound_r / 2` of the exact one for its rows and within `N 2^-53 sum_r |phi_r hphi_r|` for its
    dot product, and the denominators and the division add a few 2^-53 relative."""
    n = phi.size
    norm = float(np.dot(phi, phi))
    numerator = float(np.sum(np.abs(phi) * derived_bound(count, magnitude)))
    dots = 2.0 * n * 2.0 ** -53 * float(np.sum(np.abs(phi * hphi)))
    return (numerator + dots) / norm + 8.0 * 2.0 ** -53 * float(np.sum(np.abs(phi * hphi))) / norm


# -- tables --------------------------------------------------------------------------------------------------
@dataclass
class Table:
    name: str
    operator: object
    keys: np.ndarray      # u64[T]: the segments one after the other, each ascending and unique
    phi: np.ndarray       # f64[T] signed
    offsets: np.ndarray   # u64[S + 1]
    rows: np.ndarray      # u64[N]

    def law(self, phi=None, rows=None):
        if phi is None and rows is None:
            return _shared_law(self.name)
        return eloc_law(self.operator, self.keys, self.phi if phi is None else phi, self.offsets,
                        self.rows if rows is None else rows)

    @property
    def row_segments(self):
        return np.array([segment_of(self.offsets.astype(np.int64), int(at)) for at in self.rows], dtype=np.int64)


def signed_amplitudes(rng, count):
    """Both signs, magnitudes over a few decades, none zero."""
    return rng.normal(size=count) * np.exp(rng.normal(size=count)) + np.where(rng.random(count) < 0.5, -1e-3, 1e-3)


def one_segment(name, op, keys, seed, rows=None):
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, dtype=np.uint64)
    return Table(name, op, keys, signed_amplitudes(rng, keys.size), np.array([0, keys.size], dtype=np.uint64),
                 np.arange(keys.size, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64))


def from_segments(name, op, segments, rows, seed):
    """`segments`: ascending unique key arrays (possibly empty); `rows`: (segment, key) pairs."""
    rng = np.random.default_rng(seed)
    segments = [np.asarray(s, dtype=np.uint64) for s in segments]
    for s in segments:
        assert s.size < 2 or np.all(s[1:] > s[:-1])
    offsets = np.concatenate([[0], np.cumsum([s.size for s in segments])]).astype(np.uint64)
    keys = np.concatenate(segments) if segments else np.zeros(0, dtype=np.uint64)
    at = []
    for g, key in rows:
        p, found = positions(segments[g], np.array([key], dtype=np.uint64))
        assert found[0]
        at.append(int(offsets[g]) + int(p[0]))
    return Table(name, op, keys, signed_amplitudes(rng, keys.size), offsets, np.array(at, dtype=np.uint64))


def neighbourhood(op, key):
    """The one-hop neighbourhood of a state, itself included: the targets with a non-zero coefficient
    (in a sector: the representatives of non-zero norm), ascending."""
    other, coeffs, _ = op.batched_apply(np.array([key], dtype=np.uint64))
    return np.union1d(other[coeffs != 0, 0], np.array([key], dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def kagome16_basis():
    op = model_operator("heisenberg_kagome_16")
    op.basis.build()
    return op, op.basis.states


def _kagome16_subset(count):
    op, states = kagome16_basis()
    rng = np.random.default_rng(count)
    return one_segment("kagome16 K=%d" % count, op, np.sort(rng.choice(states, size=count, replace=False)), count)


def _from_field_case(name, field_name):
    c = field_case(field_name)
    return one_segment(name, c.operator, c.keys, 7 + len(name))


def _sk16_whole_neighbourhood():
    """One sk-type state with its one-hop neighbourhood as the table: 8 x 8 antiparallel pairs, 65 connections,
    all found, over two chunks of bonds."""
    op = model_operator("sk_16_1")
    key = int(field_case("sk16 120 bonds").keys[3])
    table = neighbourhood(op, key)
    t = one_segment("sk16 one row of 65 connections", op, table, 31)
    t.rows = np.array([int(np.searchsorted(table, np.uint64(key)))], dtype=np.uint64)
    return t


def _many_small_segments():
    """4097 segments of 1-3 keys: a random state with none, one or two of its neighbours; one row each."""
    op, states = kagome16_basis()
    rng = np.random.default_rng(4097)
    picks = rng.choice(states, size=4097, replace=True)
    other, coeffs, counts = op.batched_apply(picks)
    starts = np.concatenate([[0], np.cumsum(counts)])
    segments, rows = [], []
    for g, key in enumerate(picks.tolist()):
        near = other[starts[g] + 1:starts[g + 1], 0]
        extra = rng.choice(near, size=g % 3, replace=False)
        segments.append(np.union1d(extra, np.array([key], dtype=np.uint64)))
        rows.append((g, key))
    return from_segments("4097 segments of 1-3 keys", op, segments, rows, 41)


def _empty_segments():
    """Empty segments first, in the middle (two in a row) and last."""
    op, states = kagome16_basis()
    a, b, c = (neighbourhood(op, int(states[i])) for i in (10, 2000, 9000))
    none = np.zeros(0, dtype=np.uint64)
    segments = [none, a, none, none, b[:5], c, none]
    rows = [(1, int(k)) for k in a[:3]] + [(4, int(b[0])), (4, int(b[4]))] + [(5, int(k)) for k in c[-2:]]
    return from_segments("empty segments", op, segments, rows, 43)


def _same_state_everywhere():
    """One state in 300 segments, each with amplitudes of its own: the state alone, or with a varying part
    of its neighbourhood."""
    op, states = kagome16_basis()
    key = int(states[5000])
    near = neighbourhood(op, key)
    rng = np.random.default_rng(300)
    segments = []
    for g in range(300):
        keep = rng.random(near.size) < (g % 5) / 4.0
        segments.append(np.union1d(near[keep], np.array([key], dtype=np.uint64)))
    return from_segments("one state in 300 segments", op, segments, [(g, key) for g in range(300)], 47)


def _three_segments():
    """Segments of 5, 70 and 130 overlapping states; every entry a row."""
    op, _ = kagome16_basis()
    whole = grow(op, 160, 51)
    t = from_segments("three segments", op, [whole[:5], whole[20:90], whole[30:160]], [], 53)
    t.rows = np.arange(t.keys.size, dtype=np.uint64)
    return t


def _listed(field_name):
    """List form: the cluster of the field case as one segment (connections leave it), and the cluster with
    everything it reaches as a second one (every connection of a cluster row is found there, a representative
    reached twice included); rows: the cluster's states in both."""
    c = field_case(field_name)
    reach = np.union1d(c.keys, c.other[c.coeffs != 0])
    rows = [(0, int(k)) for k in c.keys] + [(1, int(k)) for k in c.keys]
    return from_segments(field_name, c.operator, [c.keys, reach], rows, 59 + len(field_name))


PLAIN_BONDS = {"kagome16 24 bonds": "kagome16 K=300", "j1j2 64 bonds": "j1j2 64 bonds",
               "sk16 first 65 bonds": "sk16 first 65 bonds", "sk16 120 bonds": "sk16 120 bonds",
               "ring64 bit 63": "ring64 bit 63", "ring4 full basis": "ring4 full basis"}
SIZES = (1, 63, 64, 65, 301, 4097)
LISTED = ("kagome18 inversion +1", "kagome18 inversion -1", "ring20 all-to-all, inversion -1", "ring22 inversion -1",
          "single-site flips")
BUILDERS = {name: functools.partial(_from_field_case, name, source) for name, source in PLAIN_BONDS.items()}
BUILDERS.update({"kagome16 K=%d" % k: functools.partial(_kagome16_subset, k) for k in SIZES})
BUILDERS.update({
    "sk16 one row of 65 connections": _sk16_whole_neighbourhood,
    "4097 segments of 1-3 keys": _many_small_segments,
    "empty segments": _empty_segments,
    "one state in 300 segments": _same_state_everywhere,
    "three segments": _three_segments,
})
BUILDERS.update({name: functools.partial(_listed, name) for name in LISTED})
PLAIN = tuple(name for name in BUILDERS if name not in LISTED)
NAMES = PLAIN + LISTED


@functools.lru_cache(maxsize=None)
def table(name):
    t = BUILDERS[name]()
    t.name = name
    return t


@functools.lru_cache(maxsize=None)
def _shared_law(name):
    t = table(name)
    return eloc_law(t.operator, t.keys, t.phi, t.offsets, t.rows)


def flipped(t, segments):
    """`phi` negated over the given segments."""
    phi = t.phi.copy()
    for g in segments:
        phi[int(t.offsets[g]):int(t.offsets[g + 1])] *= -1.0
    return phi


def flip_holds(hphi, eloc, flipped_hphi, flipped_eloc, sign):
    """The flip consequence of the law: with phi negated over a row's segment (`sign` -1) every term changes its
    sign and nothing else, so `hphi` is negated and `eloc` kept, bit for bit — wherever the sum is not zero.  A sum
    that is exactly zero is +0.0 either way (the accumulator starts at +0.0; `x + (-x)` and `+0.0 + -0.0` round to
    +0.0), so there `hphi` keeps its bits and `eloc` is a zero whose sign follows the row's amplitude."""
    zero = hphi == 0
    if np.any(np.signbit(hphi[zero])) or np.any(np.signbit(flipped_hphi[zero])):
        return False
    return bool(same_bits(flipped_hphi[~zero], (sign * hphi)[~zero]) and same_bits(flipped_eloc[~zero], eloc[~zero])
                and same_bits(flipped_hphi[zero], hphi[zero]) and np.all(flipped_eloc[zero] == 0)
                and np.all(eloc[zero] == 0))


def awkward_targets(t):
    """`phi` with signed zeros and subnormals everywhere but at the rows."""
    phi = awkward_amplitudes(t.keys.size)
    phi[t.rows.astype(np.int64)] = t.phi[t.rows.astype(np.int64)]
    return phi


# -- full bases ----------------------------------------------------------------------------------------------
def full_basis_cases():
    """(name, operator with its basis built): a plain and two symmetric full bases."""
    import symmetry_cases

    out = [("ring4", plain_ring(4, 2)), ("kagome16", kagome16_basis()[0])]
    for name in ("ring12 inversion -1", "ring12 inversion +1"):
        out.append((name, symmetry_cases.expected(symmetry_cases.BY_NAME[name]).operator))
    for _, op in out:
        if op.basis._states is None:
            op.basis.build()
    return out
