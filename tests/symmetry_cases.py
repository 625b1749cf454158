"""The cases of tests/test_gpu_symmetry_edges.py and tests/test_symmetry_cases.py: symmetry-adapted
bases at the EDGES of the kernels behind asp_operator_apply / _ising / _extend
(csrc/operator_apply.hip: state_info, k_source_norms, k_symmetrise, k_symmetrise_rows, k_merge_rows,
k_sym_rows), where tests/test_gpu_symmetry.py runs them at production shapes only:

  * spin inversion with character -1 (orbits of norm 0, character -1, the sign of a zero coefficient);
  * group sizes around the 64 lanes that k_symmetrise_rows spreads the elements over (1, 63, 64, 65,
    128), 64 sites (full mask), an odd site count, and tables beyond 64 KiB and 160 KiB of LDS;
  * rows of more than 64 and more than 128 connections with dozens of targets per representative;
  * single-site flips under a group.

A helper module like tests/helpers.py and tests/sector_cases.py: no fixtures, no files, nothing
compiled, no GPU.  Every case says what it is there to reach; tests/test_symmetry_cases.py asserts
from the host objects alone that it still does, and checks symmetry.py against the brute-force
reference below.  The expected values (`expected`) are computed once per case and shared.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

ROWS_LDS_SOFT = 64 * 1024    # beyond: hipFuncSetAttribute before k_symmetrise_rows
ROWS_LDS_HARD = 160 * 1024   # beyond: the entry-wise kernels, whatever ASP_SYMMETRISE_ROWS says
MAX_IMAGES = 2 * 10 ** 7     # P x connections that the numpy restatement materialises per case


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable[[], object]         # -> operators.Operator on a symmetric basis (not built)
    permutations: int                  # P the case is built for
    lds: str                           # "small" (<= 64 KiB), "large" (<= 160 KiB), "fallback"
    num_keys: Optional[int]            # None: the whole sector
    reaches: Tuple[str, ...]
    longest_row: Tuple[int, int] = (0, 64)   # (exclusive lower, inclusive upper) bound
    seeds: Optional[Callable[[object], np.ndarray]] = None   # operator -> states to grow the keys from
    zero_norms: bool = False           # the keys' targets include orbits of norm 0
    seed: int = 0


def rows_lds_bytes(group):
    """Dynamic LDS of k_symmetrise_rows: images u64[4 wavefronts][P] | table u8[number_spins][P]."""
    return 32 * group.num_permutations + group.number_spins * group.num_permutations


def lds_class(group):
    size = rows_lds_bytes(group)
    return "small" if size <= ROWS_LDS_SOFT else ("large" if size <= ROWS_LDS_HARD else "fallback")


# -- groups and invariant Hamiltonians ---------------------------------------------------------------
def _group(n, generators, inversion):
    from annealing_sign_problem_amd import symmetry

    return symmetry.SymmetryGroup(n, generators, inversion)


def translation(n):
    return [(i + 1) % n for i in range(n)]


def reflection(n):
    return [(n - i) % n for i in range(n)]


def cycle(n, sites):
    """The permutation of 0..n-1 that moves sites[k] to sites[k + 1] (cyclically)."""
    p = list(range(n))
    for k, s in enumerate(sites):
        p[s] = sites[(k + 1) % len(sites)]
    return p


def orbit_bonds(group, seeds):
    """Every bond in the group orbit of the seed bonds, as sorted (low site, high site) pairs: an
    operator with one coupling on all of them commutes with the group."""
    p = group.permutations.astype(np.int64)
    out = set()
    for a, b in seeds:
        for x, y in zip(p[:, a].tolist(), p[:, b].tolist()):
            out.add((min(x, y), max(x, y)))
    return sorted(out)


def is_invariant(op):
    """Every element of the basis' group maps every term's bond set onto itself."""
    p = op.basis.group.permutations.astype(np.int64)
    for term in op.terms:
        bonds = {(min(a, b), max(a, b)) for a, b in term.sites}
        a = np.array([s[0] for s in term.sites])
        b = np.array([s[1] for s in term.sites])
        for e in range(p.shape[0]):
            if {(min(x, y), max(x, y)) for x, y in zip(p[e, a].tolist(), p[e, b].tolist())} != bonds:
                return False
    return True


def heisenberg(n, weight, group, seeds_and_couplings):
    """sigma.sigma with one coupling per orbit of seed bonds."""
    from annealing_sign_problem_amd import operators

    terms = [operators.Term(c * operators.SIGMA_DOT_SIGMA, orbit_bonds(group, seeds))
             for seeds, c in seeds_and_couplings]
    return operators.Operator(operators.SpinBasis(n, weight, group), terms)


def ring(n, weight, inversion, with_reflection=True, couplings=(1.0,)):
    """Heisenberg ring: coupling couplings[d - 1] between sites at distance d."""
    gens = [translation(n)] + ([reflection(n)] if with_reflection else [])
    group = _group(n, gens, inversion)
    return heisenberg(n, weight, group, [([(0, d + 1)], c) for d, c in enumerate(couplings)])


def all_to_all_ring(n, inversion):
    """Uniform sigma.sigma between ALL pairs at half filling: a row holds 1 + (n/2)^2 connections,
    and the 2n lattice maps send dozens of them to the same representative."""
    return ring(n, n // 2, inversion, couplings=(1.0,) * (n // 2))


def inversion_only(inversion):
    """10 sites, no lattice map at all: the group is {1, flip}, P = 1."""
    group = _group(10, [], inversion)
    seeds = [(i, (i + 1) % 10) for i in range(10)] + [(0, 5), (2, 7), (1, 4)]
    return heisenberg(10, 5, group, [(seeds[:10], 1.0), (seeds[10:], 0.5)])


def two_cycles(inversion):
    """18 sites: a 5-cycle on sites 0..4 and a 13-cycle on sites 5..17 generate Z5 x Z13, P = 65."""
    group = _group(18, [cycle(18, list(range(5))), cycle(18, list(range(5, 18)))], inversion)
    return heisenberg(18, 9, group, [([(0, 1)], 1.0), ([(5, 6)], 1.0), ([(0, 5)], 0.25)])


def blocks64(with_three_cycle, inversion):
    """64 sites: S6 permutes six blocks of ten sites (P = 720); optionally a 3-cycle on sites 60, 61,
    62 on top (P = 2160).  Chains inside the blocks, equal positions of different blocks coupled,
    the blocks' last sites coupled to the four remaining sites."""
    swap = list(range(64))
    for k in range(10):
        swap[k], swap[10 + k] = 10 + k, k
    rotate = [(i + 10) % 60 for i in range(60)] + [60, 61, 62, 63]
    gens = [swap, rotate] + ([cycle(64, [60, 61, 62])] if with_three_cycle else [])
    group = _group(64, gens, inversion)
    chain = [(k, k + 1) for k in range(9)]
    return heisenberg(64, 32, group, [(chain, 1.0), ([(0, 10), (5, 15)], 0.5),
                                      ([(9, 60), (9, 63)], 0.75), ([(60, 61), (62, 63)], 1.0)])


ZZ = np.diag([1.0, -1.0, -1.0, 1.0])
FIELD = 0.5 * np.array([[0.0, 1.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]])
"""(X (x) 1 + 1 (x) X) / 2: a transverse field written as a two-site matrix."""


def transverse_field_ring(inversion):
    """12 sites at ANY magnetisation: ZZ plus a transverse field on the nearest bonds (single-site
    flips: `flipped == 1` in k_symmetrise_rows, and the two bonds of a site reach the same state
    twice), and a weak sigma.sigma on second neighbours so that rows hold two-site flips too.  The
    field commutes with the lattice maps and with global inversion (the product of all X)."""
    from annealing_sign_problem_amd import operators

    n = 12
    group = _group(n, [translation(n), reflection(n)], inversion)
    terms = [operators.Term(ZZ + 0.75 * FIELD, orbit_bonds(group, [(0, 1)])),
             operators.Term(0.5 * operators.SIGMA_DOT_SIGMA, orbit_bonds(group, [(0, 2)]))]
    return operators.Operator(operators.SpinBasis(n, None, group), terms)


def patterns(n, units):
    """The states that repeat each bit string of `units` around n sites (site 0 = first character)."""
    return np.array([int((u * (n // len(u)))[::-1], 2) for u in units], dtype=np.uint64)


def beside_alternating(op):
    """The states one and two exchanges away from 0101... and 00110011...: a translation maps these
    two patterns onto their complements, so with inversion -1 their orbits have norm 0 (with the
    reflection, so have the orbits one exchange away), and keys grown from here have such orbits
    among their targets."""
    plain = plain_twin(op)
    once, _, _ = plain.batched_apply(patterns(op.basis.number_spins, ["01", "0011"]))
    twice, _, _ = plain.batched_apply(np.unique(once[:, 0]))
    return np.unique(np.concatenate([once[:, 0], twice[:, 0]]))


def half_period(op):
    """Every state of period n/2 at half filling: their stabilisers hold at least the translation
    by n/2, so their rows reach each representative several times."""
    from itertools import combinations

    half = op.basis.number_spins // 2
    units = ["".join("1" if i in up else "0" for i in range(half)) for up in combinations(range(half), half // 2)]
    return patterns(op.basis.number_spins, units)


P = functools.partial

CASES = (
    Case("ring12 inversion -1", P(ring, 12, 6, -1), 24, "small", None,
         ("zero-norm targets", "character -1", "walk and minimum rule disagree", "sign of zero"),
         zero_norms=True),
    Case("ring12 inversion +1", P(ring, 12, 6, 1), 24, "small", None, ("the +1 twin of the above",)),
    Case("ring12 no inversion", P(ring, 12, 6, None), 24, "small", None, ("g.inversion == 0",)),
    Case("ring22 inversion -1", P(ring, 22, 11, -1, couplings=(1.0, 0.5)), 44, "small", 300,
         ("-1 beyond one wavefront of states", "zero-norm targets"), zero_norms=True),
    Case("inversion only -1", P(inversion_only, -1), 1, "small", None, ("P = 1", "character -1")),
    Case("inversion only +1", P(inversion_only, 1), 1, "small", None, ("P = 1",)),
    Case("ring63 translations", P(ring, 63, 31, None, with_reflection=False), 63, "small", 200,
         ("P = 63: one idle lane", "odd site count")),
    Case("ring64 translations, inversion -1", P(ring, 64, 32, -1, with_reflection=False), 64, "small",
         200, ("P = 64 = lanes", "64 sites: full mask", "states at or above 2^63", "zero-norm targets"),
         seeds=beside_alternating, zero_norms=True),
    Case("ring64 with reflection, inversion -1", P(ring, 64, 32, -1), 128, "small", 200,
         ("P = 128: two full passes", "64 sites: full mask", "states at or above 2^63", "zero-norm targets"),
         seeds=beside_alternating, zero_norms=True),
    Case("5-cycle x 13-cycle, inversion -1", P(two_cycles, -1), 65, "small", 200,
         ("P = 65: a second pass with one lane", "character -1")),
    Case("blocks64 S6, inversion -1", P(blocks64, False, -1), 720, "large", 32,
         ("LDS 69 120 B: hipFuncSetAttribute", "64 sites")),
    Case("blocks64 S6 x C3, inversion +1", P(blocks64, True, 1), 2160, "fallback", 24,
         ("LDS 207 360 B: automatic entry-wise fallback",)),
    Case("ring20 all-to-all, inversion -1", P(all_to_all_ring, 20, -1), 40, "small", 250,
         ("rows of 101 connections", "many targets per representative", "zero-norm targets"), (64, 128),
         seeds=half_period, zero_norms=True),
    Case("ring24 all-to-all, inversion -1", P(all_to_all_ring, 24, -1), 48, "small", 250,
         ("rows of 145 connections", "many targets per representative", "zero-norm targets"),
         (128, 1 << 20), seeds=half_period, zero_norms=True),
    Case("transverse-field ring12, inversion +1", P(transverse_field_ring, 1), 24, "small", None,
         ("single-site flips under a group",)),
    Case("transverse-field ring12, inversion -1", P(transverse_field_ring, -1), 24, "small", None,
         ("single-site flips under a group", "zero-norm targets"), zero_norms=True),
)

BY_NAME = {case.name: case for case in CASES}
MINUS = tuple(case for case in CASES if "inversion -1" in case.name)
DENSE = tuple(case for case in CASES if "ring12" in case.name)   # small enough for the full space


# -- brute force in Python integers --------------------------------------------------------------------
def brute_state_info(group, state):
    """(representative, characters of the elements that map `state` onto it, norm) by applying
    every element of the group — lattice maps and, with inversion, each followed by the global
    flip — to a Python integer.  norm = sqrt(max(sum of the stabiliser's characters, 0) / |G|)."""
    state = int(state)
    mask = (1 << group.number_spins) - 1
    bits = [i for i in range(group.number_spins) if (state >> i) & 1]
    images = []                                   # (image, character of the element)
    for dst in group.permutations.tolist():
        y = 0
        for i in bits:
            y |= 1 << dst[i]
        images.append((y, 1))
        if group.spin_inversion:
            images.append((~y & mask, group.spin_inversion))
    rep = min(y for y, _ in images)
    onto = {chi for y, chi in images if y == rep}
    stabiliser = sum(chi for y, chi in images if y == state)
    return rep, onto, float(np.sqrt(max(stabiliser, 0) / len(images)))


def brute_budget(group):
    """How many states brute_state_info takes in about a second of Python."""
    return int(max(20, min(3000, 3 * 10 ** 6 // (group.num_permutations * group.number_spins))))


def walk_through_flip(group, states):
    """`through_flip` as ONE sequential walk over the elements with strict `<` decides it (plain
    image, then flipped image, element by element; what the device did before it took numpy's rule:
    flipped minimum strictly below plain minimum).  The two differ where a plain image equals a
    flipped one, i.e. only on orbits that inversion maps onto themselves."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    plain = group.images(states)
    best = states.copy()
    through = np.zeros(states.shape[0], dtype=bool)
    for e in range(plain.shape[0]):
        lower = plain[e] < best
        best[lower] = plain[e][lower]
        through[lower] = False
        if group.spin_inversion:
            z = ~plain[e] & group.mask
            lower = z < best
            best[lower] = z[lower]
            through[lower] = True
    return through


# -- host expectations ---------------------------------------------------------------------------------
def plain_twin(op):
    """The same terms on the basis without any symmetry."""
    from annealing_sign_problem_amd import operators

    return operators.Operator(operators.SpinBasis(op.basis.number_spins, op.basis.hamming_weight), op.terms)


def _random_states(rng, n, weight, count):
    if weight is None:
        return rng.integers(0, 1 << n, size=count, dtype=np.uint64)
    return np.array([sum(1 << int(b) for b in rng.choice(n, size=weight, replace=False))
                     for _ in range(count)], dtype=np.uint64)


def grow_keys(op, count, rng, seeds=None):
    """A connected cluster of `count` sorted unique representatives of non-zero norm: grown from a
    random representative — or from the (at most 8) representatives of greatest norm among `seeds`
    — through the host batched_apply, zero-norm targets dropped."""
    group, n, w = op.basis.group, op.basis.number_spins, op.basis.hamming_weight
    if seeds is None:
        rep, _, norm = group.state_info(_random_states(rng, n, w, 16))
        keys = {int(rep[norm > 0][0])}
    else:
        rep, _, norm = group.state_info(seeds)
        rep, first = np.unique(rep[norm > 0], return_index=True)
        keys = {int(x) for x in rep[np.argsort(-norm[norm > 0][first], kind="stable")[:8]]}
    frontier = sorted(keys)
    while len(keys) < count:
        if not frontier:
            rep, _, norm = group.state_info(_random_states(rng, n, w, 16))
            frontier = [int(x) for x in rep[norm > 0][:1] if int(x) not in keys]
            keys.update(frontier)
            continue
        other, _, _ = op.batched_apply(np.array(frontier, dtype=np.uint64))
        cand = np.unique(other[:, 0])
        cand = cand[group.state_info(cand)[2] > 0]
        fresh = [int(x) for x in rng.permutation(cand) if int(x) not in keys]
        fresh = fresh[: max(4, min(count // 8, count - len(keys)))][: count - len(keys)]
        keys.update(fresh)
        frontier = fresh
    return np.array(sorted(keys), dtype=np.uint64)


@dataclass
class Expected:
    case: Case
    operator: object
    keys: np.ndarray           # sorted unique representatives of non-zero norm
    other: np.ndarray          # host batched_apply(keys): representatives u64[N]
    coeffs: np.ndarray         # f64[N]
    counts: np.ndarray         # i64[K]
    raw_targets: np.ndarray    # the same connections BEFORE symmetrisation u64[N]
    target_norm: np.ndarray    # norm of every raw target f64[N]
    extension: np.ndarray      # sorted unique representatives of the targets of non-zero norm
    states: np.ndarray         # what state_info is compared on
    info: tuple                # host state_info(states)
    psi: np.ndarray            # unit-norm amplitudes over the keys
    outside: Optional[int]     # a representative of norm 0 next to the keys, if the sector has one
    high_keys: Optional[np.ndarray]   # 64 sites: images of keys at or above 2^63 (sources that are
                                      # no representatives: a representative of a ring lies below)

    @property
    def group(self):
        return self.operator.basis.group


@functools.lru_cache(maxsize=None)
def expected(case):
    op = case.make()
    group, n, w = op.basis.group, op.basis.number_spins, op.basis.hamming_weight
    rng = np.random.default_rng(1000 + case.seed)
    if case.num_keys is None:
        op.basis.build()
        keys = op.basis.states
    else:
        keys = grow_keys(op, case.num_keys, rng, None if case.seeds is None else case.seeds(op))
    other, coeffs, counts = op.batched_apply(keys)
    assert not np.any(coeffs.imag)
    raw, _, raw_counts = plain_twin(op).batched_apply(keys)
    assert np.array_equal(raw_counts, counts)
    raw = np.ascontiguousarray(raw[:, 0])
    rep, _, target_norm = group.state_info(raw)
    assert np.array_equal(rep, other[:, 0])
    extension = np.unique(rep[target_norm > 0])
    if case.num_keys is None and w is not None and n <= 12:
        states = plain_twin(op).basis
        states.build()
        states = states.states                    # the whole weight class (924 states for ring12)
    else:
        budget = max(64, min(3000, MAX_IMAGES // (10 * group.num_permutations)))
        extra = _random_states(rng, n, w, 64)
        # images of the keys under a few elements: non-representatives, for 64 sites also at or
        # above 2^63
        moved = group.images(keys[:32])[:: max(1, group.num_permutations // 7)].reshape(-1)
        flipped = (~moved & group.mask) if group.spin_inversion else moved[:0]
        states = np.unique(np.concatenate([keys, moved, flipped, extra, raw[:: max(1, raw.size // 1500)]]))
        if states.size > budget:
            states = np.sort(rng.choice(states, size=budget, replace=False))
    info = group.state_info(states)
    psi = rng.normal(size=keys.shape[0]) * np.exp(rng.normal(size=keys.shape[0]))
    psi /= np.linalg.norm(psi)
    zero = np.unique(rep[target_norm == 0])
    outside = int(zero[zero.size // 2]) if zero.size else None
    high = None
    if n == 64:
        high = np.unique(group.images(keys[:48]).reshape(-1))
        high = high[high >= np.uint64(1 << 63)][:: max(1, high.size // 150)]
        high = high if high.size else None       # (the block groups leave site 63 where it is)
    return Expected(case, op, keys, np.ascontiguousarray(other[:, 0]), np.ascontiguousarray(coeffs.real),
                    counts, raw, target_norm, extension, states, info, psi, outside, high)


def merged_matrix(op, keys):
    """Dense <r'~|H|r~> over `keys` from the merged entries of the host batched_apply (rows =
    output states, as Operator.to_sparse; targets outside `keys` must carry coefficient 0)."""
    other, coeffs, counts = op.batched_apply(keys)
    col = np.repeat(np.arange(keys.size), counts)
    row = np.clip(np.searchsorted(keys, other[:, 0]), 0, keys.size - 1)
    inside = keys[row] == other[:, 0]
    assert np.all(coeffs[~inside] == 0)
    out = np.zeros((keys.size, keys.size))
    np.add.at(out, (row[inside], col[inside]), coeffs.real[inside])
    return out


def dense_projection(op, keys):
    """The same matrix from the full-space operator: V^T H V with V[s, r] = chi(s -> r) norm(r) on
    the orbit of r — the symmetrised states |r~> written out (symmetry.py, docstring)."""
    full = plain_twin(op)
    full.basis.build()
    h = full.to_sparse().real
    rep, character, norm = op.basis.group.state_info(full.basis.states)
    where = np.clip(np.searchsorted(keys, rep), 0, keys.size - 1)
    inside = (norm > 0) & (keys[where] == rep)
    v = np.zeros((full.basis.number_states, keys.size))
    v[np.nonzero(inside)[0], where[inside]] = character[inside] * norm[inside]
    return v.T @ (h @ v), abs(h).max()
