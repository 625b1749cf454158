"""The cases of tests/test_gpu_sector_widths.py and tests/test_sector_cases.py: bases as WIDE as the
production models' (36 to 48 sites, 144 and 384 lattice maps, 72 and 96 transitions, 16 + 20 bit
index words) but with few states, because the Hamming weight is low instead of the site count.
csrc/sector_basis.hip and csrc/plain_basis.hip then take the branches `make kagome_36`,
`make pyrochlore_32` and `make sk_32_1` take, and the numpy / scipy host route
(operators.SpinBasis.build, symmetry.SymmetryGroup.state_info, operators.Operator.to_sparse) still
lists every state and every matrix element in seconds.

A helper module like tests/helpers.py: no fixtures, no files, nothing compiled.  Every case says
which path of the kernels it is there to reach; tests/test_sector_cases.py asserts from the host
objects alone that the table as a whole still reaches them.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable[[], object]     # -> operators.Operator (basis not built)
    reaches: Tuple[str, ...]       # the kernel paths this case is there for


# -- the kernels' sizing, restated as plain arithmetic ---------------------------------------------
def sector_word_bits(n):
    """(lo_bits, hi_bits) of asp_sector_enumerate: a workgroup takes one value of the high bits at
    a time."""
    lo = min(n // 2 + (n & 1), 20)
    return lo, n - lo


def plain_word_bits(n):
    """(lo_bits, hi_bits) of asp_plain_basis_create."""
    lo = min(16, (n + 1) // 2)
    return lo, n - lo


def plain_bond_kind(a, b, lo_bits):
    """0: both sites in the high word, 1: first high / second low, 2: first low / second high,
    3: both low (PlainBond::kind)."""
    return (0 if b >= lo_bits else 1) if a >= lo_bits else (2 if b >= lo_bits else 3)


def transitions(operator):
    """The (bond, src ^ dst) pairs that carry a non-zero element, counted as asp_sector_rows
    counts them: a list of the values src ^ dst (1 and 2 flip one site, 3 flips both)."""
    out = []
    for term in operator.terms:
        m = term.matrix.real
        for _ in term.sites:
            for x in (1, 2, 3):
                if any(m[src ^ x, src] != 0 for src in range(4)):
                    out.append(x)
    return out


# -- operators -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    from annealing_sign_problem_amd import synthetic

    return synthetic.load_models()


def _ring_group(n, inversion):
    from annealing_sign_problem_amd import symmetry

    return symmetry.SymmetryGroup(n, [[(i + 1) % n for i in range(n)], [(n - i) % n for i in range(n)]],
                                  inversion)


def ring(n, weight, inversion):
    """Heisenberg ring with translations, reflection and (optionally) spin inversion."""
    from annealing_sign_problem_amd import operators

    basis = operators.SpinBasis(n, weight, _ring_group(n, inversion))
    return operators.Operator(basis, [
        operators.Term(operators.SIGMA_DOT_SIGMA, [(i, (i + 1) % n) for i in range(n)])])


FIELD = 0.5 * np.array([[0.0, 1.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]])
"""(X (x) 1 + 1 (x) X) / 2: a transverse field written as a two-site term (elements with
src ^ dst = 1 and 2, the single-site flips)."""


def ring12_in_a_field(field_on_second_neighbours):
    """12-site ring at ANY magnetisation, translations + reflection + spin inversion (+1):
    sigma.sigma on nearest (1) and next-nearest (0.5) bonds and a transverse field, which commutes
    with every lattice map and with global spin inversion (the product of all X).  The field sits
    on the nearest bonds (0.75 per bond: 24 + 12 = 48 transitions) or on all 24 bonds (0.75 and
    0.25: 24 x 3 = 72 transitions, so that single-site flips also fall into the second word of
    k_sector_rows' mask)."""
    from annealing_sign_problem_amd import operators

    n = 12
    first = [(i, (i + 1) % n) for i in range(n)]
    second = [(i, (i + 2) % n) for i in range(n)]
    s = operators.SIGMA_DOT_SIGMA
    terms = [operators.Term(s + 0.75 * FIELD, first),
             operators.Term(0.5 * s + (0.25 * FIELD if field_on_second_neighbours else 0.0), second)]
    return operators.Operator(operators.SpinBasis(n, None, _ring_group(n, 1)), terms)


def model_at_low_weight(name, weight, symmetric):
    """A bundled model's bonds (and, if `symmetric`, its lattice maps WITHOUT spin inversion, which
    would leave the weight class) at a low Hamming weight."""
    from annealing_sign_problem_amd import operators, symmetry

    config = _models()[name]
    n = config["basis"]["number_spins"]
    group = None
    if symmetric:
        group = symmetry.SymmetryGroup(n, [s["permutation"] for s in config["basis"]["symmetries"]], None)
    terms = [operators.Term(np.asarray(t["matrix"]), [tuple(s) for s in t["sites"]])
             for t in config["hamiltonian"]["terms"]]
    if symmetric:
        # the bonds in reverse: a representative is the SMALLEST state of its orbit, its few up
        # spins sit on the first sites, and in the models' order the bonds beyond the 64th join
        # the last sites — no row would flip one of them
        terms = [operators.Term(t.matrix, t.sites[::-1]) for t in terms[::-1]]
    return operators.Operator(operators.SpinBasis(n, weight, group), terms)


def sk_32_at_weight_4():
    """sk_32_1's 496 bonds.  Its couplings are random reals, so a diagonal element — a sum of 496
    terms — depends on the order of the additions.  csrc/plain_basis.hip adds them with the bonds
    inside the high word first, then the mixed ones, then those inside the low word (a stable
    sort); the terms are listed in that order here, so that the host's sum is the same IEEE
    sequence and whole columns can be compared exactly."""
    from annealing_sign_problem_amd import operators

    op = model_at_low_weight("sk_32_1", 4, symmetric=False)
    lo_bits = plain_word_bits(32)[0]
    bonds = [(term.matrix, site) for term in op.terms for site in term.sites]
    group_of = {0: 0, 1: 1, 2: 1, 3: 2}
    bonds.sort(key=lambda bond: group_of[plain_bond_kind(bond[1][0], bond[1][1], lo_bits)])  # stable
    return operators.Operator(op.basis, [operators.Term(m, [site]) for m, site in bonds])


def open_chain(n, weight, far, far_matrix):
    """Open chain: sigma.sigma on (i, i + 1) and `far_matrix` on (i + far, i) — the far bonds are
    written high site first, so that those across the two index words are of kind 1."""
    from annealing_sign_problem_amd import operators

    terms = [operators.Term(operators.SIGMA_DOT_SIGMA, [(i, i + 1) for i in range(n - 1)])]
    if n > far:
        terms.append(operators.Term(far_matrix, [(i + far, i) for i in range(n - far)]))
    return operators.Operator(operators.SpinBasis(n, weight), terms)


def long_chain(n):
    from annealing_sign_problem_amd import operators

    return open_chain(n, 3, 5, 0.37 * operators.SIGMA_DOT_SIGMA)


SMALL_FAR = np.diag([0.0, 0.25, -0.25, 0.0])
"""Added to the small chains' second-neighbour exchange: tells the first site of a bond from the
second (sigma.sigma does not).  Every element of the small chains is a dyadic fraction, so their
diagonal sums are exact in any order and the matrices can be compared for equality."""


def small_chain(n, weight):
    from annealing_sign_problem_amd import operators

    return open_chain(n, weight, 2, 0.375 * operators.SIGMA_DOT_SIGMA + SMALL_FAR)


# -- the table -------------------------------------------------------------------------------------
SECTOR_CASES = (
    Case("ring44 weight 3", lambda: ring(44, 3, None), (
        "n > 40: lo_bits clamped to 20, hi_bits = 24",
        "permuted(): sites >= 32 (the xh / yh halves)",
        "third filter pass: P = 88 > 41")),
    Case("ring48 weight 3", lambda: ring(48, 3, None), (
        "n = 48, the widest basis the entry point accepts: hi_bits = 28",
        "permuted(): sites >= 32",
        "third filter pass: P = 96 > 41")),
    Case("ring22 half filling, inversion -1", lambda: ring(22, 11, -1), (
        "third filter pass: P = 44 > 41, with spin inversion",
        "orbits of zero norm are dropped after three passes",
        "stabilisers larger than 1: norms differ between rows")),
    Case("ring22 half filling, inversion +1", lambda: ring(22, 11, 1), (
        "third filter pass: P = 44 > 41, with spin inversion",
        "stabilisers larger than 1: norms differ between rows")),
    Case("kagome_36 weight 4", lambda: model_at_low_weight("heisenberg_kagome_36", 4, True), (
        "the production group: 144 lattice maps of 36 sites, all three passes",
        "permuted(): sites >= 32",
        "72 transitions: the second word of the todo mask")),
    Case("pyrochlore weight 4", lambda: model_at_low_weight("heisenberg_pyrochlore_2x2x2", 4, True), (
        "the production group: 384 lattice maps, all three passes",
        "96 transitions: the second word of the todo mask")),
    Case("ring12 any magnetisation, field on nearest bonds", lambda: ring12_in_a_field(False), (
        "single-site transitions (code & 3 in {1, 2})",
        "candidates without a weight: every low word")),
    Case("ring12 any magnetisation, field on all bonds", lambda: ring12_in_a_field(True), (
        "single-site transitions in BOTH words of the todo mask: 72 transitions",
        "candidates without a weight: every low word")),
)

#: spin inversion at a weight other than n / 2: the inverted images lie outside the weight class,
#: so a state is dropped when an image of weight n - w is smaller.  The lists and norms of device and
#: host must still agree (the operator of such a basis leaves it: `to_sparse` raises, and there is
#: no matrix to compare).  On the 14-site ring weight 6 keeps 122 of the 126 orbits and weight 8
#: keeps 4, so both outcomes of that comparison occur in either case.
ENUMERATION_CASES = tuple(
    Case("ring14 weight %d, inversion %+d" % (w, inversion), lambda w=w, inversion=inversion: ring(14, w, inversion),
         ("spin inversion away from half filling",))
    for w in (6, 8) for inversion in (1, -1))

LARGE_PLAIN_CASES = (
    Case("sk_32_1 weight 4", sk_32_at_weight_4, (
        "lo_bits = 16: 256 rows of `before`, u16 entries",
        "a low class of C(16,4) = 1820 words > 1024 threads: the r0 loop runs twice")),
    Case("kagome_36 bonds weight 4", lambda: model_at_low_weight("heisenberg_kagome_36", 4, False), (
        "hi_bits = 20 > 16",
        "lo_bits = 16 and a low class of 1820 words")),
)

CHAIN_PLAIN_CASES = (
    Case("chain33 weight 3", lambda: long_chain(33), ("hi_bits = 17, odd n", "bonds of kind 1")),
    Case("chain35 weight 3", lambda: long_chain(35), ("hi_bits = 19, odd n", "bonds of kind 1")),
)

SMALL_PLAIN_CASES = tuple(
    Case("chain%d weight %d" % (n, w), lambda n=n, w=w: small_chain(n, w), (
        "lo_bits = %d < 8: rank8 filled for fewer than 256 values" % plain_word_bits(n)[0],
        "weights 0 and n: one state") + (("n = %d: one-bit words" % n,) if n < 4 else ()))
    for n in (2, 3, 5, 10, 13) for w in range(n + 1))

PLAIN_CASES = LARGE_PLAIN_CASES + CHAIN_PLAIN_CASES + SMALL_PLAIN_CASES


# -- host references, built once per process --------------------------------------------------------
class Host:
    """The host route's view of a case: basis states, norms, the matrix of `to_sparse` (real CSR;
    entry [i, j] = <state i| H |state j>) and, per source state, how many off-diagonal connections
    end inside the basis (the filled slots of the state's ELL row)."""

    def __init__(self, case, matrix=True):
        self.case = case
        self._energy = None
        op = self.operator = case.make()
        basis = op.basis
        basis.build()
        self.states = basis.states
        self.group = basis.group
        if self.group is not None:
            _, _, self.norms = self.group.state_info(self.states)
        else:
            self.norms = np.ones(self.states.shape[0])
        if not matrix:
            return
        # `to_sparse` itself, with the connections it is made of kept for the slot counts
        seen = []
        apply = op.batched_apply

        def once(spins):
            seen.append(apply(spins))
            return seen[-1]

        op.batched_apply = once
        try:
            h = op.to_sparse()
        finally:
            del op.batched_apply
        (other, coeffs, counts), = seen
        self.imaginary = float(abs(h.imag).max()) if h.nnz else 0.0
        self.h = h.real.tocsr()
        k = self.states.shape[0]
        source = np.repeat(np.arange(k), counts)
        at = np.minimum(np.searchsorted(self.states, other[:, 0]), k - 1)
        inside = self.states[at] == other[:, 0]
        inside[np.concatenate([[0], np.cumsum(counts)[:-1]])] = False   # the diagonal entries
        self.filled = np.bincount(source[inside], minlength=k)

    @property
    def largest(self):
        return float(abs(self.h).max()) if self.h.nnz else 0.0

    @property
    def largest_row_sum(self):
        return float(abs(self.h).sum(axis=1).max())

    @property
    def ground_state_energy(self):
        """scipy's lowest eigenvalue: dense below 2000 states, eigsh above."""
        if self._energy is None:
            if self.h.shape[0] < 2000:
                self._energy = float(np.linalg.eigvalsh(self.h.toarray())[0])
            else:
                import scipy.sparse.linalg

                self._energy = float(scipy.sparse.linalg.eigsh(self.h, k=1, which="SA", tol=1e-13)[0][0])
        return self._energy


@functools.lru_cache(maxsize=None)
def _host(name):
    for case in SECTOR_CASES + PLAIN_CASES:
        if case.name == name:
            return Host(case)
    for case in ENUMERATION_CASES:
        if case.name == name:
            return Host(case, matrix=False)
    raise KeyError(name)


def host(case):
    """The case's host reference: built on first use, shared by every test, never modified."""
    return _host(case.name)
