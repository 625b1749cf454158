"""Chosen models for the greedy solver's strict descent — flip iff `dE < 0`, in colour order, until a sweep
flips nothing — and an exact reference of it: the inputs of
tests/test_descent_cases.py (conditions on them, no GPU) and tests/test_gpu_descent_boundaries.py (every
descent path against the reference).  Only the oracle is asked here (the colour order, the tree); the
package is never imported.  Every array a case hands out is frozen.

The descent's other tests draw couplings from a continuous distribution, where no proposal lands on
`dE == 0`, and take their sweep counts from what random clusters give.  Here every coupling and field is a
dyadic rational chosen so that every sum the kernels form is EXACT whatever its order (`rows_are_exact`),
so the expected configuration is a matter of decisions alone, and the families put the decisions where the
rule's four statements (csrc/sa_sweep.hip: the accept phase twice, the team kernel; csrc/sa_colour.hpp: the
field cache's inert rule) and the chunk / replay bookkeeping of the single path (csrc/sa_anneal.hip:
greedy_relax) could go wrong unseen:

  ties         random graphs of even degree d (d / 2 random cycles through all spins), couplings +-1, no
               field: 14-24 % of the visits of the descent have dE == 0 (+0.0 and -0.0 alike);
  ties_field   the same graphs with h_i = -sum_j A_ij s_j (s: the tree's signs) on half the spins: g = 0 from
               a non-zero cancellation, for both signs of the sum and both spin values; one more spin carries
               an anchor field that keeps the tree's orientation (step 3 of §4.8);
  one_step     127 triangles (a, b, p): A_ab = 4 fixes s_a = -s_b, A_pa = A_pb = 1, so p's row sum is exactly
               0, and h_p is +q, -q (q = 2^-51, the smallest step for which every partial sum of the row is
               exact) or 0: `s_p h_p > 0` must flip, the other side and the centre must stay.  The roles
               rotate through the triangle's three colours; a probe of each side sits at lanes 0, 1, 31, 62, 63
               of a colour's first block and at lanes 0, 1, 31, 61, 62 of its padded last block of 63 spins
               (the "mirror" model negates every h_p: the other side at the same lanes);
  domino       a ferromagnetic chain A_{i,i+1} = -w with h = +eps everywhere, a trigger h_0 = 4w and an anchor
               h_{n-1} = -(n + 10) 4w: the tree has every spin up and the descent unzips two spins a sweep, so
               the chain's length chooses t, here every t in DOMINO_T around the single path's chunks of 8;
               without the trigger the tree is a minimum (t = 1); with h_k = 0 at one interior spin the
               cascade must end there (the two bonds cancel: dE == 0); one chain beside a tie graph (its
               blocks are still from the second sweep on), and one beside 300 spins without couplings,
               where a sweep's two flips are below the field cache's entry threshold (0.7 blocks / mean
               degree = 4; csrc/sa_sweep.hip: cache_enter_flips_of) and the descent runs in cached mode;
  cancelling   J_ij = 1, J_ji = -1 beside real bonds: A_ij = 0, no bond — the model without the pair;
  scaled       one tie graph and one chain times 2^-300 and 2^300 (tests/test_gpu_sa_visit.py: SCALES).

RECORDED holds what the reference measured per case — (t, flips, visits with dE == 0, visits) — and
tests/test_descent_cases.py compares it with the reference again."""
import fractions

import numpy as np
import scipy.sparse

import oracle

Fraction = fractions.Fraction
CAP = 10000  # the solver's default max_sweeps
Q = 2.0 ** -51
DOMINO_T = (2, 7, 8, 9, 10, 15, 16, 17, 18)
SCALES = {"tiny": -300, "huge": 300}  # tests/test_gpu_sa_visit.py: SCALES (0 is every other case)
ONE_STEP_TRIANGLES = 127              # per colour: a block of 64 and a padded block of 63
FIRST_LANES, LAST_LANES = (0, 1, 31, 62, 63), (0, 1, 31, 61, 62)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def csr(matrix):
    m = scipy.sparse.csr_matrix(matrix, dtype=np.float64)
    m.sum_duplicates()
    m.sort_indices()
    return m


def spins_of(words, n):
    """+-1 per spin of a packed configuration (bit = +1)."""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8), bitorder="little")[:n]
    return [1 if b else -1 for b in bits.tolist()]


def words_of(s):
    bits = np.array([1 if v > 0 else 0 for v in s], np.uint8)
    padded = np.zeros((len(s) + 63) // 64 * 64, np.uint8)
    padded[:len(s)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64).copy()


# ---------------------------------------------------------------------------------------------
# The exact reference
# ---------------------------------------------------------------------------------------------

class Model:
    """A = offdiag(J + J^T) with the entries that sum to exactly 0 dropped, and h, as integers over one
    denominator (every double is a dyadic rational): rows[i] = [(j, A_ij den)], field[i] = h_i den."""

    def __init__(self, J, h):
        J = csr(J)
        self.n = n = J.shape[0]
        coo = J.tocoo()
        entries = {}
        for i, j, v in zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist()):
            if i != j:
                key = (min(i, j), max(i, j))
                entries[key] = entries.get(key, 0) + Fraction(v)
        field = [Fraction(float(v)) for v in np.asarray(h, np.float64).tolist()]
        self.diagonal = sum((Fraction(v) for i, j, v in zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist())
                             if i == j), Fraction(0))
        den = 1
        for v in list(entries.values()) + field:
            den = max(den, v.denominator)  # (powers of two)
        self.den = den
        self.rows = [[] for _ in range(n)]
        for (i, j), v in sorted(entries.items()):
            if v != 0:
                self.rows[i].append((j, int(v * den)))
                self.rows[j].append((i, int(v * den)))
        for row in self.rows:
            row.sort()
        self.field = [int(v * den) for v in field]

    def energy(self, s):
        """s^T J s + h^T s = D + sum_{i<j} A_ij s_i s_j + sum_i h_i s_i, a Fraction."""
        bonds = sum(a * s[i] * s[j] for i, row in enumerate(self.rows) for j, a in row if j > i)
        return self.diagonal + Fraction(bonds + sum(f * v for f, v in zip(self.field, s)), self.den)


class Descent:
    def __init__(self, words, t, flips, ties, visits):
        self.words, self.t, self.flips, self.ties, self.visits = freeze(words), t, flips, ties, visits

    def counts(self):
        return (self.t, self.flips, self.ties, self.visits)


def exact_descent(J, h, start, order, max_sweeps, rule="<"):
    """Strict-descent sweeps in exact arithmetic: g_i = sum_j A_ij s_j + h_i, dE = -2 s_i g_i, flip iff
    dE < 0 (rule "<=": iff dE <= 0, for the sensitivity check alone), the spins visited in `order`, from the
    packed configuration `start`, until a sweep flips nothing or max_sweeps sweeps are done.  Returns a
    Descent: the final words, t = sweeps performed (the index of the first sweep that flips nothing, or
    the cap), the flips and the visits with dE == 0."""
    assert rule in ("<", "<=")
    model = J if isinstance(J, Model) else Model(J, h)
    s = spins_of(start, model.n)
    order = [int(i) for i in order]
    assert sorted(order) == list(range(model.n))
    t = flips = ties = visits = 0
    while t < max_sweeps:
        flipped = False
        for i in order:
            g = model.field[i] + sum(a * s[j] for j, a in model.rows[i])
            de = -2 * s[i] * g
            visits += 1
            ties += de == 0
            if de < 0 or (rule == "<=" and de == 0):
                s[i] = -s[i]
                flips += 1
                flipped = True
        t += 1
        if not flipped:
            break
    return Descent(words_of(s), t, flips, ties, visits)


def rows_are_exact(J, h, seed=0, vectors=20):
    """The exactness condition: J_ij + J_ji is exact, and for every row the f64 sum of the terms A_ij s_j in
    ascending column order and then h_i, and the same sum from h_i backwards, both equal the exact sum — for
    all spins up, all down and `vectors` random sign vectors.  Returns the number of (row, vector) checks."""
    J = csr(J)
    model = Model(J, h)
    n, den = model.n, model.den
    dense = {}
    coo = J.tocoo()
    for i, j, v in zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist()):
        dense[i, j] = v
    values = []
    for i, row in enumerate(model.rows):
        floats = []
        for j, a in row:
            v = dense.get((i, j), 0.0) + dense.get((j, i), 0.0)
            assert Fraction(v) == Fraction(a, den), ("J_ij + J_ji is not exact", i, j)
            floats.append(v)
        values.append(floats)
    hs = np.asarray(h, np.float64).tolist()
    rng = np.random.default_rng(seed)
    signs = [[1] * n, [-1] * n] + [[1 if b else -1 for b in rng.integers(0, 2, n).tolist()] for _ in range(vectors)]
    checks = 0
    for s in signs:
        for i, row in enumerate(model.rows):
            terms = [v if s[j] > 0 else -v for (j, _), v in zip(row, values[i])]
            exact = Fraction(model.field[i] + sum(a * s[j] for j, a in row), den)
            forward = 0.0
            for x in terms:
                forward = forward + x
            forward = forward + hs[i]
            backward = hs[i]
            for x in reversed(terms):
                backward = backward + x
            assert Fraction(forward) == exact and Fraction(backward) == exact, ("row sum is not exact", i)
            checks += 1
    return checks


def energy_is_exact(model):
    """Every partial sum of the energy's terms, in any order, is a double: all of them are multiples of one
    power of two (half a coupling's unit: the energy's terms are s (acc / 2 + h)) and the sum of their
    magnitudes stays below 2^53 units."""
    if model.diagonal != 0:  # (no case has one)
        return False
    terms = [a for row in model.rows for _, a in row] + [2 * f for f in model.field]  # in units of 1 / (2 den)
    lows = [(v & -v).bit_length() - 1 for v in terms if v]
    return sum(abs(v) for v in terms) < 2 ** (53 + (min(lows) if lows else 0))


# ---------------------------------------------------------------------------------------------
# Builders: each returns (J, h)
# ---------------------------------------------------------------------------------------------

def ties(K, d, seed):
    """d / 2 random cycles through all K spins without a repeated bond, couplings +-1 stored on a random
    side of the diagonal, no field."""
    assert d % 2 == 0 and K >= 3
    rng = np.random.default_rng(seed)
    bonds = {}
    for _ in range(d // 2):
        while True:
            p = rng.permutation(K).tolist()
            pairs = [(min(a, b), max(a, b)) for a, b in zip(p, p[1:] + p[:1])]
            if len(set(pairs)) == K and not any(pair in bonds for pair in pairs):
                break
        for pair in pairs:
            bonds[pair] = 1.0 if rng.integers(0, 2) else -1.0
    rows, cols, vals = [], [], []
    for (i, j), w in sorted(bonds.items()):
        if rng.integers(0, 2):
            i, j = j, i
        rows.append(i), cols.append(j), vals.append(w)
    return csr(scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(K, K))), np.zeros(K)


def tree_of(J, h):
    return oracle.greedy_solve(J, h, relax=False)[0]


def ties_field(K, d, seed):
    """ties(K, d, seed) with h_i = -sum_j A_ij s_j on half the spins, s the tree's signs, and on one more
    spin the anchor -s_a (sum |h| + d + 1), which keeps the orientation of the tree (asserted) and the anchor
    itself where it is."""
    J, _ = ties(K, d, seed)
    s = spins_of(tree_of(J, np.zeros(K)), K)
    model = Model(J, np.zeros(K))
    rng = np.random.default_rng(seed + 1000)
    chosen = np.sort(rng.choice(K, K // 2, replace=False)).tolist()
    h = np.zeros(K)
    for i in chosen:
        h[i] = -float(sum(a * s[j] for j, a in model.rows[i]))
    anchor = min(set(range(K)) - set(chosen))
    h[anchor] = -s[anchor] * (np.abs(h).sum() + d + 1.0)
    assert spins_of(tree_of(J, h), K) == s, "the fields turned the tree"
    return J, h


def cancelled_field_kinds(J, h):
    """Of the spins with a non-zero field that cancels the row sum at the tree's configuration: the set of
    (sign of the sum, spin value) — all four for a ties_field case."""
    n = J.shape[0]
    model = Model(J, h)
    s = spins_of(tree_of(J, h), n)
    kinds = set()
    for i in range(n):
        acc = sum(a * s[j] for j, a in model.rows[i])
        if model.field[i] != 0 and acc + model.field[i] == 0:
            kinds.add((1 if acc > 0 else -1, s[i]))
    return kinds


def positions(J):
    """{spin: (colour, block of the colour, lane, blocks of the colour, spins of its last block)} from the
    oracle's visiting order: a colour class is cut into blocks of 64, the last one padded."""
    colors, order, ncol, _, _ = oracle.sa_layout(J)
    out, seen = {}, [0] * ncol
    size = np.bincount(colors, minlength=ncol)
    for spin in order.tolist():
        c = int(colors[spin])
        blocks = (int(size[c]) + 63) // 64
        out[spin] = (c, seen[c] // 64, seen[c] % 64, blocks, int(size[c]) - 64 * (blocks - 1))
        seen[c] += 1
    return out


def one_step(mirror=False):
    """The triangles of the module docstring.  Returns (J, h, probes): probes[k] = (spin p, h_p, flips),
    `flips`: the reference rule's decision, s_p h_p > 0, for the tree's s_p."""
    N = ONE_STEP_TRIANGLES
    K = 3 * N
    rows, cols, vals = [], [], []
    h = np.zeros(K)
    roles = []
    named = set(FIRST_LANES) | {64 + lane for lane in LAST_LANES}
    cycle, k_named = 0, 0
    kinds = {}
    for k in range(N):
        r = k % 3
        p, a, b = 3 * k + r, 3 * k + (r + 1) % 3, 3 * k + (r + 2) % 3
        roles.append((p, a, b))
        for (i, j, w) in ((a, b, 4.0), (p, a, 1.0), (p, b, 1.0)):
            if (k + i + j) % 2:
                i, j = j, i
            rows.append(i), cols.append(j), vals.append(w)
        h[a] = 2.0 if k % 2 else -2.0
        if k in named:  # (a probe one step to either side; which side flips depends on s_p)
            kinds[k] = Q if k_named % 2 == 0 else -Q
            k_named += 1
        else:
            kinds[k] = (Q, 0.0, -Q)[cycle % 3]
            cycle += 1
    J = csr(scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(K, K)))
    s = spins_of(tree_of(J, h), K)
    for k, (p, _, _) in enumerate(roles):
        # named probes: the first model's h_p makes even ones flip and odd ones stay, whatever s_p is
        if k in named:
            kinds[k] = abs(kinds[k]) * s[p] * (1.0 if kinds[k] > 0 else -1.0)
        h[p] = -kinds[k] if mirror else kinds[k]
    assert spins_of(tree_of(J, h), K) == s, "the probes' fields turned a tree"
    probes = [(p, float(h[p]), s[p] * h[p] > 0) for p, _, _ in roles]
    return J, h, probes


def domino(n, w=1.0, eps=0.125, trigger=True, stop=None):
    assert n >= 2
    i = np.arange(n - 1)
    J = csr(scipy.sparse.coo_matrix((np.full(n - 1, -w), (i, i + 1)), shape=(n, n)))
    h = np.full(n, eps)
    if trigger:
        h[0] = 4.0 * w
    h[n - 1] = -(n + 10) * 4.0 * w
    if stop is not None:
        assert 0 < stop < n - 1
        h[stop] = 0.0
    return J, h


def beside(first, second):
    """Two models as the diagonal blocks of one."""
    (J1, h1), (J2, h2) = first, second
    return csr(scipy.sparse.block_diag([J1, J2], format="csr")), np.concatenate([h1, h2])


def isolated(count):
    """Spins without couplings: half without a field (dE == 0 at every visit), the others with +-eps."""
    h = np.zeros(count)
    h[1::4], h[3::4] = 0.125, -0.125
    return scipy.sparse.csr_matrix((count, count)), h


def cancelling(K, d, seed, with_pair=True):
    """ties(K, d, seed), and J_ij = 1, J_ji = -1 for the first two spins that share no bond."""
    J, h = ties(K, d, seed)
    if not with_pair:
        return J, h
    dense = (J + J.T).toarray()
    i, j = next((i, j) for i in range(K) for j in range(i + 1, K) if dense[i, j] == 0.0)
    pair = scipy.sparse.coo_matrix(([1.0, -1.0], ([i, j], [j, i])), shape=(K, K))
    both = J.tocoo()
    rows = np.concatenate([both.row, pair.row])
    cols = np.concatenate([both.col, pair.col])
    vals = np.concatenate([both.data, pair.data])
    out = scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(K, K))  # (no duplicates: the pair is no bond)
    out.sort_indices()
    assert out.nnz == J.nnz + 2
    return out, h


def scaled(model, exponent):
    J, h = model
    return csr(J * 2.0 ** exponent), h * 2.0 ** exponent


# ---------------------------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------------------------

TIE_SIZES = ((63, 4), (63, 6), (64, 4), (64, 6), (65, 4), (65, 6), (130, 4), (130, 6), (257, 4), (257, 6))
# the seed of each graph: the first for which the reference meets the tie-share condition (at least 10 % of
# the visits at dE == 0, at least one flip), searched once (tests/test_descent_cases.py asserts the condition)
TIE_SEEDS = {(63, 4): 1, (63, 6): 1, (64, 4): 3, (64, 6): 1, (65, 4): 1, (65, 6): 1, (130, 4): 1, (130, 6): 1,
             (257, 4): 1, (257, 6): 1}
# ... and all four (sign of the sum, spin value) kinds of cancelled fields
FIELD_SEEDS = {(63, 4): 38, (63, 6): 4, (64, 4): 10, (64, 6): 24, (65, 4): 13, (65, 6): 29, (130, 4): 7, (130, 6): 4,
               (257, 4): 2, (257, 6): 3}
DOMINO_N = {2: 2, 7: 11, 8: 13, 9: 15, 10: 17, 15: 27, 16: 29, 17: 31, 18: 33}  # t -> the chain's length, searched once; the test takes every t from the reference
STOP_N, STOP_AT = 36, 20

BUILDERS = {}
FAMILY = {}


def _add(family, name, builder):
    BUILDERS[name] = builder
    FAMILY[name] = family


def _register():
    for K, d in TIE_SIZES:
        if (K, d) in TIE_SEEDS:
            _add("ties", "ties_%d_%d" % (K, d), lambda K=K, d=d: ties(K, d, TIE_SEEDS[K, d]))
        if (K, d) in FIELD_SEEDS:
            _add("ties_field", "ties_field_%d_%d" % (K, d), lambda K=K, d=d: ties_field(K, d, FIELD_SEEDS[K, d]))
    _add("one_step", "one_step", lambda: one_step()[:2])
    _add("one_step", "one_step_mirror", lambda: one_step(mirror=True)[:2])
    for t, n in sorted(DOMINO_N.items()):
        _add("domino", "domino_t%d" % t, lambda n=n: domino(n))
    _add("domino", "domino_t1", lambda: domino(12, trigger=False))
    _add("stop", "domino_stop", lambda: domino(STOP_N, stop=STOP_AT))
    if (257, 4) in TIE_SEEDS and 17 in DOMINO_N:
        _add("domino", "domino_beside_ties", lambda: beside(ties(257, 4, TIE_SEEDS[257, 4]), domino(DOMINO_N[17])))
    if 18 in DOMINO_N:
        _add("domino", "domino_cached", lambda: beside(domino(DOMINO_N[18]), isolated(300)))
    if (65, 4) in TIE_SEEDS:
        _add("cancelling", "cancelling_pair", lambda: cancelling(65, 4, TIE_SEEDS[65, 4]))
        for name, exponent in sorted(SCALES.items()):
            _add("scaled", "ties_65_4@" + name, lambda e=exponent: scaled(ties(65, 4, TIE_SEEDS[65, 4]), e))
    if 9 in DOMINO_N:
        for name, exponent in sorted(SCALES.items()):
            _add("scaled", "domino_t9@" + name, lambda e=exponent: scaled(domino(DOMINO_N[9]), e))


_register()

# name -> (t, flips, visits with dE == 0, visits) of the reference descent with the default cap
RECORDED = {
    "ties_63_4": (2, 2, 18, 126),
    "ties_field_63_4": (6, 17, 148, 378),
    "ties_63_6": (2, 1, 23, 126),
    "ties_field_63_6": (6, 30, 102, 378),
    "ties_64_4": (2, 2, 31, 128),
    "ties_field_64_4": (6, 13, 155, 384),
    "ties_64_6": (2, 4, 24, 128),
    "ties_field_64_6": (2, 1, 72, 128),
    "ties_65_4": (2, 1, 23, 130),
    "ties_field_65_4": (4, 4, 146, 260),
    "ties_65_6": (2, 1, 27, 130),
    "ties_field_65_6": (6, 19, 143, 390),
    "ties_130_4": (2, 2, 37, 260),
    "ties_field_130_4": (2, 1, 152, 260),
    "ties_130_6": (2, 3, 50, 260),
    "ties_field_130_6": (7, 43, 297, 910),
    "ties_257_4": (2, 4, 96, 514),
    "ties_field_257_4": (4, 9, 590, 1028),
    "ties_257_6": (2, 8, 97, 514),
    "ties_field_257_6": (10, 112, 722, 2570),
    "one_step": (2, 45, 78, 762),
    "one_step_mirror": (2, 43, 78, 762),
    "domino_t2": (2, 1, 0, 4),
    "domino_t7": (7, 10, 0, 77),
    "domino_t8": (8, 12, 0, 104),
    "domino_t9": (9, 14, 0, 135),
    "domino_t10": (10, 16, 0, 170),
    "domino_t15": (15, 26, 0, 405),
    "domino_t16": (16, 28, 0, 464),
    "domino_t17": (17, 30, 0, 527),
    "domino_t18": (18, 32, 0, 594),
    "domino_t1": (1, 0, 0, 12),
    "domino_stop": (12, 20, 2, 432),
    "domino_beside_ties": (17, 34, 786, 4896),
    "domino_cached": (18, 32, 2700, 5994),
    "cancelling_pair": (2, 1, 23, 130),
    "ties_65_4@huge": (2, 1, 23, 130),
    "ties_65_4@tiny": (2, 1, 23, 130),
    "domino_t9@huge": (9, 14, 0, 135),
    "domino_t9@tiny": (9, 14, 0, 135),
}


class Case:
    """One model with what only the oracle and the exact reference say about it: the visiting order, the
    tree's configuration, and the descent from it."""

    def __init__(self, name):
        self.name, self.family = name, FAMILY[name]
        J, h = BUILDERS[name]()
        self.J, self.h = csr(J), np.ascontiguousarray(h, np.float64)
        self.n = self.J.shape[0]
        self.order = oracle.sa_layout(self.J)[1]
        self.colours = oracle.sa_layout(self.J)[2]
        self.start = tree_of(self.J, self.h)
        self.model = Model(self.J, self.h)
        self.energy_exact = energy_is_exact(self.model)
        self._descents = {}
        freeze(self.J.data, self.J.indices, self.J.indptr, self.h, self.order, self.start)
        self.reference = self.descent(CAP)
        self.t = self.reference.t

    def descent(self, cap, rule="<"):
        if (cap, rule) not in self._descents:
            self._descents[cap, rule] = exact_descent(self.model, None, self.start, self.order, cap, rule)
        return self._descents[cap, rule]

    def energy(self, words):
        """The energy of a configuration as the double every implementation must report: the exact value
        where every partial sum of it is a double (asserted to be one); else (q = 2^-51 beside sums of
        hundreds: one_step) the oracle's statement of §4.6's summation tree, which the kernels equal bit
        for bit."""
        if self.energy_exact:
            e = self.model.energy(spins_of(words, self.n))
            assert Fraction(float(e)) == e
            return float(e)
        return float(oracle.sa_energy(self.J, self.h, words)[0])

    def expected(self, cap=CAP):
        """(words, energy, t) of the descent capped at `cap` sweeps."""
        d = self.descent(min(cap, self.t + 1))  # (a cap above t changes nothing)
        return d.words, self.energy(d.words), min(cap, self.t)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def names(*families):
    return [name for name in BUILDERS if not families or FAMILY[name] in families]
