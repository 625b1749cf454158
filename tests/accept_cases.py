"""Chosen (random word, x) pairs for the acceptance rule `u < expneg(x)`, u = (word + 0.5) 2^-32
(csrc/sa_device.hpp: metropolis_accept_word) — the inputs of
tests/test_accept_cases.py (conditions on them, no GPU) and tests/test_gpu_accept_boundaries.py (the
five compiled sites against the oracle).  Only the oracle decides here; of the package only the host
layout is asked, for a plan's energy scale.  Every array a case hands out is frozen.

A PROBE is a pair (word, x) put in front of the rule.  The random word of a proposal or of an exchange
pair is a function of the seed and of counters the caller controls, so a model whose spin i presents
exactly x_i (sweeps) or a ladder whose pair k presents exactly x_k (exchange) can aim x at the word:

  class 0, BOUNDARY: adjacent doubles xa < xb with accept at xa and reject at xb, found by bisection
           of `accepts` around x0 = -ln((word + 0.5) 2^-32), and 1, 2, 3 doubles beyond each;
  class 1, BAND LADDER: x = x0 - log1p(delta), i.e. expneg(x) = u (1 + delta), for the DELTAS below:
           fast accept, fast reject and the exact path from both sides of both edges of the filter's
           band of +-2e-5 (see DELTAS);
  class 2, EDGE: values of x that do not depend on the word (EDGE_X).

A word whose bisection fails gets a class-1 probe instead and is counted (`fallbacks`).

SWEEPS.  Spin i of the K probe spins has field h_i = -x_i / 2 and starts down; sweep 0 (t = 0) is
downhill for every spin and chain, and in sweep 1 spin i of chain r proposes dE = x_i exactly with word
r & 3 of Philox(i, 1, r >> 2, 0).  One chain per spin is DESIGNATED: x_i is built for its word (the
chain with the smallest word for half of the spins — large x —, the largest for an eighth — small
x —, chain i mod R for the rest); every other chain's decision is an ordinary random probe and is
compared all the same.  "isolated": no couplings between probe spins; "pairs": spins 2j and 2j + 1
coupled by 2^-200, which rn(acc + h) absorbs for every |h| >= 2^-140 (asserted), so the model has two
colours of probe spins and still presents x_i.

The annealer reports a chain's BEST configuration by tracked energy, and sweep 1 only moves uphill.  Two
more spins (GATE, HELPER, powers of two far above every accepted x) make the state after sweep 1 the
best one whatever was accepted: the helper flips at its visit of sweep 0 and turns the gate, which was a
certain rejection (x = 3 * 2^990) at its own earlier visit of sweep 0, downhill for sweep 1, where it
drops the energy by 2^990; the helper is a certain rejection from then on.  Which of the two indices is
visited first in sweep 0 depends on the order (colours, or the priorities of the shuffled sweep), so a
case is built for one order.
"""
import math

import numpy as np
import scipy.sparse

import oracle

TWO32 = 4294967296.0
# +-2e-6 is there for the host model of tests/test_accept_cases.py: a filter that misjudges by a factor
# (1 + 3e-6) outside |delta| <= 1e-6 changes a probe only for 1e-6 < |delta| < 3e-6 — strictly, since
# (1 - 3e-6)(1 + 3e-6) < 1 —, and 2e-6 is the only value in there
_MAGNITUDES = (1e-7, 3e-7, 1e-6, 2e-6, 3e-6, 1e-5, 1.5e-5, 1.8e-5, 2e-5, 2.2e-5, 2.5e-5, 3e-5, 1e-4)
DELTAS = tuple(s * m for m in _MAGNITUDES for s in (1.0, -1.0))
DBL_MAX = float(np.finfo(np.float64).max)
EDGE_X = (5e-324, 2.0 ** -1022, 1e-300, 2.0 ** -53, 2.0 ** -33 * (1 - 2.0 ** -20), 2.0 ** -33 * (1 + 2.0 ** -20),
          float(np.nextafter(23.0, 0.0)), 23.0, float(np.nextafter(23.0, 99.0)), 1e300, DBL_MAX)
ABSORBED = 2.0 ** -200   # the coupling of "pairs"
SMALLEST_PAIRED = 2.0 ** -140
BIG = 2.0 ** 990         # the gate's scale
SMALL_WORD = int(TWO32 * math.exp(-8.0))  # words below it have x0 > 8
BOUNDARY, LADDER, EDGE, RANDOM = 0, 1, 2, 3
CLASS_NAMES = ("boundary", "band ladder", "edge", "random")
BOUNDARY_STEPS = ((0, 0), (1, 0), (0, -1), (1, 1), (0, -2), (1, 2), (0, -3), (1, 3))  # (side, doubles beyond)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ---------------------------------------------------------------------------------------------
# Philox4x32-10 on arrays
# ---------------------------------------------------------------------------------------------

def philox(c0, c1, c2, c3, seed):
    """uint32[..., 4]: the four words of Philox4x32-10(counter (c0, c1, c2, c3), key seed)."""
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3)]
    low, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & low, p1 & low, ((p0 >> s32) ^ c3 ^ k1) & low, p0 & low
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & low, (k1 + np.uint64(0xBB67AE85)) & low
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def proposal_words(spins, t, replicas, seed):
    """uint32[len(spins), len(replicas)]: the word of spin i, sweep t, global replica r."""
    spins, replicas = np.asarray(spins, np.int64), np.asarray(replicas, np.int64)
    calls = np.unique(replicas >> 2)
    w = philox(spins[:, None], t, calls[None, :], 0, seed)            # [spins, calls, 4]
    return np.ascontiguousarray(w[:, np.searchsorted(calls, replicas >> 2), replicas & 3])


def exchange_words(pairs, sweeps_done, draw, seed):
    """uint32[len(pairs)]: word 0 of Philox(k, sweeps_done, 0xFFFFFFFC, draw)."""
    return np.ascontiguousarray(philox(np.asarray(pairs, np.int64), sweeps_done, 0xFFFFFFFC, draw, seed)[..., 0])


# ---------------------------------------------------------------------------------------------
# The rule, as the oracle states it, and the probes of one word
# ---------------------------------------------------------------------------------------------

def accepts(word, x):
    """x <= 0, or x < 23 and u < expneg(x) (tests/tempering_law.py: accepts)."""
    if x <= 0.0:
        return True
    if not x < 23.0:
        return False
    return (float(int(word)) + 0.5) * 2.0 ** -32 < oracle.expneg(x)


def accepts_with(word, x, exp):
    """The rule with another exp(-x) in the place of the oracle's."""
    return x <= 0.0 or (x < 23.0 and (float(int(word)) + 0.5) * 2.0 ** -32 < exp(x))


def _as_int(x):
    return int(np.float64(x).view(np.int64))


def _as_float(n):
    return float(np.int64(n).view(np.float64))


def boundary(word):
    """(xa, xb): adjacent doubles, accept at xa and reject at xb; None when the bisection has no
    bracket.  (Positive doubles are ordered like their bit patterns.)"""
    x0 = -math.log((float(int(word)) + 0.5) / TWO32)
    # a bracket of a few doubles first (x0 is the boundary up to the roundings of log and expneg), then
    # one of 1e-9: expneg 1e-9 above and below u, relatively
    for width in (8.0 * float(np.spacing(x0)) + 1e-15, 1e-9):
        lo, hi = x0 - width, x0 + width
        if 0.0 < lo and hi < 23.0 and accepts(word, lo) and not accepts(word, hi):
            break
    else:
        return None
    a, b = _as_int(lo), _as_int(hi)
    while b - a > 1:
        mid = (a + b) // 2
        if accepts(word, _as_float(mid)):
            a = mid
        else:
            b = mid
    return _as_float(a), _as_float(b)


def ladder_x(word, delta):
    return -math.log((float(int(word)) + 0.5) / TWO32) - math.log1p(delta)


def delta_of(word, x):
    """expneg(x) 2^32 / (word + 0.5) - 1: how far the word is from the decision, as the band counts it."""
    p = oracle.expneg(x) if x < 23.0 else 0.0
    return p * TWO32 / (float(int(word)) + 0.5) - 1.0


class Probes:
    """x[n], cls[n] and the oracle's decision accept[n] for n designated words, the class and its
    variant cyclic in `index`; `edge_x`: the edge values in use, `edge_once`: one more, used once."""

    def __init__(self, words, index, edge_x=EDGE_X, edge_once=None):
        n = len(words)
        self.words = np.asarray(words, np.uint32)
        self.x = np.zeros(n)
        self.cls = np.zeros(n, np.int8)
        self.fallbacks = 0
        for j in range(n):
            word, i = int(self.words[j]), int(index[j])
            cls, variant = i % 3, i // 3
            if cls == BOUNDARY:
                pair = boundary(word)
                if pair is None:
                    cls, self.fallbacks = LADDER, self.fallbacks + 1
                else:
                    side, steps = BOUNDARY_STEPS[variant % len(BOUNDARY_STEPS)]
                    x = pair[side]
                    for _ in range(abs(steps)):
                        x = float(np.nextafter(x, 99.0 if steps > 0 else 0.0))
            if cls == LADDER:
                x = ladder_x(word, DELTAS[variant % len(DELTAS)])
                if x <= 0.0:  # (a word next to 2^32: only the rejecting side exists)
                    x = ladder_x(word, -abs(DELTAS[variant % len(DELTAS)]))
            if cls == EDGE:
                x = edge_x[variant % len(edge_x)]
                if edge_once is not None:  # (the first edge probe)
                    x, edge_once = edge_once, None
            assert x > 0.0 and math.isfinite(x)
            self.x[j], self.cls[j] = x, cls
        p = np.array([oracle.expneg(x) if x < 23.0 else 0.0 for x in self.x.tolist()])  # (every x is > 0)
        u = (self.words.astype(np.float64) + 0.5) * 2.0 ** -32                          # (exact)
        self.accept = u < p                                                             # `accepts`
        self.delta = p * TWO32 / (self.words.astype(np.float64) + 0.5) - 1.0            # `delta_of`
        freeze(self.words, self.x, self.cls, self.accept, self.delta)

    def counts(self):
        """What tests/test_accept_cases.py asserts, and what DESIGN.md §4.4 lists."""
        aimed = self.cls != EDGE
        return {
            "probes": len(self.x),
            "boundary": int((self.cls == BOUNDARY).sum()),
            "bisected": int((self.cls == BOUNDARY).sum()) + self.fallbacks,
            "in_band": int((aimed & (np.abs(self.delta) <= 1.7e-5)).sum()),
            "x_above_8": int((self.x > 8.0).sum()),
            "x_above_8_aimed": int((aimed & (self.x > 8.0)).sum()),
            "x_below_1e-3": int((self.x < 1e-3).sum()),
            "x_below_1e-3_aimed": int((aimed & (self.x < 1e-3)).sum()),
            "accept_share": float(self.accept.mean()),
            "fallbacks": self.fallbacks,
        }

    def changed_by_exp(self, exp):
        """Boundary probes that another exp(-x) decides differently: (changed, boundary probes)."""
        rows = np.nonzero(self.cls == BOUNDARY)[0]
        changed = sum(accepts_with(self.words[j], self.x[j], exp) != self.accept[j] for j in rows)
        return int(changed), len(rows)

    def changed_by_misjudged_band(self, e):
        """Probes that a filter with a too-narrow band decides differently: accept iff word + 0.5 <
        p 2^32 (1 + e) outside |delta| <= 1e-6, the oracle inside."""
        rows = np.nonzero((self.cls != EDGE) & (np.abs(self.delta) > 1e-6))[0]
        changed = 0
        for j in rows:
            p = oracle.expneg(self.x[j]) if self.x[j] < 23.0 else 0.0
            changed += (float(self.words[j]) + 0.5 < p * TWO32 * (1.0 + e)) != self.accept[j]
        return int(changed)


# ---------------------------------------------------------------------------------------------
# Sweeps
# ---------------------------------------------------------------------------------------------

def _shuffled_first(a, b, sweep, seed):
    """Of spins a < b, the one the shuffled sweep `sweep` visits first: ascending (priority, index)."""
    pa, pb = (int(philox(i, sweep, 0xFFFFFFFE, 0, seed)[0]) for i in (a, b))
    return a if (pa, a) < (pb, b) else b


class SweepCase:
    """One model, one range of chains, one visiting order; see the module docstring.

    ladder = True: chain r of the range runs at beta_r = 2^((r mod 3) - 1) and h_i is divided by the
    designated chain's beta (exact; an edge x takes a designated chain at beta = 1)."""

    SEED = 777 + (3 << 32)
    T = 1  # the sweep that probes

    def __init__(self, model, spins, chains, first=0, order="colour", ladder=False):
        assert model in ("isolated", "pairs") and order in ("colour", "shuffled") and spins % 2 == 0
        self.model, self.order, self.ladder = model, order, ladder
        self.K, self.R, self.first, self.size = spins, chains, first, spins + 2
        replicas = first + np.arange(chains)
        self.words = proposal_words(np.arange(spins), self.T, replicas, self.SEED)
        self.chain_betas = np.ldexp(1.0, (np.arange(chains) % 3) - 1) if ladder else np.ones(chains)
        i = np.arange(spins)
        self.designated = np.where(i % 8 < 4, self.words.argmin(1), np.where(i % 8 == 4, self.words.argmax(1), i % chains))
        if ladder:  # an edge x goes to a chain at beta = 1: x / beta would not be exact at both ends
            self.designated = np.where(i % 3 == EDGE, 1 + 3 * ((i // 3) % (chains // 3)), self.designated)
        # dE = 2 |h| is an even multiple of the smallest subnormal: 1e-323 stands in for 5e-324; and one
        # spin only at the largest double: a plan needs a finite sum of |h|
        edge_x = tuple(max(x, 1e-323) for x in EDGE_X if (model == "isolated" or x >= SMALLEST_PAIRED) and x != DBL_MAX)
        self.probes = Probes(self.words[i, self.designated], i, edge_x, edge_once=DBL_MAX)
        beta = self.chain_betas[self.designated]
        self.de = self.probes.x / beta
        assert np.array_equal(self.de * beta, self.probes.x) and np.all(np.isfinite(self.de))
        field = np.zeros(self.size)
        field[:spins] = -0.5 * self.de
        assert np.array_equal(-2.0 * field[:spins], self.de)
        rows, cols, vals = [], [], []
        if model == "pairs":
            assert np.all(np.abs(field[:spins]) >= SMALLEST_PAIRED)
            for sign in (ABSORBED, -ABSORBED):
                assert np.array_equal(sign + field[:spins], field[:spins])
            rows, cols, vals = list(range(0, spins, 2)), list(range(1, spins, 2)), [ABSORBED] * (spins // 2)
        # the gate and its helper: module docstring
        a, b = spins, spins + 1
        J = scipy.sparse.csr_matrix((vals + [-BIG], (rows + [a], cols + [b])), shape=(self.size, self.size))
        if order == "colour":
            position = np.argsort(oracle.sa_layout(J)[1])
            gate = a if position[a] < position[b] else b
        else:
            gate = _shuffled_first(a, b, 0, self.SEED)
        field[gate], field[a + b - gate] = 0.5 * BIG, -2.0 * BIG
        self.gate, self.J, self.field = gate, J, field
        self.x0 = np.zeros((self.size + 63) // 64, np.uint64)
        self.betas = np.ones(2)
        freeze(self.words, self.chain_betas, self.designated, self.de, self.field, self.x0, self.betas)

    def presented(self, spin, chain):
        """(x, word, class name) of probe spin `spin` in chain `chain` of the range at sweep 1."""
        x = float(self.chain_betas[chain] * self.de[spin])
        name = CLASS_NAMES[self.probes.cls[spin] if chain == self.designated[spin] else RANDOM]
        return x, int(self.words[spin, chain]), name

    def expected_down(self):
        """bool[K, R]: the probe spins that are down after sweep 1 — the accepted proposals —, decided
        here by `accepts` (the designated ones: Probes.accept)."""
        down = np.zeros((self.K, self.R), bool)
        for r in range(self.R):
            beta = float(self.chain_betas[r])
            down[:, r] = [accepts(w, beta * float(de)) for w, de in zip(self.words[:, r], self.de)]
        return down


def host_scale(case):
    """(energy_scale_exp, colours, blocks) of the case's plan, from the library's host layout (no GPU) — the one
    place where this module calls the package."""
    import ctypes

    from annealing_sign_problem_amd import _lib

    info = _lib.SaInfo()
    colors = np.zeros(case.size, np.int32)
    position = np.zeros(case.size, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(
        case.size, _lib.ptr(np.ascontiguousarray(case.J.indptr, np.int64)),
        _lib.ptr(np.ascontiguousarray(case.J.indices, np.int32)), _lib.ptr(np.ascontiguousarray(case.J.data, np.float64)),
        _lib.ptr(np.ascontiguousarray(case.field)), ctypes.byref(info), _lib.ptr(colors), _lib.ptr(position)))
    return info.energy_scale_exp, info.num_colors, info.num_blocks


# ---------------------------------------------------------------------------------------------
# Exchange
# ---------------------------------------------------------------------------------------------

class ExchangeCase:
    """A handle of R chains on the plan K = 1, J empty, h = [0.5]: even slots up (E = 0.5), odd slots down
    (E = -0.5), so E_k - E_{k+1} = +-1 exactly, and with 0 on the even and x on the odd slots of the ladder
    pair k presents exactly x.  One probe per (parity, draw, pair), classes cyclic in the pair and the draw."""

    SEED = 4242 + (9 << 32)
    SWEEPS_DONE = 0

    def __init__(self, chains, draws):
        self.R, self.draws = chains, tuple(draws)
        self.energies = freeze(np.where(np.arange(chains) % 2 == 0, 0.5, -0.5))
        self.x0 = freeze((np.arange(chains) % 2 == 0).astype(np.uint64).reshape(chains, 1))
        self.steps = {}
        for parity in (0, 1):
            pairs = np.arange(parity, chains - 1, 2)
            words = np.stack([exchange_words(pairs, self.SWEEPS_DONE, draw, self.SEED) for draw in self.draws])
            index = pairs[None, :] // 2 + 5 * np.arange(len(self.draws))[:, None]
            # the draws with a pair's three largest words are boundary probes: at their small x adjacent doubles
            # are less than an ulp of expneg apart, where a wrong last bit of expneg shows most often
            for largest in np.argsort(words, axis=0)[-3:]:
                index[largest, np.arange(len(pairs))] -= index[largest, np.arange(len(pairs))] % 3
            # ... and no word small enough for x > 8 (one in 3000) is spent on an edge value
            index[(words < SMALL_WORD) & (index % 3 == EDGE)] += 1
            for n, draw in enumerate(self.draws):
                probes = Probes(words[n], index[n])
                betas = np.zeros(chains)
                betas[pairs + 1 - parity] = probes.x  # the odd slot of the pair
                self.steps[parity, draw] = (freeze(pairs), probes, freeze(betas))

    def expected(self, parity, draw):
        """(source uint32[R], accepted) of the step: tempering_law's steps 2-5 with this module's words."""
        import tempering_law

        pairs, probes, betas = self.steps[parity, draw]
        source, accepted = tempering_law.select(self.energies, betas, parity, dict(zip(pairs.tolist(), probes.words)))
        return np.array(source, np.uint32), accepted

    def all_probes(self):
        return [probes for _, probes, _ in self.steps.values()]

    def counts(self):
        total = {}
        for probes in self.all_probes():
            for name, value in probes.counts().items():
                total[name] = total.get(name, 0) + value
        total["accept_share"] /= len(self.steps)
        return total


# ---------------------------------------------------------------------------------------------
# Resample weights
# ---------------------------------------------------------------------------------------------

WEIGHT_SPINS = 40
WEIGHT_GRID = 2.0 ** -35  # every gap of the model is a multiple of it


def weight_case(seed=11):
    """K = 40, J empty, h_i = 16 * 2^-(i + 1): every energy is an exact dyadic, and with chain 0 all down
    (the minimum) chain r's gap is m_r * 2^-35, bit 39 - i of m_r = spin i up.  Gaps: 0, the smallest one,
    23 and the grid point below it, and the grid points on either side of -ln(q 2^-31) — where floor(expneg(gap) 2^31) steps from q
    to q - 1 — for q = 1 .. 64 and 200 random q < 2^31.  Returns (field, x0 uint64[R, 1], gaps)."""
    rng = np.random.default_rng(seed)
    qs = list(range(1, 65)) + [int(q) for q in rng.integers(65, 2 ** 31, 200)]
    at_23 = int(23.0 / WEIGHT_GRID)
    m = [0, 1, at_23 - 1, at_23]
    for q in qs:
        below = int(math.floor(-math.log(q * 2.0 ** -31) / WEIGHT_GRID))
        m += [below, below + 1]
    m = np.array(m, np.uint64)
    assert m.max() < 2 ** WEIGHT_SPINS
    field = 16.0 * np.ldexp(1.0, -(np.arange(WEIGHT_SPINS) + 1))
    x0 = np.zeros(len(m), np.uint64)
    for i in range(WEIGHT_SPINS):
        x0 |= ((m >> np.uint64(WEIGHT_SPINS - 1 - i)) & np.uint64(1)) << np.uint64(i)
    gaps = m.astype(np.float64) * WEIGHT_GRID
    return freeze(field, x0.reshape(-1, 1), gaps)


# ---------------------------------------------------------------------------------------------
# The cases both test files use, built on first use
# ---------------------------------------------------------------------------------------------

SPINS, CHAINS = 16382, 128  # (+ gate and helper: 16384 spins)
SWEEP_CASES = {
    "isolated": dict(model="isolated", spins=SPINS, chains=CHAINS),
    "isolated_from_3": dict(model="isolated", spins=SPINS, chains=CHAINS, first=3),
    "pairs": dict(model="pairs", spins=SPINS, chains=CHAINS),
    "isolated_shuffled": dict(model="isolated", spins=SPINS, chains=CHAINS, order="shuffled"),
    "pairs_shuffled": dict(model="pairs", spins=SPINS, chains=CHAINS, order="shuffled"),
    "ladder": dict(model="isolated", spins=SPINS, chains=CHAINS, ladder=True),
    "ladder_shuffled": dict(model="isolated", spins=SPINS, chains=CHAINS, order="shuffled", ladder=True),
}
EXCHANGE_CHAINS, EXCHANGE_DRAWS = 16384, tuple(range(24))  # (16 draws hold ~88 words with x0 > 8)
_cache = {}


def sweep_case(name):
    if name not in _cache:
        _cache[name] = SweepCase(**SWEEP_CASES[name])
    return _cache[name]


def exchange_case(chains=EXCHANGE_CHAINS, draws=EXCHANGE_DRAWS):
    if ("exchange", chains, tuple(draws)) not in _cache:
        _cache["exchange", chains, tuple(draws)] = ExchangeCase(chains, draws)
    return _cache["exchange", chains, tuple(draws)]
