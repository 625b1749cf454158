"""The exact joint law of small tempering ensembles: sweeps (the ladder law of §4.10),
replica exchange (§4.12, ASP-PT-1) and isoenergetic cluster moves (§4.13, ASP-ICM-1) composed.

tests/tempering_law.py and tests/cluster_move_law.py restate the two ensemble moves with the product's
Philox counters and rounding and are compared with the kernels bit for bit; this module is independent of
them, of the kernels and of the oracle's annealer.  A handle of R slots is used as R/G independent groups
of G slots (exchange with parity 0 only, cluster pairs inside a group), and for a system of n <= 5 spins
the joint law of a group -- 2^(nG) float64 probabilities -- is propagated through the moves, following the
specification literally (for the 7 spins of P1 the law is kept per pair of slots, see ``Ensemble.forget``):

* one sweep of a slot at its beta: the proposals of sa_exact_law (accept with probability 1 if dE <= 0,
  0 if beta dE >= 23, exp(-beta dE) otherwise) in that sweep's order, on the current configuration;
* exchange of the slots (a, b) = (k, k+1): x = (beta_b - beta_a)(E_a - E_b); the configurations swap with
  probability 1 if x <= 0, 0 if x >= 23, exp(-x) otherwise; the betas stay with the slots;
* cluster move of a pair: D = c_a ^ c_b, nothing if D is empty; the seed site uniform over D; C = the
  component of the seed in the graph of A = offdiag(J + J^T) induced on D; both configurations ^= C.

The product draws u = (w + 1/2) 2^-32 and a seed floor(v n / 2^32) from 32-bit words and evaluates
expneg within 4e-16 of exp; each moves a probability by less than 1e-9, far below what 2^18 slots
resolve.

``WRONG_LAWS`` change one rule each.  ``CASES`` are the runs the GPU tests make (tests/test_gpu_ensemble_law.py);
tests/test_ensemble_law.py checks without a device that every one of them, at its sample count and on its
statistics, has the power to reject the wrong laws it lists, and proves the harness on ``sample``, a plain
numpy sampler of the same process.
"""
import numpy as np
import scipy.sparse
import scipy.stats

from sa_exact_law import (EMBED_AT, PASS_P, REJECT_P, X0, _acceptance, chi2_pvalue, colour_order,  # noqa: F401
                          embedded_system, energies, local_configs, shuffled_orders, system_p1)

WRONG_LAWS = {
    "A": "no exchange",
    "B": "the exchange accepts with the sign of x reversed",
    "C": "the exchange always swaps",
    "D": "the exchange cost uses beta_k in place of beta_{k+1} - beta_k",
    "E": "the cluster move flips the seed site only",
    "F": "the cluster move flips all differing sites",
    "G": "no cluster move",
    "H": "the cluster move is applied to replica a only",
    "I": "betas travel with the configurations in a swap",
}
_EXCHANGE_RULES = ("A", "B", "C", "D")
_CLUSTER_RULES = ("E", "F", "G", "H")

SEED = (1 << 41) + 0x2545F4914F     # >= 2**32: both Philox key words in use


def system_q():
    """n = 5: the path 0-1-2-3-4 with the chord 1-3.  The triangle 1-2-3 is frustrated (its three
    symmetrised couplings are positive), J is not symmetric and stores a diagonal, there is a field;
    every value is a multiple of 1/8 with |.| <= 2.  The differing set {0, 2, 3} induces the components
    {0} and {2, 3}: the seed's component, the whole set and the seed alone are three different moves."""
    n = 5
    J = np.zeros((n, n))
    edges = {(0, 1): (-1.0, 0.25), (1, 2): (0.5, 0.75), (2, 3): (1.0, -0.25), (1, 3): (0.625, 0.375),
             (3, 4): (0.5, 0.375)}
    for (i, j), (a, b) in edges.items():
        J[i, j], J[j, i] = a, b
    J[0, 0], J[2, 2] = 0.5, -0.25
    h = np.array([0.25, -0.375, 0.125, 0.5, -0.625])
    return J, h


def coupling_graph(J):
    """A = offdiag(J + J^T), dense (§4.2)."""
    J = np.asarray(J, dtype=np.float64)
    A = J + J.T
    np.fill_diagonal(A, 0.0)
    return A


# ----------------------------------------------------------------------------
# operators on probability vectors
# ----------------------------------------------------------------------------

def sweep_operator(E, beta, order):
    """K[c', c]: one sweep at ``beta`` visiting the spins in ``order`` takes configuration c to c'."""
    size = E.shape[0]
    idx = np.arange(size)
    K = np.eye(size)
    for i in order:
        bit = 1 << int(i)
        a = _acceptance(E[idx ^ bit] - E, beta, None)
        M = np.zeros((size, size))
        M[idx, idx] = 1.0 - a
        M[idx ^ bit, idx] += a
        K = M @ K
    return K


def swap_probability(E, beta_a, beta_b, rule=None):
    """s[a, b]: the pair in the configurations (a, b) at (beta_a, beta_b) swaps."""
    de = E[:, None] - E[None, :]
    x = (beta_a if rule == "D" else beta_b - beta_a) * de
    if rule == "B":
        x = -x
    s = np.where(x <= 0, 1.0, np.where(x >= 23.0, 0.0, np.exp(-np.clip(x, 0.0, 23.0))))
    if rule == "A":
        s = np.zeros_like(s)
    elif rule == "C":
        s = np.ones_like(s)
    return s


def exchange_parts(E, beta_a, beta_b, rule=None):
    """(stay, swap): the two sparse parts of the exchange operator on the joint index a * 2^n + b."""
    size = E.shape[0]
    s = swap_probability(E, beta_a, beta_b, rule).ravel()
    idx = np.arange(size * size)
    a, b = np.divmod(idx, size)
    shape = (size * size, size * size)
    stay = scipy.sparse.csr_matrix((1.0 - s, (idx, idx)), shape=shape)
    swap = scipy.sparse.csr_matrix((s, (b * size + a, idx)), shape=shape)
    return stay, swap


def exchange_operator(E, beta_a, beta_b, rule=None):
    stay, swap = exchange_parts(E, beta_a, beta_b, rule)
    return (stay + swap).tocsr()


def component_table(A, n):
    """comp[D, i]: the bit mask of the component of site i in the graph of A induced on the set D
    (0 where i is not in D)."""
    adj = [sum(1 << j for j in range(n) if j != i and A[i, j] != 0.0) for i in range(n)]
    comp = np.zeros((1 << n, n), dtype=np.int64)
    for D in range(1 << n):
        for i in range(n):
            if not (D >> i) & 1:
                continue
            C, frontier = 1 << i, [i]
            while frontier:
                j = frontier.pop()
                new = adj[j] & D & ~C
                C |= new
                frontier.extend(k for k in range(n) if (new >> k) & 1)
            comp[D, i] = C
    return comp


def _popcount(x):
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros_like(x)
    while np.any(x):
        out += x & 1
        x = x >> 1
    return out


def _flipped_set(comp, D, i, rule):
    if rule == "E":
        return np.full_like(D, 1 << i)
    if rule == "F":
        return D
    if rule == "G":
        return np.zeros_like(D)
    return comp[D, i]


def cluster_operator(A, n, rule=None):
    """Sparse operator of one cluster move on the joint index a * 2^n + b of a pair."""
    size = 1 << n
    comp = component_table(A, n)
    idx = np.arange(size * size)
    a, b = np.divmod(idx, size)
    D = a ^ b
    count = _popcount(D)
    same = D == 0
    rows, cols, vals = [idx[same]], [idx[same]], [np.ones(int(same.sum()))]
    for i in range(n):
        has = ((D >> i) & 1) == 1
        C = _flipped_set(comp, D[has], i, rule)
        rows.append((a[has] ^ C) * size + (b[has] ^ (0 if rule == "H" else C)))
        cols.append(idx[has])
        vals.append(1.0 / count[has])
    M = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                                shape=(size * size, size * size)).tocsr()
    M.sum_duplicates()
    return M


def cluster_report_law(A, n, pair_joint, rule=None, comp=None):
    """Law of (differing sites, cluster size) that the move reports from the pair's joint law before it,
    flattened as differing * (n + 1) + size.  comp: component_table(A, n), if the caller has it."""
    size = 1 << n
    comp = component_table(A, n) if comp is None else comp
    p = np.asarray(pair_joint, dtype=np.float64).ravel()
    idx = np.arange(size * size)
    a, b = np.divmod(idx, size)
    D = a ^ b
    count = _popcount(D)
    out = np.zeros((n + 1) * (n + 1))
    out[0] = p[D == 0].sum()
    for i in range(n):
        has = ((D >> i) & 1) == 1
        C = _flipped_set(comp, D[has], i, rule if rule in ("E", "F") else None)
        np.add.at(out, count[has] * (n + 1) + _popcount(C), p[has] / count[has])
    return out


def boltzmann(E, beta):
    w = np.exp(-beta * (E - E.min()))
    return w / w.sum()


class System:
    """A tiny system with its operators, cached."""

    def __init__(self, J, h, members=None, J_full=None):
        self.J, self.h = np.asarray(J, dtype=np.float64), np.asarray(h, dtype=np.float64)
        self.n = self.h.shape[0]
        self.size = 1 << self.n
        self.E = energies(self.J, self.h)
        self.A = coupling_graph(self.J)
        self.members = np.arange(self.n) if members is None else np.asarray(members)
        self.colour = colour_order(scipy.sparse.csr_matrix(self.J) if J_full is None else J_full, self.members)
        self._cache = {}

    def orders(self, order, count, seed=SEED):
        """The visiting orders of the sweeps 0 .. count-1 of a handle (local spin indices)."""
        if order == "colour":
            return [self.colour] * count
        return shuffled_orders(seed, count, self.members)

    def _cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def sweep(self, beta, order):
        return self._cached(("s", float(beta), tuple(int(i) for i in order)),
                            lambda: sweep_operator(self.E, beta, order))

    def swap(self, beta_a, beta_b, rule):
        return self._cached(("x", float(beta_a), float(beta_b), rule),
                            lambda: swap_probability(self.E, beta_a, beta_b, rule))

    def components(self):
        return self._cached("components", lambda: component_table(self.A, self.n))

    def cluster(self, rule):
        return self._cached(("c", rule), lambda: cluster_operator(self.A, self.n, rule))


# ----------------------------------------------------------------------------
# a G-slot ensemble
# ----------------------------------------------------------------------------

def _apply_axis(K, P, axis):
    return np.moveaxis(np.tensordot(K, P, axes=(1, axis)), 0, axis)


def _apply_pair(M, P, ax_a, ax_b):
    size = P.shape[0]
    Q = np.moveaxis(P, (ax_a, ax_b), (0, 1))
    shape = Q.shape
    Q = M @ Q.reshape(size * size, -1)
    return np.moveaxis(np.asarray(Q).reshape(shape), (0, 1), (ax_a, ax_b))


class Ensemble:
    """The joint law of a group of slots as independent factors.  A factor is a set of slots with
    ``parts``: {betas the slots sweep at (a tuple, one per slot of the factor): array of shape
    (2^n,) * len(slots)}.  Under the true law and every wrong law but "I" a factor has one part, keyed by
    its slots' own betas.  Factors merge (outer product) when a pair move joins them; that is exact while
    their slots are independent, which ``_component`` keeps track of.  ``forget`` replaces every factor
    by its slots' marginals: the joint law of a set of slots is changed only by moves that touch it, so
    factors formed afterwards from slots that were independent are again exact, while projections
    across factors are refused."""

    def __init__(self, system, betas, starts, rule=None):
        self.system, self.rule = system, rule
        self.betas = [float(b) for b in betas]
        self.G = len(self.betas)
        self.factors = []
        for g, start in enumerate(starts):
            p = np.zeros(system.size)
            if np.ndim(start) == 0:
                p[int(start)] = 1.0
            else:
                p[:] = start
            self.factors.append(((g,), {(self.betas[g],): p}))
        self._component = list(range(self.G))       # true dependence classes of the slots

    # -- bookkeeping of factors
    def _factor_of(self, slot):
        for k, (slots, _) in enumerate(self.factors):
            if slot in slots:
                return k
        raise KeyError(slot)

    def _join(self, pairs):
        """Make every pair of ``pairs`` lie inside one factor."""
        before = list(self._component)
        for a, b in pairs:
            ka, kb = self._factor_of(a), self._factor_of(b)
            if ka != kb:
                sa, pa = self.factors[ka]
                sb, pb = self.factors[kb]
                assert all(before[x] != before[y] for x in sa for y in sb), \
                    "slots %s and %s are not independent: their joint law was forgotten" % (sa, sb)
                parts = {}
                for keya, A in pa.items():
                    for keyb, B in pb.items():
                        parts[keya + keyb] = np.multiply.outer(A, B)
                self.factors = [f for k, f in enumerate(self.factors) if k not in (ka, kb)]
                self.factors.append((sa + sb, parts))
            ca, cb = self._component[a], self._component[b]
            self._component = [ca if c == cb else c for c in self._component]

    def forget(self):
        singles = []
        for slots, parts in self.factors:
            for ax, g in enumerate(slots):
                out = {}
                other = tuple(k for k in range(len(slots)) if k != ax)
                for key, P in parts.items():
                    out[(key[ax],)] = out.get((key[ax],), 0.0) + P.sum(axis=other)
                singles.append(((g,), out))
        self.factors = singles

    # -- the three moves
    def sweep(self, order):
        for slots, parts in self.factors:
            for key in list(parts):
                P = parts[key]
                for ax, g in enumerate(slots):
                    beta = key[ax] if self.rule == "I" else self.betas[g]
                    P = _apply_axis(self.system.sweep(beta, order), P, ax)
                parts[key] = P

    def exchange(self, pairs):
        """Exchange of every (a, b) of ``pairs``; returns the expected number of swaps."""
        self._join(pairs)
        rule = self.rule if self.rule in _EXCHANGE_RULES else None
        expected = 0.0
        for a, b in pairs:
            k = self._factor_of(a)
            slots, parts = self.factors[k]
            ax_a, ax_b = slots.index(a), slots.index(b)
            # the operator of exchange_parts, applied element by element: a cell keeps 1 - s of its mass and
            # sends s to the cell with the two configurations swapped
            s = self.system.swap(self.betas[a], self.betas[b], rule)
            if ax_a > ax_b:
                s = s.T
            shape = [1] * len(slots)
            shape[ax_a], shape[ax_b] = self.system.size, self.system.size
            s = s.reshape(shape)
            out = {}
            for key, P in parts.items():
                moved = np.swapaxes(P * s, ax_a, ax_b)
                expected += float(moved.sum())
                swapped = list(key)
                if self.rule == "I":
                    swapped[ax_a], swapped[ax_b] = key[ax_b], key[ax_a]
                swapped = tuple(swapped)
                out[key] = out.get(key, 0.0) + P * (1.0 - s)
                out[swapped] = out.get(swapped, 0.0) + moved
            self.factors[k] = (slots, out)
        return expected

    def cluster(self, pairs):
        """Cluster move of every (a, b) of ``pairs``; returns the law of the reported (differing, size)
        of each pair."""
        self._join(pairs)
        rule = self.rule if self.rule in _CLUSTER_RULES else None
        reports = []
        M = self.system.cluster(rule)
        for a, b in pairs:
            reports.append(cluster_report_law(self.system.A, self.system.n, self.pair(a, b), rule,
                                              self.system.components()))
            k = self._factor_of(a)
            slots, parts = self.factors[k]
            ax_a, ax_b = slots.index(a), slots.index(b)
            self.factors[k] = (slots, {key: _apply_pair(M, P, ax_a, ax_b) for key, P in parts.items()})
        return reports

    # -- projections
    def joint(self, slots):
        """The joint law of ``slots`` (inside one factor), an array with one axis per slot in that order."""
        k = self._factor_of(slots[0])
        have, parts = self.factors[k]
        assert all(s in have for s in slots), "slots %s are not in one factor" % (slots,)
        total = sum(parts.values())
        drop = tuple(ax for ax, g in enumerate(have) if g not in slots)
        kept = [g for g in have if g in slots]
        total = total.sum(axis=drop) if drop else total
        return np.transpose(total, [kept.index(s) for s in slots])

    def marginal(self, slot):
        return self.joint((slot,))

    def pair(self, a, b):
        return self.joint((a, b))


# ----------------------------------------------------------------------------
# the planned runs: one description, three interpreters (exact, numpy sampler, device)
# ----------------------------------------------------------------------------
# A case: G slots per group with ``betas`` and point-mass ``starts``; ``steps`` of
#   ("sweep", count) | ("exchange", draw) | ("cluster", pairs, draw) | ("forget",);
# exchange is parity 0 over the group: the pairs (0, 1), (2, 3), ...  ``groups``: the sample count N of
# the device run; ``joints``: the slot tuples whose joint law is compared at the end, beside every
# slot's marginal; ``laws``: {order: the wrong laws that run must reject}, with the reason where one is
# left out.

def _system_q():
    return System(*system_q())


_systems = {}


def system(name):
    if name not in _systems:
        if name == "Q":
            _systems[name] = _system_q()
        else:
            J, _, _, _ = embedded_system()
            _systems[name] = System(*system_p1(), members=EMBED_AT, J_full=J)
    return _systems[name]


CASES = {
    # hot slot 0 starts low (E = -3.25, the first excited level), cold slot 1 starts at the top (E = 5.5): the first
    # exchange is decisive
    "pairs": dict(
        system="Q", betas=(0.3, 1.5), starts=(18, 1), groups=1 << 17,
        steps=[("sweep", 1), ("exchange", 0), ("sweep", 1), ("exchange", 0), ("sweep", 2), ("exchange", 0),
               ("exchange", 1), ("sweep", 1), ("exchange", 0)],
        joints=[(0, 1)],
        # no cluster move in this case: E-H do not apply
        laws={"colour": "ABCDI", "shuffled": "ABCDI"}),
    # the driver's hairpin in miniature.  The starts of each cluster pair differ on a set that induces two
    # components -- slots (0, 3) on {0, 2, 3}: {0} and {2, 3}; slots (1, 2) on {0, 1, 4}: {0, 1} and {4} --
    # and the first move comes before any sweep, so E and F act at once; the second round moves twice at
    # one sweep count, with draws 0 and 1
    "hairpin": dict(
        system="Q", betas=(0.4, 1.25, 1.25, 0.4), starts=(18, 1, 18, 31), groups=1 << 16,
        steps=[("cluster", [(0, 3), (1, 2)], 0), ("sweep", 1), ("cluster", [(0, 3), (1, 2)], 0), ("exchange", 0),
               ("sweep", 1), ("cluster", [(0, 3), (1, 2)], 0), ("cluster", [(0, 3), (1, 2)], 1), ("exchange", 0),
               ("sweep", 2), ("cluster", [(0, 3), (1, 2)], 0), ("exchange", 0),
               ("sweep", 1), ("cluster", [(0, 3), (1, 2)], 0), ("exchange", 0)],
        joints=[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)],
        laws={"colour": "ABCDEFGHI", "shuffled": "ABCDEFGHI"}),
    # P1 (7 spins): a group of four is 2^28 states, so the exchange rounds run inside the pairs (0, 1) and
    # (2, 3), their joint law is then forgotten, and the cluster move joins (0, 3) and (1, 2), whose slots
    # are independent at that point; only sweeps follow.  Hot slot 0 starts at X0["P1"] (E = -6.125), cold slot
    # 1 at the top (E = 8.875); the starts of (0, 3) differ on {1, 3, 4}, those of (1, 2) on {0, 4, 5}
    "embedded": dict(
        system="P1", betas=(0.25, 1.5, 1.5, 0.25), starts=(76, 104, 104 ^ 0x31, 76 ^ 0x1A), groups=1 << 13,
        steps=[("sweep", 1), ("exchange", 0), ("sweep", 1), ("exchange", 0), ("sweep", 1), ("forget",),
               ("cluster", [(0, 3), (1, 2)], 0), ("sweep", 1)],
        joints=[],
        laws={"colour": "ABCDEFGHI", "shuffled": "ABCDEFGHI"}),
}


def stat_names(case):
    G = len(case["betas"])
    names = ["m%d" % g for g in range(G)] + ["j" + "".join(map(str, j)) for j in case["joints"]]
    for k, step in enumerate(case["steps"]):
        if step[0] == "cluster":
            names += ["r%d_%d%d" % (k, a, b) for a, b in step[1]]
    return names


class Stats:
    """probs: {statistic name: law over its cells}; accepted: the expected swaps per group of every
    exchange step, in order."""

    def __init__(self, probs, accepted):
        self.probs, self.accepted = probs, accepted


def number_of_sweeps(case):
    return sum(step[1] for step in case["steps"] if step[0] == "sweep")


def exact(case, order, rule=None, seed=SEED):
    """The exact statistics of one group of ``case`` in the sweep order ``order`` under ``rule``."""
    sys_ = system(case["system"])
    orders = sys_.orders(order, number_of_sweeps(case), seed)
    G = len(case["betas"])
    ens = Ensemble(sys_, case["betas"], case["starts"], rule)
    probs, accepted = {}, []
    t = 0
    for k, step in enumerate(case["steps"]):
        if step[0] == "sweep":
            for _ in range(step[1]):
                ens.sweep(orders[t])
                t += 1
        elif step[0] == "exchange":
            accepted.append(ens.exchange([(g, g + 1) for g in range(0, G - 1, 2)]))
        elif step[0] == "cluster":
            for (a, b), law in zip(step[1], ens.cluster(step[1])):
                probs["r%d_%d%d" % (k, a, b)] = law
        else:
            ens.forget()
    for g in range(G):
        probs["m%d" % g] = ens.marginal(g)
    for j in case["joints"]:
        probs["j" + "".join(map(str, j))] = ens.joint(tuple(j)).ravel()
    return Stats(probs, accepted)


def counts(case, configs, reports):
    """The observed counterpart of Stats.probs.  configs: int64[N, G] final local configurations of the
    groups; reports: {step index: (differing[N, pairs], sizes[N, pairs])}."""
    sys_ = system(case["system"])
    size, n = sys_.size, sys_.n
    out = {}
    for g in range(configs.shape[1]):
        out["m%d" % g] = np.bincount(configs[:, g], minlength=size)
    for j in case["joints"]:
        flat = np.zeros(configs.shape[0], dtype=np.int64)
        for g in j:
            flat = flat * size + configs[:, g]
        out["j" + "".join(map(str, j))] = np.bincount(flat, minlength=size ** len(j))
    for k, step in enumerate(case["steps"]):
        if step[0] == "cluster":
            differing, sizes = reports[k]
            for col, (a, b) in enumerate(step[1]):
                cell = differing[:, col].astype(np.int64) * (n + 1) + sizes[:, col].astype(np.int64)
                out["r%d_%d%d" % (k, a, b)] = np.bincount(cell, minlength=(n + 1) ** 2)
    return out


def pvalues(observed, stats):
    return {name: chi2_pvalue(observed[name], stats.probs[name]) for name in stats.probs}


def rejection_bound(p_true, p_wrong, N):
    """An upper bound, six standard deviations out, on the p-value that N samples of ``p_true`` give
    against ``p_wrong`` with the pooling of chi2_pvalue: chi2.sf(df + lam - 6 sqrt(2 df + 4 lam), df) with
    the noncentrality lam = N sum (p_true - p_wrong)^2 / p_wrong over the pooled cells."""
    p_true, p_wrong = np.asarray(p_true, dtype=np.float64), np.asarray(p_wrong, dtype=np.float64)
    big = p_wrong * N >= 5
    t, w = list(p_true[big]), list(p_wrong[big])
    rest_t, rest_w = p_true[~big].sum(), p_wrong[~big].sum()
    if rest_w > 0:
        t.append(rest_t)
        w.append(rest_w)
    elif rest_t * N >= 64:
        return 0.0          # counts fall where the wrong law has no mass, but for probability e^-64
    t, w = np.array(t), np.array(w)
    df = t.shape[0] - 1
    if df < 1:
        return 1.0
    lam = N * float(((t - w) ** 2 / w).sum())
    return float(scipy.stats.chi2.sf(df + lam - 6.0 * np.sqrt(2.0 * df + 4.0 * lam), df))


def power(case, true, wrong, N=None):
    """{statistic: rejection_bound}; the planned run rejects ``wrong`` if the smallest is <= REJECT_P."""
    N = case["groups"] if N is None else N
    return {name: rejection_bound(true.probs[name], wrong.probs[name], N) for name in true.probs}


def assert_case(label, case, laws, configs, reports, accepted, report=print, N=None):
    """laws: {None: true Stats, rule: wrong Stats}.  Every statistic follows the true law (the smallest p
    >= PASS_P), every wrong law is rejected by at least one (the smallest p <= REJECT_P), and the mean
    accepted swaps per group of every exchange step lie within 5 standard errors of the exact
    expectation.  accepted: float[steps, N]."""
    observed = counts(case, configs, reports)
    ps = {rule: min(pvalues(observed, stats).values()) for rule, stats in laws.items()}
    line = "%s: true law p = %.3g; wrong laws: %s" % (
        label, ps[None], ", ".join("%s p = %.3g" % (k, ps[k]) for k in sorted(k for k in ps if k is not None)))
    accepted = np.asarray(accepted, dtype=np.float64)
    swaps = []
    for row, want in zip(accepted, laws[None].accepted):
        se = max(row.std(ddof=1), 1e-300) / np.sqrt(row.shape[0])
        swaps.append((row.mean(), want, (row.mean() - want) / se if row.mean() != want else 0.0))
    line += "; accepted swaps per group " + ", ".join("%.5f (exact %.5f, %+.1f s.e.)" % s for s in swaps)
    sizes = []
    n = system(case["system"]).n
    cells = np.arange((n + 1) ** 2) % (n + 1)
    for name in [k for k in stat_names(case) if k.startswith("r")]:
        sizes.append("%s %.5f (exact %.5f)" % (name, float(cells @ observed[name]) / observed[name].sum(),
                                               float(cells @ laws[None].probs[name])))
    if sizes:
        line += "; mean cluster size " + ", ".join(sizes)
    report(line)
    assert ps[None] >= PASS_P, line
    for rule in ps:
        if rule is not None:
            assert ps[rule] <= REJECT_P, "wrong law %s (%s) not rejected: %s" % (rule, WRONG_LAWS[rule], line)
    for mean, want, z in swaps:
        assert abs(z) <= 5.0, line


# ----------------------------------------------------------------------------
# a plain numpy sampler of the same process
# ----------------------------------------------------------------------------

def sample(case, order, N, rng, rule=None, seed=SEED):
    """N independent groups of ``case`` with randomness from ``rng`` (numpy.random.Generator) alone; the
    visiting orders are the run's, an input like the betas.
    Returns (configs int64[N, G], reports {step: (differing[N, P], sizes[N, P])}, accepted float[steps, N])."""
    sys_ = system(case["system"])
    E, n = sys_.E, sys_.n
    adj = np.array([sum(1 << j for j in range(n) if j != i and sys_.A[i, j] != 0.0) for i in range(n)])
    orders = sys_.orders(order, number_of_sweeps(case), seed)
    G = len(case["betas"])
    c = np.tile(np.asarray(case["starts"], dtype=np.int64), (N, 1))
    beta = np.tile(np.asarray(case["betas"], dtype=np.float64), (N, 1))     # what each slot sweeps at
    slot_beta = np.asarray(case["betas"], dtype=np.float64)
    reports, accepted = {}, []
    t = 0
    for k, step in enumerate(case["steps"]):
        if step[0] == "sweep":
            for _ in range(step[1]):
                for i in orders[t]:
                    bit = 1 << int(i)
                    de = E[c ^ bit] - E[c]
                    x = beta * de
                    p = np.where(de <= 0, 1.0, np.where(x >= 23.0, 0.0, np.exp(-np.clip(x, 0.0, 23.0))))
                    c = np.where(rng.random(c.shape) < p, c ^ bit, c)
                t += 1
        elif step[0] == "exchange":
            swaps = np.zeros(N)
            for a in range(0, G - 1, 2):
                b = a + 1
                de = E[c[:, a]] - E[c[:, b]]
                x = (slot_beta[a] if rule == "D" else slot_beta[b] - slot_beta[a]) * de
                if rule == "B":
                    x = -x
                p = np.where(x <= 0, 1.0, np.where(x >= 23.0, 0.0, np.exp(-np.clip(x, 0.0, 23.0))))
                if rule == "A":
                    p = np.zeros(N)
                elif rule == "C":
                    p = np.ones(N)
                go = rng.random(N) < p
                swaps += go
                c[go, a], c[go, b] = c[go, b], c[go, a]
                if rule == "I":
                    beta[go, a], beta[go, b] = beta[go, b], beta[go, a]
            accepted.append(swaps)
        elif step[0] == "cluster":
            differing = np.zeros((N, len(step[1])), dtype=np.int64)
            sizes = np.zeros((N, len(step[1])), dtype=np.int64)
            for col, (a, b) in enumerate(step[1]):
                D = c[:, a] ^ c[:, b]
                count = _popcount(D)
                pick = np.floor(rng.random(N) * count).astype(np.int64)     # the pick-th set bit
                seed_site = np.zeros(N, dtype=np.int64)
                seen = np.zeros(N, dtype=np.int64)
                for i in range(n):
                    here = ((D >> i) & 1) == 1
                    seed_site = np.where(here & (seen == pick), i, seed_site)
                    seen += here
                C = np.where(count > 0, np.int64(1) << seed_site, 0)
                if rule == "F":
                    C = D.copy()
                elif rule != "E":
                    for _ in range(n):
                        grow = np.zeros(N, dtype=np.int64)
                        for i in range(n):
                            grow |= np.where((C >> i) & 1 == 1, adj[i], 0)
                        C = C | (grow & D)
                differing[:, col], sizes[:, col] = count, _popcount(C)
                if rule == "G":
                    continue
                c[:, a] ^= C
                if rule != "H":
                    c[:, b] ^= C
            reports[k] = (differing, sizes)
    return c, reports, np.array(accepted)


_exact = {}


def exact_cached(name, order, rule=None):
    """exact(CASES[name], order, rule), computed once per process."""
    key = (name, order, rule)
    if key not in _exact:
        _exact[key] = exact(CASES[name], order, rule)
    return _exact[key]


def laws_of(name, order):
    """{None: the true Stats, rule: the Stats of every wrong law the run must reject}."""
    return {rule: exact_cached(name, order, rule) for rule in [None] + list(CASES[name]["laws"][order])}


# ----------------------------------------------------------------------------
# the invariance run: the loop of parallel_tempering_cluster on a ladder of three betas
# ----------------------------------------------------------------------------
# slot k runs at INVARIANCE_BETAS[k % 3], so both parities pair slots of different beta; the cluster pairs
# (6m + j, 6m + j + 3), j = 0, 1, 2, join slots of equal beta.  beta dE <= 1.4 * 6.75 and |dbeta dE| <=
# 1.1 * 9.75 stay below 23: no acceptance is cut off and the product Boltzmann measure is invariant.
INVARIANCE_BETAS = (0.3, 1.4, 0.8)
INVARIANCE_ROUNDS = 4
INVARIANCE_SWEEPS = 2


def invariance_plan(R):
    """(betas float64[R], pairs uint32[P, 2]) of the invariance run on R slots."""
    betas = np.array([INVARIANCE_BETAS[k % 3] for k in range(R)])
    base = np.arange(0, R - 5, 6)
    pairs = (base[:, None, None] + np.array([[0, 3], [1, 4], [2, 5]])[None]).reshape(-1, 2)
    return betas, pairs.astype(np.uint32)
