"""The exact Markov law of the annealer (ASP-SA-1 / ASP-SA-1S) on a tiny system.

Every other annealer test compares the kernels with oracle/sa_oracle.c bit for bit; this module
is independent of both.  For a system of n <= 8 spins it propagates the exact distribution of the
joint state (current configuration, best configuration) -- 2^n x 2^n float64 probabilities --
through the sweeps, following the specification literally:

* configuration bit i set means s_i = +1 (§4.3); E(c) = s^T J s + h^T s with J's diagonal
  included and J not necessarily symmetric.  With dyadic couplings and fields every E and every
  dE = E(c ^ 2^i) - E(c) is exact;
* one proposal of spin i at beta: accept with probability 1 if dE <= 0; with probability 0 if
  beta * dE >= 23 (beta = +inf included); exp(-beta * dE) otherwise.  The product draws
  u = (w + 1/2) 2^-32 from a 32-bit word w and compares it with expneg(beta * dE), which is
  within 4e-16 relative of exp(-beta * dE); both move an acceptance probability by less than
  2^-32, far below what 2^20 chains can resolve;
* sweep t visits the spins in that sweep's order, each with beta_t.  At the end of the sweep
  only, best <- current if E(current) < E(best) (strict).  The start is the first candidate;
* the start is uniform without x0 (§4.3), a point mass at x0 with one.

``WRONG_LAWS`` are rules that each change one thing; the tests assert that the chains' counts
reject every one of them, so that the reference can tell these laws apart.
"""
import numpy as np
import scipy.stats

import oracle

# one changed rule each (see propagate)
WRONG_LAWS = {
    "a": "sweep t uses beta_{t+1}",
    "b": "beta doubled",
    "c": "best snapshotted after every accepted flip",
    "d": "start not a best candidate",
    "e": "synchronous sweep (every proposal sees the sweep's starting configuration)",
    "f": "heat-bath acceptance 1/(1+exp(beta dE))",
    "g": "colour order in every sweep (shuffled runs only)",
}

PASS_P = 1e-6      # the true law passes at p >= PASS_P
REJECT_P = 1e-12   # every wrong law is rejected at p <= REJECT_P


def energies(J, h):
    """E(c) for every configuration c of len(h) spins (dense J, float64)."""
    J = np.asarray(J, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    c = np.arange(1 << n)
    s = 2.0 * ((c[:, None] >> np.arange(n)) & 1) - 1.0
    return np.einsum("ci,ij,cj->c", s, J, s) + s @ h


def colour_order(J_full, members):
    """Local spin indices of ``members`` (global ids) in the colour order of oracle.sa_layout."""
    _, order, _, _, _ = oracle.sa_layout(J_full)
    where = {int(g): i for i, g in enumerate(members)}
    return np.array([where[int(g)] for g in order if int(g) in where], dtype=np.int64)


def shuffled_orders(seed, num_sweeps, members):
    """Per sweep t the local spin indices in ascending (pi_t(g), g), pi_t(g) = word 0 of
    Philox4x32-10(counter (g, t, 0xFFFFFFFE, 0), key (seed lo, seed hi)) for global id g."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = []
    for t in range(num_sweeps):
        keys = [(int(oracle.philox4x32_10((int(g), t, 0xFFFFFFFE, 0), key)[0]), int(g), i)
                for i, g in enumerate(members)]
        out.append(np.array([i for _, _, i in sorted(keys)], dtype=np.int64))
    return out


def _acceptance(de, beta, rule):
    de = np.asarray(de, dtype=np.float64)
    if rule == "f":
        with np.errstate(over="ignore", invalid="ignore"):
            x = beta * de
            p = 1.0 / (1.0 + np.exp(np.where(de == 0, 0.0, x)))
        return p
    with np.errstate(invalid="ignore"):
        x = np.where(de > 0, beta * de, 0.0)
    p = np.where(x >= 23.0, 0.0, np.exp(-np.minimum(x, 23.0)))
    return np.where(de <= 0, 1.0, p)


class Law:
    """best[c]: law of the returned configuration; current[t][c]: law of the current
    configuration after t sweeps; accepted: expected accepted flips per chain."""

    def __init__(self, best, current, accepted):
        self.best, self.current, self.accepted = best, current, accepted


def propagate(E, betas, orders, x0=None, rule=None):
    """The exact law of one chain.  E: energies(J, h); betas[T]; orders: T arrays of local spin
    indices (one per sweep); x0: a local configuration int or None (uniform); rule: None or a
    key of WRONG_LAWS ("g" is the caller's: it passes the colour order)."""
    size = E.shape[0]
    n = size.bit_length() - 1
    betas = [float(b) for b in betas]
    T = len(betas)
    if rule == "a":
        betas = betas[1:] + betas[-1:]
    elif rule == "b":
        betas = [2.0 * b for b in betas]
    P = np.zeros((size, size))
    idx = np.arange(size)
    if x0 is None:
        P[idx, idx] = 1.0 / size
    else:
        P[x0, x0] = 1.0
    better = E[:, None] < E[None, :]        # better[c, b]: E(c) < E(b)
    current = {0: P.sum(axis=1)}
    accepted = 0.0

    def snapshot(P, all_to_current=False):
        move = np.ones_like(better) if all_to_current else better
        gain = np.where(move, P, 0.0).sum(axis=1)
        P = np.where(move, 0.0, P)
        P[idx, idx] += gain
        return P

    for t in range(T):
        beta = betas[t]
        if rule == "e":
            # every spin proposes against the sweep's starting configuration c0
            K = np.ones((size, size))           # K[c0, c1]
            diff = idx[:, None] ^ idx[None, :]
            for i in range(n):
                a = _acceptance(E[idx ^ (1 << i)] - E, beta, rule)
                accepted += float(a @ P.sum(axis=1))
                K *= np.where((diff >> i) & 1, a[:, None], 1.0 - a[:, None])
            P = K.T @ P
        else:
            for i in orders[t]:
                a = _acceptance(E[idx ^ (1 << int(i))] - E, beta, rule)
                accepted += float(a @ P.sum(axis=1))
                flipped = a[:, None] * P
                P = P - flipped + flipped[idx ^ (1 << int(i))]
                if rule == "c":
                    P = snapshot(P)
        P = snapshot(P, all_to_current=(rule == "d" and t == 0))
        current[t + 1] = P.sum(axis=1)
    return Law(P.sum(axis=0), current, accepted)


def local_configs(xs, members):
    """(R,) local configuration ints of the spins ``members`` (global ids) of packed words xs."""
    xs = np.asarray(xs, dtype=np.uint64)
    out = np.zeros(xs.shape[0], dtype=np.int64)
    for i, g in enumerate(members):
        bit = (xs[:, int(g) // 64] >> np.uint64(int(g) % 64)) & np.uint64(1)
        out |= bit.astype(np.int64) << i
    return out


def chi2_pvalue(observed, probs):
    """Pearson chi-square of counts ``observed`` against the law ``probs`` (same cells): cells
    with expected count >= 5 on their own, the rest pooled into one cell.  Returns the p-value
    (scipy.stats.chi2.sf); 0.0 if a count falls where the law puts no mass."""
    observed = np.asarray(observed, dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64)
    total = observed.sum()
    expected = probs * total
    big = expected >= 5
    obs = list(observed[big])
    exp = list(expected[big])
    rest_obs, rest_exp = observed[~big].sum(), expected[~big].sum()
    if rest_exp > 0:
        obs.append(rest_obs)
        exp.append(rest_exp)
    elif rest_obs > 0:
        return 0.0
    obs, exp = np.array(obs), np.array(exp)
    if obs.shape[0] < 2:
        return 1.0
    stat = float(((obs - exp) ** 2 / exp).sum())
    return float(scipy.stats.chi2.sf(stat, obs.shape[0] - 1))


def energy_law(E, law_c, values):
    """Law over the sorted distinct ``values`` of E(c) under the configuration law ``law_c``."""
    pos = np.searchsorted(values, E)
    return np.bincount(pos, weights=law_c, minlength=values.shape[0])


# ----------------------------------------------------------------------------
# the two systems and the ladder the law tests share
# ----------------------------------------------------------------------------

def system_p1():
    """n = 7, frustrated (odd rings), non-symmetric J with a diagonal, a field; >= 3 colours.
    Every value is a multiple of 1/8 with |.| <= 2."""
    n = 7
    J = np.zeros((n, n))
    edges = {(0, 1): (1.0, -0.25), (1, 2): (0.5, 0.75), (2, 0): (0.875, 0.0),
             (2, 3): (-1.0, 0.25), (3, 4): (0.625, 0.5), (4, 2): (0.25, 0.5),
             (4, 5): (-0.75, -0.5), (5, 6): (1.25, 0.0), (6, 0): (0.375, 0.5),
             (1, 5): (0.5, -1.5), (3, 6): (-0.125, 0.875)}
    for (i, j), (a, b) in edges.items():
        J[i, j], J[j, i] = a, b
    J[0, 0], J[3, 3], J[5, 5] = 0.5, -1.25, 2.0
    h = np.array([0.25, -0.5, 0.0, 1.0, -0.125, 0.375, -0.75])
    return J, h


def system_p2():
    """n = 8: spin 7 isolated with no field (every proposal has dE = 0), spin 6 coupled to 0 and
    1 with equal weight and no field (dE = 0 whenever s_0 = -s_1), the rest a frustrated
    non-symmetric block with a diagonal and a field."""
    n = 8
    J = np.zeros((n, n))
    edges = {(0, 1): (0.75, 0.25), (1, 2): (-0.5, 1.0), (2, 3): (0.625, 0.125),
             (3, 0): (0.5, 0.5), (0, 2): (-0.25, -0.5), (3, 4): (1.5, -0.25),
             (4, 5): (-0.375, -0.375), (5, 1): (0.875, 0.25), (6, 0): (0.25, 0.25),
             (6, 1): (0.5, 0.0)}
    for (i, j), (a, b) in edges.items():
        J[i, j], J[j, i] = a, b
    J[2, 2], J[4, 4] = -0.5, 1.0
    h = np.array([-0.25, 0.5, 0.125, 0.0, -0.625, 0.25, 0.0, 0.0])
    return J, h


# low-lying starting configurations (E = -6.125 and -5.625, not the ground states) from which every
# wrong law, "d" included, moves the returned law far beyond the noise of 2^18 chains
X0 = {"P1": 76, "P2": 10}

# hot and cold alternate; one sweep at beta = 0 (every proposal accepted), one at +inf
LADDER = np.array([0.35, 3.0, 0.0, 1.75, 0.25, np.inf, 0.5, 1.25, 0.2, 2.5, 0.6, 1.0,
                   0.3, 4.0, 0.45, 1.5])


def laws_for(E, betas, orders, colour, x0=None, shuffled=False):
    """{None: the true law, key: the law with WRONG_LAWS[key]} for a run in ``orders`` (T
    arrays); ``colour``: the colour order (one array), which is what "g" runs."""
    laws = {None: propagate(E, betas, orders, x0)}
    # "d" only from a low-lying x0: a uniform start is beaten by the end of the beta = +inf sweep
    # in nearly every chain, so with or without it as a candidate the returned law moves by less
    # than 2^18 chains resolve (noncentrality < 20 on both systems for every ladder tried)
    for rule in ("abcdef" if x0 is not None else "abcef"):
        laws[rule] = propagate(E, betas, orders, x0, rule)
    if shuffled:
        laws["g"] = propagate(E, betas, [colour] * len(betas), x0)
    return laws


def pvalue(E, law, best_configs, current_energies=None):
    """The smallest p-value among: the returned configurations against law.best, and for each
    t of ``current_energies`` ({t: E(current) after t sweeps per chain}) the energies against the
    law of E(current) after t sweeps."""
    ps = [chi2_pvalue(np.bincount(best_configs, minlength=E.shape[0]), law.best)]
    values = np.unique(E)
    for t, e in (current_energies or {}).items():
        pos = np.clip(np.searchsorted(values, e), 0, values.shape[0] - 1)
        assert np.array_equal(values[pos], e), "a current energy is not an energy of the system"
        ps.append(chi2_pvalue(np.bincount(pos, minlength=values.shape[0]),
                              energy_law(E, law.current[t], values)))
    return min(ps)


def assert_law(label, E, laws, best_configs, accepted=None, current_energies=None, report=print):
    """The true law passes (p >= PASS_P), every wrong law in ``laws`` is rejected
    (p <= REJECT_P), and the mean accepted flips per chain lie within 5 standard errors of the
    exact expectation."""
    ps = {rule: pvalue(E, law, best_configs, current_energies) for rule, law in laws.items()}
    line = "%s: true law p = %.3g; wrong laws: %s" % (
        label, ps[None], ", ".join("%s p = %.3g" % (k, ps[k]) for k in sorted(k for k in ps if k is not None)))
    if accepted is not None:
        accepted = np.asarray(accepted, dtype=np.float64)
        mean, se = accepted.mean(), accepted.std(ddof=1) / np.sqrt(accepted.shape[0])
        line += "; accepted flips %.5f (exact %.5f, %.1f s.e.)" % (
            mean, laws[None].accepted, (mean - laws[None].accepted) / se)
    report(line)
    assert ps[None] >= PASS_P, line
    for rule in ps:
        if rule is not None:
            assert ps[rule] <= REJECT_P, "wrong law %s (%s) not rejected: %s" % (
                rule, WRONG_LAWS[rule], line)
    if accepted is not None:
        assert abs(mean - laws[None].accepted) <= 5 * se, line


# ----------------------------------------------------------------------------
# P1 inside a production-sized frozen filler
# ----------------------------------------------------------------------------

EMBED_SIZE = 20000
EMBED_AT = np.array([5, 63, 64, 127, 4093, 11111, 19999])   # P1's spin i sits at EMBED_AT[i]
FILLER_FIELD = 512.0
# LADDER without its beta = 0 sweep: the smallest beta keeps every filler flip at beta dE >= 23
EMBED_LADDER = np.where(LADDER == 0.0, 0.05, LADDER)


def embedded_system(seed=20000):
    """(J csr, h, x0 words, filler_energy): P1 at the global ids EMBED_AT of an EMBED_SIZE-spin
    system whose other spins (the filler) have the couplings of synthetic.random_symmetric_graph
    (mean degree 20, values +-1/8), fields +-2^9, no coupling to P1, and x0 aligned with their
    fields.  Every filler flip away from x0 costs dE >= 1000 and EMBED_LADDER's smallest beta
    makes beta dE >= 23 for all of them: the filler never moves, P1's chains follow P1's exact law
    (the random word depends on (spin, sweep, replica) only), and every energy is exact.
    x0's P1 bits are X0["P1"]; filler_energy is E of the filler part of x0 alone."""
    from annealing_sign_problem_amd import synthetic

    rng = np.random.default_rng(seed)
    K = EMBED_SIZE
    lo, hi = synthetic.random_symmetric_graph(K, 20.0, 40, rng)
    p1 = np.zeros(K, dtype=bool)
    p1[EMBED_AT] = True
    keep = ~(p1[lo] | p1[hi])
    lo, hi = lo[keep], hi[keep]
    val = rng.choice([-0.125, 0.125], size=lo.shape[0])
    rows = np.concatenate([lo, hi])
    cols = np.concatenate([hi, lo])
    vals = np.concatenate([val, val])
    h = rng.choice([-FILLER_FIELD, FILLER_FIELD], size=K)
    Jp, hp = system_p1()
    pi, pj = np.nonzero(Jp)
    rows = np.concatenate([rows, EMBED_AT[pi]])
    cols = np.concatenate([cols, EMBED_AT[pj]])
    vals = np.concatenate([vals, Jp[pi, pj]])
    h[EMBED_AT] = hp
    import scipy.sparse

    J = scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(K, K))
    J.sum_duplicates()
    J.sort_indices()
    bits = h < 0                       # s = +1 where the field is negative: aligned
    bits[EMBED_AT] = [(X0["P1"] >> i) & 1 for i in range(EMBED_AT.shape[0])]
    x0 = np.zeros((K + 63) // 64, dtype=np.uint64)
    for g in np.nonzero(bits)[0]:
        x0[g // 64] |= np.uint64(1) << np.uint64(g % 64)
    s = np.where(bits, 1.0, -1.0)
    s[EMBED_AT] = 0.0                  # no coupling crosses: P1's part drops out
    filler_energy = float(s @ (J @ s) + h @ s)
    # the filler is frozen: its smallest flip cost at x0 times the smallest beta
    A = (J + J.T).tocsr()
    A.setdiag(0)
    g = A @ np.where(bits, 1.0, -1.0) + h
    de = np.where(bits, -2.0, 2.0) * g
    assert np.min(de[~p1]) * EMBED_LADDER.min() >= 23.0
    return J, h, x0, filler_energy
