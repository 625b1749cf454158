"""The word layout's best configuration kept as difference bits (csrc/sa_device.hpp): the
cases the GPU test runs (tests/test_gpu_sa_lazy_best.py) and a numpy restatement of the word algebra that
the CPU test checks on the same cases (tests/test_lazy_best_cases.py).

Byte m of a position's 32-bit word is 0x80 * s_m + d_m: s_m replica m's sign bit, d_m "differs from
replica m's best configuration".  A flip toggles both, an improvement of replica m clears d_m at every
position, and the best configuration is s_m ^ d_m."""
import numpy as np
import scipy.sparse

M = 4  # replicas of a word
SIZES = {70: dict(mean_degree=6.0, seed=70), 600: dict(mean_degree=6.0, seed=600), 3000: dict(mean_degree=8.0, seed=3000)}
SWEEPS = (1, 2, 24)
SCHEDULES = ("monotone", "reheat", "hot", "frozen")


def model(spins):
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(spins, **SIZES[spins])
    J = scipy.sparse.csr_matrix(J)
    # a weak random field: no proposal has dE = 0 exactly (an isolated spin without a field flips in every
    # sweep at any beta), and s and -s differ in energy
    h = np.random.default_rng(spins).normal(size=spins) * 0.1 * np.abs(J.data).mean()
    return J, np.ascontiguousarray(h, np.float64)


def schedule(name, beta0, beta1, sweeps):
    """monotone: the geometric ladder.  reheat: freeze, reheat, freeze again — the best is mid-run and is
    followed by flips.  hot: beta = 0, every proposal is accepted: the best is the start or one of the two states the chain
    alternates between (about half of the chains never improve and report their start).  frozen: beta =
    1e15 (from the greedy minimum as x0: nothing flips)."""
    from annealing_sign_problem_amd import annealer as sa

    if name == "monotone":
        return sa.make_schedule(beta0, beta1, sweeps)
    if name == "reheat":
        third = max(1, sweeps // 3)
        down = sa.make_schedule(beta0, beta1, third)
        rest = sweeps - 2 * third
        return np.concatenate([down, down[::-1][:third], sa.make_schedule(beta0, beta1, rest) if rest else down[:0]])[:sweeps]
    if name == "hot":
        return np.zeros(sweeps)
    assert name == "frozen"
    return np.full(sweeps, 1e15)


# ---------------------------------------------------------------------------------------------
# The word algebra
# ---------------------------------------------------------------------------------------------

def differs_mask(mask):
    return ((np.asarray(mask, np.uint32) & np.uint32(0xF)) * np.uint32(0x00204081)) & np.uint32(0x01010101)


def start_words(signs):
    """signs[M, P] (1 = s = -1) -> words with d = 0."""
    w = np.zeros(signs.shape[1], np.uint32)
    for m in range(signs.shape[0]):
        w |= signs[m].astype(np.uint32) << np.uint32(8 * m + 7)
    return w


def flip(words, masks, variant="both"):
    """masks[P]: bit m = replica m flips at the position.  variant "sign_only" is the WRONG flip that
    toggles bit 8m + 7 alone."""
    t = differs_mask(masks)
    return words ^ ((t << np.uint32(7)) | (t if variant == "both" else np.uint32(0)))


def clear(words, improved, variant="improved"):
    """The replicas in `improved` are at their best.  variant "all" is the WRONG clear of every replica."""
    if improved == 0:
        return words
    return words & ~differs_mask((1 << M) - 1 if variant == "all" else improved)


def current(words, m):
    return ((words >> np.uint32(8 * m + 7)) & np.uint32(1)).astype(np.uint8)


def best(words, m):
    return (((words ^ (words << np.uint32(7))) >> np.uint32(8 * m + 7)) & np.uint32(1)).astype(np.uint8)


def sign_byte(words, m):
    """The top byte of the k-loop's multiplier: byte m OR 0x3F."""
    return ((words >> np.uint32(8 * m)) & np.uint32(0xFF)) | np.uint32(0x3F)


def replay(start, events, flip_variant="both", clear_variant="improved"):
    """events: per sweep (masks[P], improved).  Returns (words, best[M, P] of the plain "copy on
    improvement" model, current[M, P] of it)."""
    cur = start.copy()
    kept = start.copy()
    words = start_words(start)
    for masks, improved in events:
        words = flip(words, masks, flip_variant)
        for m in range(start.shape[0]):
            cur[m] ^= ((masks >> m) & 1).astype(np.uint8)
            if (improved >> m) & 1:
                kept[m] = cur[m]
        words = clear(words, improved, clear_variant)
    return words, kept, cur


# ---------------------------------------------------------------------------------------------
# Flip / improve sequences of the cases: a numpy Metropolis anneal of four chains (numpy random numbers,
# not the device's chains; one sequence per case)
# ---------------------------------------------------------------------------------------------

def _colours(A):
    colour = np.full(A.shape[0], -1)
    for i in range(A.shape[0]):
        used = set(colour[A.indices[A.indptr[i]:A.indptr[i + 1]]])
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return [np.nonzero(colour == c)[0] for c in range(colour.max() + 1)]


def events_of(spins, name, sweeps, seed=1):
    """(start[M, P], events) of the case: per sweep the flip masks and the replicas whose energy fell below
    their best so far."""
    J, h = model(spins)
    A = scipy.sparse.csr_matrix(J + J.T)
    A.setdiag(0)
    A.eliminate_zeros()
    classes = _colours(A)
    scale = np.abs(A).sum(axis=1).max() or 1.0
    betas = schedule(name, 0.1 / scale, 20.0 / np.abs(A.data).min(), sweeps)
    rng = np.random.default_rng(seed)
    s = np.where(rng.random((spins, M)) < 0.5, -1.0, 1.0)
    if name == "frozen":  # one shared local minimum
        s[:] = s[:, :1]
        for _ in range(200):
            moved = False
            for members in classes:
                de = -2.0 * s[members] * (A[members] @ s + h[members][:, None])
                s[members] = np.where(de < 0.0, -s[members], s[members])
                moved = moved or bool((de < 0.0).any())
            if not moved:
                break
    start = (s.T < 0).astype(np.uint8)
    energy = np.zeros(M)
    lowest = np.zeros(M)
    events = []
    for beta in betas:
        masks = np.zeros(spins, np.uint32)
        for members in classes:
            de = -2.0 * s[members] * (A[members] @ s + h[members][:, None])
            accept = (de <= 0.0) | (rng.random(de.shape) < np.exp(-np.clip(beta * de, 0.0, 700.0)))
            s[members] = np.where(accept, -s[members], s[members])
            energy += (de * accept).sum(axis=0)
            masks[members] = (accept << np.arange(M)).sum(axis=1).astype(np.uint32)
        improved = 0
        for m in range(M):
            if energy[m] < lowest[m]:
                lowest[m] = energy[m]
                improved |= 1 << m
        events.append((masks, improved))
    return start, events


def cases():
    """(spins, schedule, sweeps) of every case, CPU and GPU."""
    return [(k, name, n) for k in sorted(SIZES) for name in SCHEDULES for n in SWEEPS]
