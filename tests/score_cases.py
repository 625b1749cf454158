"""Named cases and the numpy law of the sign scores (specification ASP-SCORE-1, DESIGN.md §3.11;
csrc/sign_scores.hip): shared by test_score_cases.py (no GPU: the law against the host function) and
test_gpu_sign_scores.py (the kernels against the law, bit for bit).

The sizes the cases are placed around are the kernels' constants."""
import functools

import numpy as np

PASS = 256   # positions one pass of a scoring workgroup takes (kPass)
TILE = 64    # configurations per side of a distance tile (kTile)
CHUNK = 16   # words of a configuration staged in LDS at a time (kChunk)

SCORED = (1, 2, 63, 64, 65, 127, 128, 129, PASS - 1, PASS, PASS + 1, 2 * PASS + 1, 7 * PASS + 1)
COUNTS = (1, 2, 63, 64, 65, 257)
WEIGHTS = ("none", "lognormal", "zeros_subnormals", "all_zero")
SELECTS = ("none", "reversed", "subset", "repeats")
DISTANCE_COUNTS = (1, 2, 63, 64, 65, 130)
DISTANCE_WORDS = (1, 2, 3, CHUNK + 1)


def words_of(spins: int) -> int:
    return (spins + 63) // 64


def pack(bits) -> np.ndarray:
    """0/1 values [..., n] -> uint64 words [..., ceil(n / 64)], bit i of word i // 64."""
    bits = np.asarray(bits, dtype=np.uint8)
    n = bits.shape[-1]
    padded = np.zeros(bits.shape[:-1] + (words_of(n) * 64,), dtype=np.uint8)
    padded[..., :n] = bits
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(bits.shape[:-1] + (words_of(n),))


def unpack(words, n: int) -> np.ndarray:
    """uint64 words [..., W] -> 0/1 values [..., n]."""
    words = np.ascontiguousarray(words, dtype="<u8")
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n]


def tree_sum(terms) -> np.float64:
    """THE LAW's sum: terms padded with +0.0 to the next power of two, then neighbours added, level by
    level (strides 1, 2, 4, ... ascending), every add rounded on its own."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    size = 1
    while size < max(terms.shape[0], 1):
        size *= 2
    p = np.zeros(size, dtype=np.float64)
    p[:terms.shape[0]] = terms
    while p.shape[0] > 1:
        p = p.reshape(-1, 2)
        p = p[:, 0] + p[:, 1]
    return np.float64(p[0])


def gathered(case, xs=None) -> np.ndarray:
    """0/1 values [C, K0]: bit select[i] of every configuration (bits at and beyond K never read)."""
    xs = case["xs"] if xs is None else xs
    bits = unpack(np.ascontiguousarray(xs[:, :max(words_of(case["spins"]), 0)]), case["spins"])
    if case["select"] is None:
        return bits
    return bits[:, case["select"]]


def scores_law(case, xs=None):
    """``(matches uint64[C], signed float64[C], total float64)`` of a case by the specification."""
    g = gathered(case, xs)
    scored = case["scored"]
    e = unpack(case["exact"], scored)
    w = np.ones(scored, dtype=np.float64) if case["weights"] is None else case["weights"]
    same = g == e[None, :]
    matches = same.sum(axis=1).astype(np.uint64)
    signed = np.array([tree_sum(np.where(row, w, -w)) for row in same], dtype=np.float64).reshape(-1)
    return matches, signed, tree_sum(w)


def distances_law(xs, spins: int) -> np.ndarray:
    """uint32[C, C] Hamming distances over the first ``spins`` bits, through np.unpackbits."""
    bits = unpack(np.ascontiguousarray(xs[:, :words_of(spins)]), spins).astype(np.int64)
    agree = bits @ bits.T + (1 - bits) @ (1 - bits).T
    return (spins - agree).astype(np.uint32)


def bits_of(value: np.ndarray) -> np.ndarray:
    """Bit patterns for an exact comparison; ``+ 0.0`` first: a zero may carry either sign."""
    return (np.asarray(value, dtype=np.float64) + 0.0).view(np.uint64)


def _weights(kind: str, scored: int, rng):
    if kind == "none":
        return None
    if kind == "all_zero":
        return np.zeros(scored, dtype=np.float64)
    w = np.exp(rng.normal(0.0, 3.0, size=scored)) ** 2
    if kind == "zeros_subnormals":
        where = rng.permutation(scored)
        w[where[::3]] = 0.0
        w[where[1::3]] = 5e-324 * rng.integers(1, 1000, size=where[1::3].shape[0])
    return w


def _select(kind: str, scored: int, rng):
    """``(spins K, select)`` for K0 = scored."""
    if kind == "none":
        return scored, None
    if kind == "reversed":
        return scored, np.arange(scored, dtype=np.int32)[::-1].copy()
    if kind == "subset":  # the frozen-cluster case: K0 of K spins, in order
        spins = scored + scored // 2 + 70
        return spins, np.sort(rng.choice(spins, size=scored, replace=False)).astype(np.int32)
    spins = max(scored // 3, 1)  # repeats: K0 > K (K0 = K = 1 at the smallest)
    return spins, rng.integers(0, spins, size=scored).astype(np.int32)


def _case(name, scored, count, weights, select, rng, extra_stride=0):
    spins, sel = _select(select, scored, rng)
    words = words_of(spins)
    exact_bits = rng.integers(0, 2, size=scored, dtype=np.uint8)
    exact = pack(exact_bits)
    # content: configuration 0 reproduces `exact` at the scored positions where that is possible (no
    # select, or a permutation / subset), 1 is its complement, the others are random
    bits = rng.integers(0, 2, size=(count, spins), dtype=np.uint8)
    if select != "repeats":
        first = rng.integers(0, 2, size=spins, dtype=np.uint8)
        first[np.arange(scored) if sel is None else sel] = exact_bits
        bits[0] = first
        if count > 1:
            bits[1] = 1 - first
    xs = np.zeros((count, words + extra_stride), dtype=np.uint64)
    xs[:, :words] = pack(bits)
    # garbage where nothing may be read: the bits beyond K of the last word, and the words beyond W
    if spins % 64:
        xs[:, words - 1] |= rng.integers(0, 2**63, size=count, dtype=np.uint64) << np.uint64(spins % 64)
    if extra_stride:
        xs[:, words:] = rng.integers(0, 2**63, size=(count, extra_stride), dtype=np.uint64)
    exact_garbage = exact.copy()
    if scored % 64:
        exact_garbage[-1] |= np.uint64(rng.integers(0, 2**63)) << np.uint64(scored % 64)
    return {"name": name, "spins": spins, "scored": scored, "xs": xs, "exact": exact_garbage,
            "weights": _weights(weights, scored, rng), "select": sel}


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> case: ``spins`` K, ``scored`` K0, ``xs`` uint64[C, stride], ``exact`` uint64[ceil(K0/64)]
    (garbage beyond K0), ``weights`` float64[K0] or None, ``select`` int32[K0] or None.  Do not modify."""
    rng = np.random.default_rng(20240611)
    out = {}

    def add(name, *args, **kwargs):
        out[name] = _case(name, *args, rng=rng, **kwargs)

    for scored in SCORED:  # every size with weights and without, three configurations
        add("k%d_lognormal" % scored, scored, 3, "lognormal", "none")
        add("k%d_none" % scored, scored, 3, "none", "none")
    for count in COUNTS:  # every number of configurations, across a pass boundary
        add("c%d_lognormal" % count, PASS + 1, count, "lognormal", "none")
    add("c257_select", 65, 257, "none", "subset")
    for kind in WEIGHTS:  # every kind of weights with every kind of select, two passes + 1
        for select in SELECTS:
            add("w_%s_s_%s" % (kind, select), 2 * PASS + 1, 4, kind, select)
    for scored in (1, 63, 65, PASS, 7 * PASS + 1):  # the selects at the small and the largest sizes
        for select in SELECTS[1:]:
            add("k%d_s_%s" % (scored, select), scored, 2, "lognormal", select)
    for scored in (64, PASS + 1):  # a stride above the words of a configuration
        add("k%d_stride" % scored, scored, 5, "zeros_subnormals", "none", extra_stride=3)
        add("k%d_stride_select" % scored, scored, 5, "lognormal", "subset", extra_stride=2)
    return out


@functools.lru_cache(maxsize=None)
def laws() -> dict:
    """name -> :func:`scores_law` of the case, computed once."""
    return {name: scores_law(case) for name, case in cases().items()}


@functools.lru_cache(maxsize=None)
def distance_cases() -> dict:
    """name -> ``(xs uint64[C, stride], spins)``; garbage beyond K and beyond W.  Do not modify."""
    rng = np.random.default_rng(977)
    out = {}

    def add(name, count, words, spins, extra_stride=0):
        assert words_of(spins) == words
        bits = rng.integers(0, 2, size=(count, spins), dtype=np.uint8)
        if count > 2:
            bits[2] = bits[0]  # two equal configurations: a zero off the diagonal
        if count > 1:
            bits[1] = 1 - bits[0]  # and a complement: the distance K
        xs = np.zeros((count, words + extra_stride), dtype=np.uint64)
        xs[:, :words] = pack(bits)
        if spins % 64:
            xs[:, words - 1] |= rng.integers(0, 2**63, size=count, dtype=np.uint64) << np.uint64(spins % 64)
        if extra_stride:
            xs[:, words:] = rng.integers(0, 2**63, size=(count, extra_stride), dtype=np.uint64)
        out[name] = (xs, spins)

    for count in DISTANCE_COUNTS:
        for words in DISTANCE_WORDS:
            add("c%d_w%d_tail" % (count, words), count, words, 64 * words - 27)
    add("c65_w2_whole_words", 65, 2, 128)
    add("c130_w17_whole_words", 130, CHUNK + 1, 64 * (CHUNK + 1))
    add("c3_w1_one_spin", 3, 1, 1)
    add("c65_w3_stride", 65, 3, 150, extra_stride=2)
    return out
