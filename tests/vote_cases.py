"""Named cases and the numpy restatement of the consensus vote (law ASP-VOTE-1, DESIGN.md §3.12;
csrc/sign_vote.hip): shared by test_vote_cases.py (no GPU: the restatement against a scalar loop, the
planted truth and the order of the sums), test_gpu_sign_vote.py (the kernels against the restatement, bit
for bit) and the chain and driver tests.

The sizes the cases are placed around are the kernels' constants."""
import functools

import numpy as np

from score_cases import pack, unpack, words_of

WAVES = 4            # configurations of an alignment workgroup and word columns of a site workgroup (kWaves)
BLOCK = 64 * WAVES   # sites of a site workgroup
STRIDE = 64          # words a wavefront of the alignment pass takes at a time: 64 * STRIDE spins

SPINS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097, 70001)
COUNTS = (1, 2, 3, 63, 64, 65, 129, 1025)
WEIGHTS = ("none", "lognormal", "span")


def vote_law(spins, xs, weights=None, ref=None, anchor=0, align=True, rounds=1) -> dict:
    """THE LAW, restated: ``distance uint32[R]``, ``flipped bool[R]``, ``ones uint32[K]``, ``plus`` /
    ``minus float64[K]``, ``x uint64[W]`` and ``changed`` of the last of ``rounds`` rounds.  A plain loop
    over the configurations in ascending order; every add is one rounded float64 add."""
    xs = np.asarray(xs, dtype=np.uint64)
    count, words = xs.shape[0], words_of(spins)
    bits = unpack(np.ascontiguousarray(xs[:, :words]), spins)  # (bits at and beyond K never read)
    w = np.ones(count, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    ref_bits = bits[anchor].copy() if ref is None else unpack(np.asarray(ref, dtype=np.uint64)[:words], spins)
    for _ in range(rounds):
        distance = (bits != ref_bits[None, :]).sum(axis=1).astype(np.uint32)
        flipped = np.logical_and(bool(align), 2 * distance.astype(np.int64) > spins)
        aligned = bits ^ flipped[:, None].astype(np.uint8)
        ones = aligned.sum(axis=0, dtype=np.uint32)
        plus, minus = np.zeros(spins, dtype=np.float64), np.zeros(spins, dtype=np.float64)
        for r in range(count):
            up = aligned[r] == 1
            plus[up] += w[r]
            minus[~up] += w[r]
        c = np.where(plus > minus, 1, np.where(plus < minus, 0, ref_bits)).astype(np.uint8)
        changed = int((c != ref_bits).sum())
        ref_bits = c
    return {"distance": distance, "flipped": flipped, "ones": ones, "plus": plus, "minus": minus, "x": pack(c),
            "changed": changed}


def law_of(case) -> dict:
    return vote_law(case["spins"], case["xs"], case["weights"], case["ref"], case["anchor"], case["align"],
                    case["rounds"])


def arguments(case) -> tuple:
    """The case as ``scores.consensus`` takes it."""
    return (case["xs"], case["spins"], case["weights"], case["ref"], case["anchor"], case["align"], case["rounds"])


def bits_of(value) -> np.ndarray:
    """Bit patterns for an exact comparison (the law's sums start at +0.0 and add nothing negative except
    -0.0, so no zero is negative)."""
    return np.asarray(value, dtype=np.float64).view(np.uint64)


def same(got, law) -> bool:
    """``got`` (a ``scores.Consensus`` or a dict of the law's arrays) is the law, every bit."""
    if not isinstance(got, dict):
        got = {name: getattr(got, name) for name in law}
    return (np.array_equal(np.asarray(got["distance"], dtype=np.uint32), law["distance"])
            and np.array_equal(np.asarray(got["flipped"], dtype=bool), law["flipped"])
            and np.array_equal(np.asarray(got["ones"], dtype=np.uint32), law["ones"])
            and np.array_equal(bits_of(got["plus"]), bits_of(law["plus"]))
            and np.array_equal(bits_of(got["minus"]), bits_of(law["minus"]))
            and np.array_equal(np.asarray(got["x"], dtype=np.uint64), law["x"])
            and int(got["changed"]) == law["changed"])


def make_weights(kind: str, count: int, rng):
    if kind == "none":
        return None
    if kind == "lognormal":
        return np.exp(rng.normal(0.0, 3.0, size=count)) ** 2
    if kind == "span":  # 2^-40 .. 2^53, random mantissas: sums that round at every step
        return np.ldexp(rng.uniform(0.5, 1.0, size=count), rng.integers(-39, 54, size=count).astype(np.int32))
    raise ValueError(kind)


def stored(bits, spins: int, rng, extra_stride: int = 0) -> np.ndarray:
    """0/1 values [R, K] as uint64[R, W + extra_stride] with garbage where nothing may be read: the bits
    beyond K of the last word and the words beyond W."""
    count, words = bits.shape[0], words_of(spins)
    xs = np.zeros((count, words + extra_stride), dtype=np.uint64)
    xs[:, :words] = pack(bits)
    if spins % 64:
        xs[:, words - 1] |= rng.integers(0, 2**63, size=count, dtype=np.uint64) << np.uint64(spins % 64)
    if extra_stride:
        xs[:, words:] = rng.integers(0, 2**63, size=(count, extra_stride), dtype=np.uint64)
    return xs


def planted_bits(spins: int, count: int, rng, defects: float = 0.1):
    """``(truth uint8[K], bits uint8[R, K])``: every configuration is the truth with independent defects
    on a tenth of the sites, then flipped as a whole with probability 1/2."""
    truth = rng.integers(0, 2, size=spins, dtype=np.uint8)
    wrong = (rng.random(size=(count, spins)) < defects).astype(np.uint8)
    flips = rng.integers(0, 2, size=(count, 1), dtype=np.uint8)
    return truth, truth[None, :] ^ wrong ^ flips


def _case(name, spins, xs, weights=None, ref=None, anchor=0, align=True, rounds=1, truth=None):
    return {"name": name, "spins": spins, "xs": xs, "weights": weights, "ref": ref, "anchor": anchor, "align": align,
            "rounds": rounds, "truth": truth}


def _garbage_ref(bits, spins: int, rng) -> np.ndarray:
    """A reference as packed words, with garbage in the tail bits of its last word."""
    return stored(np.asarray(bits, dtype=np.uint8)[None, :], spins, rng)[0]


def _with_distances(spins: int, distances, rng) -> np.ndarray:
    """uint8[1 + len(distances), K]: a random configuration, then one at each of the Hamming distances."""
    first = rng.integers(0, 2, size=spins, dtype=np.uint8)
    rows = [first]
    for d in distances:
        row = first.copy()
        row[rng.choice(spins, size=d, replace=False)] ^= 1
        rows.append(row)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> case: ``spins`` K, ``xs`` uint64[R, stride], ``weights`` float64[R] or None, ``ref``
    uint64[W] or None, ``anchor``, ``align``, ``rounds``, and ``truth`` (uint8[K]) where the consensus must
    recover the planted configuration or its complement.  Do not modify."""
    rng = np.random.default_rng(20241021)
    out = {}

    def add(name, *args, **kwargs):
        assert name not in out
        out[name] = _case(name, *args, **kwargs)

    def planted(name, spins, count, kind, recovers=None, extra_stride=0, **kwargs):
        truth, bits = planted_bits(spins, count, rng)
        # (enough sites to align on, enough equal votes to outvote the defects)
        recovers = (kind == "none" and spins >= 63 and count >= 63) if recovers is None else recovers
        add(name, spins, stored(bits, spins, rng, extra_stride), make_weights(kind, count, rng),
            truth=truth if recovers else None, **kwargs)

    # every K with two of the R (every R with one K at least), the weights in turn; R <= 8 at the two largest
    for i, spins in enumerate(SPINS):
        large = spins > 4096
        for j, count in enumerate(((2, 3) if spins == 4097 else (1, 8)) if large
                                  else (COUNTS[i % 8], COUNTS[(3 * i + 5) % 8])):
            kind = WEIGHTS[(i + j) % 3]
            planted("k%d_r%d_%s" % (spins, count, kind), spins, count, kind, anchor=(i + j) % count,
                    extra_stride=(i + j) % 2)
    # each side of every block constant: the configurations of an alignment workgroup, the sites of a site
    # workgroup (K = 255, 256, 257 above), the words of an alignment wavefront's stride
    for count in (WAVES - 1, WAVES, WAVES + 1, 2 * WAVES + 1):
        planted("waves_r%d" % count, 130, count, "lognormal", anchor=count - 1)
    for spins in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1):
        planted("block_k%d" % spins, spins, 65, "none")
    for spins in (64 * STRIDE - 1, 64 * STRIDE, 64 * STRIDE + 1, 128 * STRIDE + 1):
        planted("stride_k%d" % spins, spins, 5, "span", anchor=4)
    # the flip threshold: d = K / 2 stays, K / 2 + 1 flips (even K); (K - 1) / 2 stays, (K + 1) / 2 flips (odd K)
    for spins in (2, 64, 128, 130):
        add("flip_even_k%d" % spins, spins,
            stored(_with_distances(spins, (spins // 2, spins // 2 + 1, spins // 2 - 1), rng), spins, rng))
    for spins in (1, 63, 65, 129):
        add("flip_odd_k%d" % spins, spins,
            stored(_with_distances(spins, ((spins - 1) // 2, (spins + 1) // 2), rng), spins, rng),
            make_weights("lognormal", 3, rng))
    # an even R split exactly in half on the first 40 sites: the tie takes ref, here one with both values
    half = np.zeros((4, 70), dtype=np.uint8)
    half[:2, :40] = 1
    half[:, 40:] = rng.integers(0, 2, size=(4, 30), dtype=np.uint8)
    ref = rng.integers(0, 2, size=70, dtype=np.uint8)
    add("tie_takes_ref", 70, stored(half, 70, rng), ref=_garbage_ref(ref, 70, rng), align=False)
    add("tie_takes_ref_weighted", 70, stored(half, 70, rng), np.array([0.75, 0.25, 0.5, 0.5]),
        ref=_garbage_ref(ref, 70, rng), align=False)
    add("tie_takes_anchor", 70, stored(half, 70, rng), anchor=2, align=False)
    # weights: all zero (c is ref, nothing changes), some zero
    truth, bits = planted_bits(200, 9, rng)
    add("weights_all_zero", 200, stored(bits, 200, rng), np.zeros(9), anchor=3)
    some = make_weights("lognormal", 9, rng)
    some[::2] = 0.0
    add("weights_some_zero", 200, stored(bits, 200, rng), some, anchor=3)
    add("weights_negative_zero", 200, stored(bits, 200, rng), np.array([-0.0, 1.0, -0.0] * 3))
    # align off on flipped chains; an explicit ref, random and planted; rounds 1, 2 and 3 from a random ref
    truth, bits = planted_bits(300, 65, rng)
    xs = stored(bits, 300, rng, extra_stride=2)
    add("align_off", 300, xs, align=False)
    add("align_off_weighted", 300, xs, make_weights("span", 65, rng), align=False, anchor=64)
    add("ref_is_truth", 300, xs, ref=_garbage_ref(truth, 300, rng), truth=truth)
    far = truth.copy()  # half way between the truth and its complement: the first alignment is a coin toss
    far[rng.choice(300, size=150, replace=False)] ^= 1
    for rounds in (1, 2, 3):
        add("rounds%d_random_ref" % rounds, 300, xs, ref=_garbage_ref(far, 300, rng), rounds=rounds)
        add("rounds%d_weighted" % rounds, 300, xs, make_weights("lognormal", 65, rng), anchor=7, rounds=rounds)
    add("rounds16", 300, xs, ref=_garbage_ref(far, 300, rng), rounds=16)
    # a stride above W with garbage in the padding words and in the tail bits
    truth, bits = planted_bits(257, 64, rng)
    add("stride_k257", 257, stored(bits, 257, rng, extra_stride=3), truth=truth)
    add("stride_k257_span", 257, stored(bits, 257, rng, extra_stride=5), make_weights("span", 64, rng), rounds=2)
    # the order of the sums: see order_case()
    order = order_case()
    add("order", order["spins"], order["xs"], order["weights"], order["ref"], 0, False, 1)
    return out


def order_case() -> dict:
    """One site, bits 1, 0, 1, 1 with weights 2^53, 2^53, 1, 1, ref bit 0, align off.  In ascending order
    plus = (2^53 + 1) + 1 = 2^53 (each add rounds to even) ties with minus = 2^53 and the site takes ref's 0;
    a pairwise tree gives plus = (2^53 + 0) + (1 + 1) = 2^53 + 2 and the reversed order (1 + 1) + 2^53, so 1."""
    return {"spins": 1, "xs": pack(np.array([[1], [0], [1], [1]], dtype=np.uint8)),
            "weights": np.array([2.0 ** 53, 2.0 ** 53, 1.0, 1.0]), "ref": np.zeros(1, dtype=np.uint64),
            "bits": np.array([1, 0, 1, 1], dtype=np.uint8)}


@functools.lru_cache(maxsize=None)
def laws() -> dict:
    """name -> :func:`law_of` the case, computed once."""
    return {name: law_of(case) for name, case in cases().items()}
