"""The cases of tests/test_gpu_build_edges.py and tests/test_build_cases.py: inputs for the coupling
build and the sign extraction of csrc/build_matrix.hip (`build_matrix`, `extract_signs`, the
`asp_build_*` handle) at the sizes and values its special paths were written for: the search
instantiation for tables without tails meeting a needle that has one, the hash's zero fingerprint
(key 0), full home buckets and the wrap of a chain past the last bucket, a block's output position
on and next to the 64 / 2048 / 131072 boundaries of the four partial sums, the two rows a wavefront
shares, rows that do not exist, more than 64 super-chunks, and values that show the rounding and the
order of the arithmetic (subnormals, -0.0, counts beyond 2^31 and 2^53, heavy cancellation).

A helper module like tests/prep_cases.py: no fixtures, no files, nothing compiled.  The right
answers are the numpy restatements written here (`build_matrix`, `extract_signs`); next to them
stand named WRONG variants, one keyword switch each.  tests/test_build_cases.py asserts on the CPU
that the restatements equal oracle.build_matrix / oracle.extract_signs bit for bit (the oracle is
pinned to the reference and stays the checker on the GPU) and that every wrong variant is told apart
by a named case, so that the GPU comparison cannot pass a kernel with that mistake.

No NaN and no infinity goes INTO the build, and the magnitudes are kept so that the arithmetic
produces none: a NaN produced by the arithmetic (inf * 0, inf - inf) has no agreed bit pattern
between the CPU oracle and the GPU, so a byte-for-byte comparison of it would test nothing about
the kernel.  `extract_signs` only compares with zero; its cases do contain NaN and both infinities.
"""
import functools
from dataclasses import dataclass, field
from typing import Callable, Tuple

import numpy as np

# The kernel's constants, each with the line of csrc/build_matrix.hip it mirrors.
ROW_LANES = 32                      # kRowLanes :59 — lanes that share a row in k_emit_rows
ROWS_PER_BLOCK = 8                  # kRowsPerBlock :60
GROUP = 64                          # kGroup :61 — needles a wavefront resolves per trip
CHUNK = 2048                        # kChunk :66 — needles of a workgroup of k_search_flat
SUPER = 64 * CHUNK                  # kChunksPerSuper :67 — 131072 needles
BUCKET = 8                          # kBucket :73 — hash slots a probe reads
SLOTS_PER_KEY = 2                   # kSlotsPerKey :63
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def slot_count(k):
    """asp_build_create :473-474: max(64, next power of two >= 2 K)."""
    count = 64
    while count < SLOTS_PER_KEY * k:
        count <<= 1
    return count


def mix64(x):
    """mix64 :82-89, the splitmix64 finaliser.  mix64(0) == 0."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def home_bucket(word0, k):
    """Home bucket of a key in a table of k keys (:105, :140: h & bucket_mask)."""
    return (mix64(word0) & np.uint64(slot_count(k) // BUCKET - 1)).astype(np.int64)


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable[[], object]     # -> BuildInput | np.ndarray (the sign cases)
    reaches: Tuple[str, ...]       # the kernel paths this case is there for


@dataclass(frozen=True)
class BuildInput:
    spins: np.ndarray              # u64[K, 8], sorted by ls_bits512_cmp (word 0 first), unique
    counts: np.ndarray             # i64[K]
    psi: np.ndarray                # f64[K]
    other_spins: np.ndarray        # u64[N, 8]
    other_coeffs: np.ndarray       # f64[N]
    other_counts: np.ndarray       # i64[K]
    other_psi: np.ndarray          # f64[N]
    mixed: bool = False            # hits and misses are meant to be about even
    marks: dict = field(default_factory=dict, compare=False)   # what the structure tests look at

    @property
    def args(self):
        return (self.spins, self.counts, self.psi, self.other_spins, self.other_coeffs,
                self.other_counts, self.other_psi)

    @property
    def num_other(self):
        return int(self.other_spins.shape[0])


# ==================================================================================================
# the restatements
# ==================================================================================================
def keys512(keys):
    """u64[n] -> u64[n, 8] zero-padded; u64[n, 8] passes through."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim == 1:
        out = np.zeros((keys.shape[0], 8), dtype=np.uint64)
        out[:, 0] = keys
        return out
    assert keys.ndim == 2 and keys.shape[1] == 8
    return np.ascontiguousarray(keys)


def _whole_rows(rows):
    """One 64-byte string per key, big-endian words, word 0 first: byte order is ls_bits512_cmp."""
    return np.ascontiguousarray(keys512(rows).astype(">u8")).view("S64").reshape(-1)


def find(table, needles, *, word0_only=False, tail_ignored_without_tails=False, key0_absent=False,
         needle0_present=False):
    """i64[N]: index of every needle in the sorted unique table, -1 when absent — np.unique /
    searchsorted on the full 8-word rows.  The keyword arguments switch on the WRONG variants."""
    table, needles = keys512(table), keys512(needles)
    k, n = table.shape[0], needles.shape[0]
    if k == 0 or n == 0:
        return np.full(n, -1, dtype=np.int64)
    rows = _whole_rows(table)
    assert np.array_equal(np.unique(rows), rows), "the table is not sorted and unique"
    if word0_only or (tail_ignored_without_tails and not table[:, 1:].any()):
        # WRONG: the first key with the needle's word 0, whatever the other seven words say
        at = np.searchsorted(table[:, 0], needles[:, 0])
        hit = table[np.minimum(at, k - 1), 0] == needles[:, 0]
    else:
        wanted = _whole_rows(needles)
        at = np.searchsorted(rows, wanted)
        hit = rows[np.minimum(at, k - 1)] == wanted
    pos = np.where(hit, at, -1).astype(np.int64)
    zero = ~needles.any(axis=1)
    if key0_absent:            # WRONG: the all-zero slot is "empty", so key 0 is never found
        pos[zero] = -1
    if needle0_present:        # WRONG: an empty slot "matches" fingerprint 0 and yields index 0
        pos[zero & (pos < 0)] = 0
    return pos


def build_matrix(spins, counts, psi, other_spins, other_coeffs, other_counts, other_psi, *,
                 pairwise_field=False, field_from_first_term=False, signed_x_in_element=False,
                 abs_x_in_field=False, other_product_order=False, counts_through_int32=False,
                 counts_through_float32=False, empty_row_keeps_previous_field=False,
                 hits_in_column_order=False, **search):
    """``(nnz, row u32[nnz], col u32[nnz], elements f64[nnz], field f64[K])`` of the reference's
    build_matrix: the element of a hit is ((counts * coeff) * |psi|) * |x|, every product rounded
    on its own; the field of a row is the strict left-to-right sum, from +0.0, of
    ((counts * coeff) * |psi|) * x over its misses; hits in input order.  The keyword arguments
    switch on the WRONG variants (`search`: those of `find`)."""
    table = keys512(spins)
    counts = np.asarray(counts, dtype=np.int64)
    psi = np.asarray(psi, dtype=np.float64)
    coeffs = np.asarray(other_coeffs, dtype=np.float64)
    lengths = np.asarray(other_counts, dtype=np.int64)
    x = np.asarray(other_psi, dtype=np.float64)
    k = table.shape[0]
    pos = find(table, other_spins, **search)
    hit = pos >= 0
    row_of = np.repeat(np.arange(k, dtype=np.int64), lengths)
    if counts_through_int32:       # WRONG
        c = counts.astype(np.int32).astype(np.float64)
    elif counts_through_float32:   # WRONG
        c = counts.astype(np.float32).astype(np.float64)
    else:
        c = counts.astype(np.float64)            # exact i64 -> f64 conversion, round to nearest even
    a = np.abs(psi)
    if other_product_order:        # WRONG: (c * |psi|) * coeff
        head = (c[row_of] * a[row_of]) * coeffs
    else:
        head = (c[row_of] * coeffs) * a[row_of]
    elements = (head * (x if signed_x_in_element else np.abs(x)))[hit]
    row, col = row_of[hit].astype(np.uint32), pos[hit].astype(np.uint32)
    if hits_in_column_order:       # WRONG: the hits of a row sorted by column
        order = np.lexsort((col, row))
        col, elements = col[order], elements[order]
    terms = (head * (np.abs(x) if abs_x_in_field else x))[~hit]
    starts = np.searchsorted(row_of[~hit], np.arange(k + 1))
    out = np.zeros(k, dtype=np.float64)
    for r in np.nonzero(np.diff(starts))[0]:
        seg = terms[starts[r]:starts[r + 1]]
        if pairwise_field:             # WRONG: numpy's pairwise sum
            out[r] = np.sum(seg) + 0.0
        elif field_from_first_term:    # WRONG: f = t0, so a -0.0 survives
            out[r] = np.add.accumulate(seg)[-1]
        else:                          # ufunc.accumulate is sequential: ((0 + t0) + t1) + ...
            out[r] = np.add.accumulate(np.concatenate([[0.0], seg]))[-1]
    if empty_row_keeps_previous_field:   # WRONG: the accumulator is not reset for an empty row
        for r in range(1, k):
            if lengths[r] == 0:
                out[r] = out[r - 1]
    return int(hit.sum()), row, col, elements, out


BUILD_VARIANTS = {
    "compares word 0 only": dict(word0_only=True),
    "ignores a needle's tail when the table is single-word": dict(tail_ignored_without_tails=True),
    "treats key 0 as absent": dict(key0_absent=True),
    "treats an absent needle 0 as present at index 0": dict(needle0_present=True),
    "field by np.sum (pairwise)": dict(pairwise_field=True),
    "field starts from its first term (-0.0 survives)": dict(field_from_first_term=True),
    "signed x in an element": dict(signed_x_in_element=True),
    "|x| in the field": dict(abs_x_in_field=True),
    "product in the order (c * |psi|) * coeff": dict(other_product_order=True),
    "counts through int32": dict(counts_through_int32=True),
    "counts through float32": dict(counts_through_float32=True),
    "a row of count 0 keeps the previous row's field": dict(empty_row_keeps_previous_field=True),
    "hits in column order": dict(hits_in_column_order=True),
}


def extract_signs(psi, *, not_negative=False, by_sign_bit=False, not_less_equal=False):
    """u64[ceil(n / 64)]: bit i of word i / 64 set where psi[i] > 0 (NaN, +-0 -> clear), the bits
    above n clear.  The keyword arguments switch on the WRONG variants."""
    psi = np.asarray(psi, dtype=np.float64)
    n = psi.shape[0]
    with np.errstate(invalid="ignore"):
        if not_negative:        # WRONG: >= 0
            positive = psi >= 0
        elif by_sign_bit:       # WRONG: the sign bit alone (+0.0 and a positive NaN count)
            positive = ~np.signbit(psi)
        elif not_less_equal:    # WRONG: !(x <= 0), true for NaN
            positive = ~(psi <= 0)
        else:
            positive = psi > 0
    bits = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    bits[:n] = positive
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


SIGN_VARIANTS = {
    ">= 0": dict(not_negative=True),
    "the sign bit alone": dict(by_sign_bit=True),
    "!(x <= 0)": dict(not_less_equal=True),
}


# ==================================================================================================
# building blocks of the cases
# ==================================================================================================
def _sorted_table(rows):
    rows = keys512(rows)
    _, first = np.unique(_whole_rows(rows), return_index=True)    # sorted by ls_bits512_cmp, unique
    return np.ascontiguousarray(rows[first])


def _random_table(rng, k):
    """k single-word keys over the full uint64 range (bit 63 set in about half), never key 0."""
    keys = np.unique(rng.integers(1, 1 << 64, size=k, dtype=np.uint64, endpoint=False))
    assert keys.shape[0] == k
    return keys512(keys)


def _needles(rng, table, hit):
    """One needle per entry of `hit`: a random table key where it is set, else that key with one bit
    flipped (in word 0 for a single-word table, in any word otherwise) and checked to be absent."""
    k, n = table.shape[0], hit.shape[0]
    pick = rng.integers(0, k, size=n)
    out = table[pick].copy()
    multi = bool(table[:, 1:].any())
    miss = np.nonzero(~hit)[0]
    while miss.size:
        word = rng.integers(0, 8, size=miss.size) if multi else np.zeros(miss.size, dtype=np.int64)
        bit = rng.integers(0, 64, size=miss.size).astype(np.uint64)
        out[miss] = table[pick[miss]]
        out[miss, word] ^= np.uint64(1) << bit
        miss = miss[find(table, out[miss]) >= 0]
    return out


def _split(rng, n, k, empty=0.15):
    """n connections over k rows, about `empty` of the rows empty, the others of uneven length."""
    if k == 1:
        return np.array([n], dtype=np.int64)
    weight = rng.random(k) + 0.05
    weight[rng.random(k) < empty] = 0.0
    if not weight.any():
        weight[0] = 1.0
    return rng.multinomial(n, weight / weight.sum()).astype(np.int64)


def _plain_values(rng, k, n):
    """counts in {1, 2, 3}; both signs, exact zeros and -0.0, magnitudes over six decades — far from
    the subnormals, so that the rounding of every product shows and nothing underflows."""
    counts = rng.choice(np.array([1, 2, 3, 3], dtype=np.int64), size=k)
    psi = rng.choice([-1.0, 1.0], size=k) * 10.0 ** rng.uniform(-6.0, 0.0, size=k)
    psi[rng.random(k) < 0.05] = 0.0
    coeffs = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.1, 3.0, size=n)
    x = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 0.0, size=n)
    x[rng.random(n) < 0.03] = 0.0
    x[rng.random(n) < 0.03] = -0.0
    return counts, psi, coeffs, x


def _assemble(rng, table, lengths, hit, *, needles=None, mixed=False, marks=None, values=None):
    table = keys512(table)
    lengths = np.asarray(lengths, dtype=np.int64)
    k, n = table.shape[0], int(lengths.sum())
    assert lengths.shape[0] == k and hit.shape[0] == n
    if needles is None:
        needles = _needles(rng, table, hit) if n else np.zeros((0, 8), dtype=np.uint64)
    counts, psi, coeffs, x = values if values is not None else _plain_values(rng, k, n)
    return BuildInput(table, counts, psi, np.ascontiguousarray(needles), coeffs, lengths, x,
                      mixed=mixed, marks=dict(marks or {}))


def _case(name, fn, reaches, *args):
    return Case(name, lambda: _cached_input(fn, args), tuple(reaches))


@functools.lru_cache(maxsize=None)
def _cached_input(fn, args):
    return fn(*args)


# ==================================================================================================
# search / hash
# ==================================================================================================
SEARCH_N = (0, 1, 63, 64, 65, 2047, 2048, 2049, 131071, 131072, 131073)
SEARCH_K = (1, 32, 33, 200)


def search_n(n):
    """K = 200 single-word keys, n connections, half of them misses."""
    rng = np.random.default_rng(3000 + n % 1000 + n // 1000)
    table = _random_table(rng, 200)
    hit = rng.random(n) < 0.5
    return _assemble(rng, table, _split(rng, n, 200), hit, mixed=n >= 63)


def search_k(k):
    """k single-word keys and 150 connections (three groups, the last of 22), half misses."""
    rng = np.random.default_rng(3100 + k)
    hit = rng.random(150) < 0.5
    return _assemble(rng, _random_table(rng, k), _split(rng, 150, k), hit, mixed=True)


def key_zero(present):
    """33 single-word keys.  `present`: key 0 is table[0], a quarter of the needles are 0 (hits at
    column 0).  Otherwise the table starts at key 1 and the needles 0 are misses; table[0] is
    there to be returned by a kernel that takes an empty slot for fingerprint 0."""
    rng = np.random.default_rng(3200 + int(present))
    keys = np.unique(rng.integers(2, 1 << 64, size=32, dtype=np.uint64, endpoint=False))
    table = keys512(np.concatenate([[np.uint64(0 if present else 1)], keys]))
    lengths = _split(rng, 120, 33)
    hit = rng.random(120) < 0.5
    needles = _needles(rng, table, hit)
    zero = np.arange(120) % 4 == 0
    needles[zero] = 0
    # the needles next to key 0: 1 (absent or table[0]) and the needle whose only set bit is bit 63
    needles[1], needles[2] = keys512([1])[0], keys512([np.uint64(1) << np.uint64(63)])[0]
    return _assemble(rng, table, lengths, hit, needles=needles, mixed=True, marks=dict(zero=zero))


def key_zero_with_a_tail():
    """Multi-word table whose key with word 0 == 0 has a tail: the all-zero needle has its
    fingerprint (0) and its home bucket (0) and is absent; (0, tail) itself is present."""
    rng = np.random.default_rng(3210)
    rows = keys512(np.unique(rng.integers(1, 1 << 64, size=16, dtype=np.uint64, endpoint=False)))
    first = np.zeros((2, 8), dtype=np.uint64)
    first[0, 5], first[1, 7] = 9, U64_MAX
    table = _sorted_table(np.concatenate([first, rows]))
    hit = rng.random(90) < 0.5
    needles = _needles(rng, table, hit)
    needles[np.arange(90) % 4 == 0] = 0            # absent: every key with word 0 == 0 has a tail
    needles[np.arange(90) % 4 == 1] = first[0]     # present
    return _assemble(rng, table, _split(rng, 90, 18), hit, needles=needles, mixed=True)


def high_keys():
    """32 keys: 2^64 - 1, 2^63, 2^63 + 1, 2^64 - 2^32 (high word all ones), 2^32 - 1, 1 and random
    keys with bit 63 set; needles present, and absent next to them (2^64 - 2, 2^63 - 1)."""
    rng = np.random.default_rng(3300)
    top = np.uint64(1) << np.uint64(63)
    named = np.array([U64_MAX, top, top + np.uint64(1), U64_MAX - np.uint64(0xFFFFFFFF),
                      np.uint64(0xFFFFFFFF), np.uint64(1)], dtype=np.uint64)
    more = rng.integers(1 << 63, (1 << 64) - 2, size=64, dtype=np.uint64, endpoint=False)
    more = np.unique(more[~np.isin(more, named)])[:26]
    table = keys512(np.sort(np.concatenate([named, more])))
    assert table.shape[0] == 32
    hit = rng.random(130) < 0.5
    needles = _needles(rng, table, hit)
    needles[:8] = keys512([U64_MAX, U64_MAX - np.uint64(1), top, top - np.uint64(1), named[3], named[4],
                           np.uint64(1) << np.uint64(32), np.uint64(2)])
    return _assemble(rng, table, _split(rng, 130, 32), hit, needles=needles, mixed=True)


LAST_BUCKET_K = 200      # 512 slots, 64 buckets


@functools.lru_cache(maxsize=None)
def _integers_by_home():
    """The integers 1 .. 199 999 and their home buckets in a table of 200 keys."""
    candidates = np.arange(1, 200_000, dtype=np.uint64)
    return candidates, home_bucket(candidates, LAST_BUCKET_K)


def last_bucket(crowd, absent_into_it):
    """200 single-word keys of which `crowd` (9 or 17) have the LAST bucket (63) as their home;
    the others have homes 3 .. 62, at most four to a bucket, so that buckets 0, 1 and 2 receive
    only what overflows from bucket 63: with 9 the ninth key wraps to bucket 0, with 17 the chain
    is bucket 63 (full), bucket 0 (full), bucket 1.  Needles: every crowded key (present), other
    keys, and — `absent_into_it` — absent integers whose home is bucket 63 as well: they read the
    full bucket, wrap, and end at the first bucket with an empty slot."""
    rng = np.random.default_rng(3400 + crowd + int(absent_into_it))
    candidates, home = _integers_by_home()
    last = slot_count(LAST_BUCKET_K) // BUCKET - 1
    there = rng.permutation(candidates[home == last])
    crowded, strangers = there[:crowd], there[crowd:crowd + 40]
    rest = []
    for b in range(3, last):
        rest.append(rng.permutation(candidates[home == b])[:4])
    rest = rng.permutation(np.concatenate(rest))[:LAST_BUCKET_K - crowd]
    table = keys512(np.sort(np.concatenate([crowded, rest])))
    n = 260
    lengths = _split(rng, n, LAST_BUCKET_K)
    hit = rng.random(n) < 0.5
    needles = _needles(rng, table, hit)
    where = rng.permutation(n)
    needles[where[:crowd]] = keys512(crowded)
    marks = dict(crowded=crowded)
    if absent_into_it:
        at = where[crowd:crowd + strangers.shape[0]]
        needles[at] = keys512(strangers)
        marks["strangers"] = at
    return _assemble(rng, table, lengths, hit, needles=needles, mixed=True, marks=marks)


def tails_on_a_single_word_table():
    """33 single-word keys; two needles in three equal a key in word 0 and are non-zero in exactly
    one of the words 1 .. 7 (each word in turn; a single bit, bit 63, or all ones): every one of
    them is a miss, decided by `wanted` without a probe.  The others are plain hits."""
    rng = np.random.default_rng(3500)
    table = _random_table(rng, 33)
    n = 126
    pick = rng.integers(0, 33, size=n)
    needles = table[pick].copy()
    tailed = np.arange(n) % 3 != 0
    word = 1 + (np.arange(n) // 3) % 7
    value = np.array([1, 1 << 63, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)[(np.arange(n) // 21) % 3]
    needles[tailed, word[tailed]] = value[tailed]
    return _assemble(rng, table, _split(rng, n, 33), ~tailed, needles=needles,
                     marks=dict(tailed=tailed, word=word))


def one_word_differs(which):
    """20 keys that agree in seven words and differ in word `which` (7 or 1) only: one home bucket
    for all of them, so the table is a chain of two full buckets and four keys in a third, and every
    slot read carries the needle's fingerprint — the candidates loop of find_key runs eight times per
    bucket and the eight-word comparison decides.  Needles: present keys, and keys that agree in
    the seven words and are absent in word `which`."""
    rng = np.random.default_rng(3600 + which)
    base = rng.integers(1, 1 << 64, size=8, dtype=np.uint64, endpoint=False)
    values = np.unique(rng.integers(0, 1 << 64, size=40, dtype=np.uint64, endpoint=False))
    table = np.tile(base, (20, 1))
    table[:, which] = values[:20]
    table = _sorted_table(table)
    n = 100
    hit = rng.random(n) < 0.5
    needles = table[rng.integers(0, 20, size=n)].copy()
    needles[~hit, which] = values[20 + rng.integers(0, 20, size=int((~hit).sum()))]
    return _assemble(rng, table, _split(rng, n, 20), hit, needles=needles, mixed=True)


def only_the_last_key_has_a_tail():
    """33 keys, single-word but for the last: asp_build_upload's scan for a tail runs to the end of
    the table before it picks k_search_flat<true>.  Needles with a tail on a single-word key's word 0
    are misses now decided by the eight-word comparison; the last key is present, its word 0 with a
    zero tail absent."""
    rng = np.random.default_rng(3700)
    table = _random_table(rng, 33)
    table[32, 3] = 5
    n = 99
    hit = np.arange(n) % 3 == 0
    needles = table[rng.integers(0, 32, size=n)].copy()
    needles[np.arange(n) % 3 == 1, 1 + np.arange(n)[np.arange(n) % 3 == 1] % 7] = 7     # tailed: misses
    absent = np.arange(n) % 3 == 2
    needles[absent] = _needles(rng, table, np.zeros(int(absent.sum()), dtype=bool))
    needles[0] = table[32]                       # present (hit[0] is set)
    needles[2] = keys512([table[32, 0]])[0]      # the last key without its tail: absent
    return _assemble(rng, table, _split(rng, n, 33), hit, needles=needles, mixed=True)


# ==================================================================================================
# emission
# ==================================================================================================
ROW_PAIRS = ((0, 0), (0, 1), (1, 0), (32, 0), (0, 32), (31, 32), (32, 33), (33, 1), (64, 65), (65, 64),
             (1000, 0), (0, 1000))
MISS_PATTERNS = ("all hit", "all miss", "alternating", "only lane 31 misses",
                 "even row all-miss, odd row all-hit", "even row all-hit, odd row all-miss")


def row_pairs(pattern):
    """24 rows: rows (2 w, 2 w + 1) have the lengths ROW_PAIRS[w] and share a wavefront of
    k_emit_rows (three blocks of eight rows); `pattern` says which connections miss."""
    rng = np.random.default_rng(4000 + MISS_PATTERNS.index(pattern))
    lengths = np.array(ROW_PAIRS, dtype=np.int64).reshape(-1)
    k, n = lengths.shape[0], int(lengths.sum())
    row_of = np.repeat(np.arange(k), lengths)
    j = np.arange(n) - np.repeat(np.cumsum(lengths) - lengths, lengths)     # position inside the row
    hit = {"all hit": np.ones(n, dtype=bool), "all miss": np.zeros(n, dtype=bool),
           "alternating": j % 2 == 0, "only lane 31 misses": j % ROW_LANES != ROW_LANES - 1,
           "even row all-miss, odd row all-hit": row_of % 2 == 1,
           "even row all-hit, odd row all-miss": row_of % 2 == 0}[pattern]
    return _assemble(rng, _random_table(rng, k), lengths, hit, mixed=pattern == "alternating")


PARTIAL_K = (1, 7, 8, 9, 15, 17)


def partial_blocks(k):
    """k rows of 0 .. 70 connections: the last block (and, for odd k, the last wavefront) is partly
    rows that do not exist."""
    rng = np.random.default_rng(4100 + k)
    lengths = rng.integers(0, 71, size=k).astype(np.int64)
    lengths[-1] = 37                    # the last existing row emits and sums beside a missing one
    hit = rng.random(int(lengths.sum())) < 0.5
    return _assemble(rng, _random_table(rng, k), lengths, hit, mixed=True)


BLOCK_OFFSETS = (0, 63, 64, 65, 2047, 2048, 2049, 131071, 131072, 131073)
TRAILING_N = (131136, 133120, 262144)      # multiples of 64, of 2048 and of 131072 (and of no more)


def block_offsets(n, k):
    """Eleven blocks of eight rows whose first needles are BLOCK_OFFSETS and then `n` itself: the
    last block has empty rows only (k = 88), or empty rows and rows that do not exist (k < 88).
    Half of the needles miss; the needles 0, 64, 2048 and 131072 — the only ones counted by a sum
    that would otherwise be empty for some block — are hits."""
    rng = np.random.default_rng(4200 + n % 977)
    starts = np.array(BLOCK_OFFSETS + (n,), dtype=np.int64)
    lengths = np.zeros(88, dtype=np.int64)
    for b, total in enumerate(np.diff(starts)):
        lengths[8 * b:8 * b + 8] = _split(rng, int(total), 8, empty=0.25)
    lengths = lengths[:k]
    assert int(lengths.sum()) == n
    hit = rng.random(n) < 0.5
    hit[[0, 64, 2048, 131072]] = True
    return _assemble(rng, _random_table(rng, k), lengths, hit, mixed=True)


# ==================================================================================================
# values
# ==================================================================================================
COUNT_VALUES = (0, 1, 3, 2 ** 31 + 1, 2 ** 53 + 1, -2)


def wide_values():
    """34 rows of 40 connections, half misses.  counts cycle through COUNT_VALUES; |psi| and |x|
    span 1e-160 .. 1e2 with exact zeros, -0.0 and subnormal inputs, so that many products land in
    the subnormal range (rounded there) or underflow to a signed zero; nothing can overflow:
    |count * coeff * psi * x| <= 2^53 * 8 * 1e2 * 1e2."""
    rng = np.random.default_rng(5000)
    k, per = 34, 40
    n = k * per
    counts = np.array(COUNT_VALUES, dtype=np.int64)[np.arange(k) % len(COUNT_VALUES)]
    psi = rng.choice([-1.0, 1.0], size=k) * 10.0 ** rng.uniform(-160.0, 2.0, size=k)
    x = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-160.0, 2.0, size=n)
    coeffs = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.125, 8.0, size=n)
    psi[[6, 7, 8, 9, 10, 11]] = [0.0, -0.0, 3e-310, -5e-324, 1e-158, -1e-150]
    psi[12:18] = rng.choice([-1.0, 1.0], size=6) * 10.0 ** rng.uniform(-1.0, 2.0, size=6)   # one of each count
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1e-310, 1e-155, -1e-165])
    x[rng.permutation(n)[:160]] = np.tile(special, 20)
    hit = rng.random(n) < 0.5
    return _assemble(rng, _random_table(rng, k), np.full(k, per), hit, mixed=True,
                     values=(counts, psi, coeffs, x))


def minus_zero_rows():
    """Rows whose misses ALL contribute -0.0, each in its own way: x = -0.0 under a positive head;
    a coefficient of -0.0; products that underflow from below (-1e-200 * 1e-200); a count of 0
    with negative x; psi = -0.0 (|psi| = +0.0) with negative x.  The reference's sum starts from
    +0.0, so these fields are +0.0.  A row of +0.0 terms, rows with one hit between the misses and
    a row whose -0.0 terms are followed by a real one stand beside them."""
    rng = np.random.default_rng(5100)
    table = _random_table(rng, 16)
    per = 6
    k, n = 16, 16 * per
    counts = np.ones(k, dtype=np.int64)
    psi = np.ones(k)
    coeffs = np.ones(n).reshape(k, per)
    x = -rng.uniform(0.5, 2.0, size=n).reshape(k, per)
    hit = np.zeros((k, per), dtype=bool)
    x[0] = -0.0
    coeffs[1] = -0.0; x[1] = np.abs(x[1])
    psi[2] = 1e-200; x[2] = -1e-200
    counts[3] = 0
    psi[4] = -0.0
    x[5] = 0.0                                   # +0.0 terms
    x[6] = -0.0; hit[6, 2] = True                # a hit between the -0.0 misses
    x[7] = -0.0; x[7, per - 1] = 0.75            # ... followed by a real term
    x[8] = -0.0; x[8, 0] = -0.75                 # a real term first
    x[9] = -0.0; hit[9, 1:] = True               # one miss only
    psi[10] = -1e-200; x[10] = -1e-200           # |psi|: still -0.0 terms
    hit[11] = True                               # no miss at all: +0.0
    x[12] = -5e-324; coeffs[12] = 0.25           # subnormal * 0.25 rounds to -0.0
    hit[13:, ::2] = True
    return _assemble(rng, table, np.full(k, per), hit.reshape(-1), values=(
        counts, psi, coeffs.reshape(-1), x.reshape(-1)), marks=dict(minus_zero_rows=(0, 1, 2, 3, 4, 10, 12)))


def cancelling_row():
    """Three rows; the middle one has 300 misses (and 20 hits between them) whose terms are pairs
    +-B with B over 1e10 .. 1e16 and small terms of order 1, shuffled: the left-to-right sum loses
    the small terms wherever a large partial sum stands, so another order of summation differs in
    the leading digits.  head = 1 exactly (count 1, coefficient 1, psi -1), so the terms are x."""
    rng = np.random.default_rng(5200)
    big = 10.0 ** rng.uniform(10.0, 16.0, size=120)
    terms = rng.permutation(np.concatenate([big, -big, rng.uniform(1.0, 9.0, size=60)]))
    lengths = np.array([5, 320, 0], dtype=np.int64)
    hit = np.zeros(325, dtype=bool)
    hit[5 + rng.permutation(320)[:20]] = True
    x = np.empty(325)
    x[~hit] = np.concatenate([rng.uniform(-1.0, 1.0, size=5), terms])
    x[hit] = rng.uniform(-1.0, 1.0, size=20)
    values = (np.ones(3, dtype=np.int64), np.array([0.5, -1.0, 2.0]), np.ones(325), x)
    return _assemble(rng, _random_table(rng, 3), lengths, hit, values=values)


# ==================================================================================================
# the handle path and the one large case
# ==================================================================================================
HANDLE_N = 2 * SUPER + CHUNK + 5       # three super-chunks, the last of one chunk and five needles
HANDLE_K = 200


def handle_upload(which):
    """Two uploads for ONE asp_build handle: the same K, the same row lengths.  "A" has a
    single-word table (k_search_flat<false>) and 60 % hits; "B" another table, multi-word with
    few distinct first words (k_search_flat<true>, long chains), 35 % hits at other places, and
    other values.  A build that left a slot of A's table behind would find B's needles at A's
    indices, or fill B's hash."""
    lengths = _split(np.random.default_rng(6000), HANDLE_N, HANDLE_K)
    rng = np.random.default_rng(6001 if which == "A" else 6002)
    if which == "A":
        table = _random_table(rng, HANDLE_K)
    else:
        rows = rng.integers(0, 3, size=(4 * HANDLE_K, 8), dtype=np.uint64)
        rows[:, 0] = rng.integers(0, 12, size=4 * HANDLE_K, dtype=np.uint64) << np.uint64(40)
        table = _sorted_table(rows)
        table = table[np.sort(rng.permutation(table.shape[0])[:HANDLE_K])]
        assert table.shape[0] == HANDLE_K
    hit = rng.random(HANDLE_N) < (0.6 if which == "A" else 0.35)
    return _assemble(rng, table, lengths, hit, mixed=True)


LARGE_N = 65 * SUPER + CHUNK + 77      # the smallest size at which `t += 64` (:332) takes a second step
LARGE_K = 3001


def large_lengths():
    """Only a block whose first needle is one of the last CHUNK + 77 takes the second step, so the
    last 17 rows (the last three blocks) have 100 connections each; 200 rows are empty and one
    has two super-chunks more than the others (8192 trips of its half-wavefront)."""
    rng = np.random.default_rng(7000)
    head = LARGE_K - 17
    weight = np.ones(head)
    weight[rng.permutation(head)[:200]] = 0.0
    lengths = np.full(LARGE_K, 100, dtype=np.int64)
    lengths[:head] = rng.multinomial(LARGE_N - 1700 - 2 * SUPER, weight / weight.sum())
    lengths[1500] += 2 * SUPER
    return lengths


def large():
    """65 super-chunks and a little: the blocks whose first needle lies beyond super-chunk 64 add
    super_total[64] in a second step of the loop at :332.  Single-word even keys; a miss is the
    key plus one.  NOT cached: 550 MB of needles, made for one test and freed after it."""
    rng = np.random.default_rng(7001)
    keys = np.unique(rng.integers(1, 1 << 63, size=LARGE_K + 64, dtype=np.uint64, endpoint=False) << np.uint64(1))
    keys = keys[:LARGE_K]
    assert keys.shape[0] == LARGE_K
    lengths = large_lengths()
    hit = rng.random(LARGE_N) < 0.5
    needles = np.zeros((LARGE_N, 8), dtype=np.uint64)
    needles[:, 0] = keys[rng.integers(0, LARGE_K, size=LARGE_N)] | (~hit).astype(np.uint64)
    counts = rng.choice(np.array([1, 2, 3], dtype=np.int64), size=LARGE_K)
    psi = rng.choice([-1.0, 1.0], size=LARGE_K) * rng.uniform(1e-3, 1.0, size=LARGE_K)
    coeffs = rng.uniform(-3.0, 3.0, size=LARGE_N)
    x = rng.uniform(-1.0, 1.0, size=LARGE_N)
    return BuildInput(keys512(keys), counts, psi, needles, coeffs, lengths, x, mixed=True)


# ==================================================================================================
# the tables
# ==================================================================================================
BUILD_CASES = tuple(
    _case("search N=%d" % n, search_n, (
        {0: "N = 0: k_search_flat is not launched, k_emit_rows reads no look-up result",
         1: "N = 1: one lane of one group wanted; every clamped load re-reads the last 16 bytes"}.get(
             n, "N = %d: %d groups, %d chunks, %d super-chunks; the last group has %d needles" % (
                 n, -(-n // GROUP), -(-n // CHUNK), -(-n // SUPER), (n - 1) % GROUP + 1)),
        "K = 200: 512 slots, 64 buckets"), n)
    for n in SEARCH_N
) + tuple(
    _case("search K=%d" % k, search_k, (
        "K = %d: %d slots, %d buckets" % (k, slot_count(k), slot_count(k) // BUCKET),), k)
    for k in SEARCH_K[:3]
) + (
    _case("key 0 in the table", key_zero, (
        "find_key: fingerprint 0 in home bucket 0, told from the empty slots by `match &= ~empty` (:149)",
        "k_insert_keys: entry = 0 | (0 + 1), a non-zero slot"), True),
    _case("needle 0, key 0 absent", key_zero, (
        "find_key: every empty slot of bucket 0 carries fingerprint 0 and must not be a candidate",), False),
    _case("key (0, tail) and needle 0", key_zero_with_a_tail, (
        "find_key: a real candidate with fingerprint 0 that the eight-word comparison rejects",)),
    _case("keys with bit 63, 2^64-1", high_keys, (
        "mix64, fingerprint = h >> 32 and h & bucket_mask on keys with the high bits set",)),
    _case("9 keys at home in the last bucket", last_bucket, (
        "k_insert_keys / find_key: a full home bucket, b = (b + 1) & bucket_mask wraps 63 -> 0",), 9, False),
    _case("17 keys at home in the last bucket", last_bucket, (
        "find_key: a chain over two full buckets (63, 0) into a third",), 17, False),
    _case("absent needles into the full last bucket", last_bucket, (
        "find_key: no candidate and no empty slot: moves on; -1 only at the first bucket with an empty slot",),
        9, True),
    _case("absent needles into two full buckets", last_bucket, (
        "find_key: an absent needle walks the chain 63, 0, 1",), 17, True),
    _case("tails on a single-word table", tails_on_a_single_word_table, (
        "k_search_flat<false>: `wanted` (:232) is false for a needle with a non-zero word 1 .. 7",
        "each of the words 1 .. 7 in turn, so `needle_tail |= key[w]` covers all seven")),
    _case("20 keys differ in word 7 only", one_word_differs, (
        "verify: the last word of the eight-word comparison decides",
        "find_key: eight candidates with the needle's fingerprint per bucket, three buckets"), 7),
    _case("20 keys differ in word 1 only", one_word_differs, (
        "verify: the first word after table0 decides",), 1),
    _case("only the last key has a tail", only_the_last_key_has_a_tail, (
        "asp_build_upload: the scan for a tail (:533-538) finds it at the last key",
        "k_search_flat<true> on needles with a tail whose word 0 is a single-word key")),
) + tuple(
    _case("row pairs, %s" % pattern, row_pairs, (
        "k_emit_rows: the two halves of a wavefront run the longer row's `trips` and the larger `rounds`",
        "row lengths (even, odd) = " + " ".join("%d,%d" % p for p in ROW_PAIRS),
        "misses: " + pattern), pattern)
    for pattern in MISS_PATTERNS
) + tuple(
    _case("rows K=%d" % k, partial_blocks, (
        "k_emit_rows: row_ok false for %d of the last block's rows%s" % (
            -k % ROWS_PER_BLOCK, ", the last row's half-wavefront beside a row that does not exist" if k % 2 else ""),),
        k)
    for k in PARTIAL_K
) + tuple(
    _case("block offsets, N=%d K=%d" % (n, k), block_offsets, (
        "k_emit_rows: first needle of a block o = " + ", ".join(map(str, BLOCK_OFFSETS)) + " and N",
        "o = N = %d, a multiple of %d: the last block %s" % (
            n, unit, "has empty rows only" if k == 88 else "has empty rows and rows that do not exist"),
        "each of the four partial sums (:326-345) alone, and zero beside the others"), n, k)
    for n, k, unit in zip(TRAILING_N, (88, 85, 88), (GROUP, CHUNK, SUPER))
) + (
    _case("wide values", wide_values, (
        "i64 -> f64 of counts 0, 1, 3, 2^31 + 1, 2^53 + 1 (rounds to 2^53), -2",
        "__dmul_rn on subnormal inputs and results; products that underflow to a signed zero")),
    _case("rows of -0.0 misses", minus_zero_rows, (
        "k_emit_rows: f starts from +0.0 (:367), so a row whose misses all contribute -0.0 has field +0.0",)),
    _case("cancelling row", cancelling_row, (
        "k_emit_rows: the strict left-to-right __dadd_rn over 300 misses in ten trips",)),
    _case("handle upload A", handle_upload, (
        "three super-chunks through one handle; k_search_flat<false>",), "A"),
    _case("handle upload B", handle_upload, (
        "the same shape with a multi-word table: k_search_flat<true>, other hits",), "B"),
)

LARGE_CASE = Case("large", large, (
    "k_emit_rows: more than 64 super-chunks, the second step of `for (t = lane; t < s0; t += 64)` (:332)",
    "a row of two super-chunks; offsets beyond 2^23"))


@functools.lru_cache(maxsize=None)
def _build_oracle(name):
    import oracle

    return oracle.build_matrix(*{c.name: c for c in BUILD_CASES}[name].make().args)


def build_oracle(case):
    """oracle.build_matrix on the case: ``(nnz, row, col, elements, field)``, computed on first use,
    shared by every test, never modified.  (Not for LARGE_CASE.)"""
    return _build_oracle(case.name)


# -- extract_signs ---------------------------------------------------------------------------------
SIGN_N = (1, 63, 64, 65, 255, 256, 257, 511, 513, 4097)


def sign_values(n):
    """n values drawn from {+x, -x, +0.0, -0.0, NaN, +inf, -inf, 5e-324, -5e-324}; the last one is
    5e-324, the smallest positive double: bit n - 1 is set and everything above it must not be."""
    rng = np.random.default_rng(8000 + n)
    x = 10.0 ** rng.uniform(-300.0, 300.0, size=n)
    kinds = np.stack([x, -x] + [np.full(n, v) for v in (0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324)])
    which = rng.integers(0, 9, size=n)
    which[:min(n, 9)] = rng.permutation(9)[:min(n, 9)]          # every kind once where there is room
    if n > 9:
        which[-10:-1] = rng.permutation(9)                      # ... and once more at the far end
    psi = kinds[which, np.arange(n)]
    psi[-1] = 5e-324
    if n > 1:
        psi[0] = -np.nan
    return psi


SIGN_CASES = tuple(
    Case("signs n=%d" % n, functools.partial(_cached_input, sign_values, (n,)), (
        "k_extract_signs: %d words, %d workgroups of 256; the last word has %d bits" % (
            -(-n // 64), -(-n // 256), (n - 1) % 64 + 1),
        "psi > 0 on NaN, +-0.0, +-inf and the smallest subnormals"))
    for n in SIGN_N)
