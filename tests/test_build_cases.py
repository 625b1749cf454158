"""The table of tests/build_cases.py still does what it is there for — asserted on the CPU (no GPU,
nothing compiled besides the oracle): the numpy restatements of `build_matrix` and `extract_signs`
equal the oracle bit for bit on every case, every named WRONG variant is told apart from the right
answer by at least one named case, and the structure the cases name is really in their inputs: the
crowded last bucket, the absent needles that land in it, the block offsets on the 64 / 2048 /
131072 boundaries, the four partial sums, the row-length pairs, the hit shares.
tests/test_gpu_build_edges.py then compares the kernels of csrc/build_matrix.hip with the oracle
on the same cases."""
import numpy as np
import pytest

import oracle

import build_cases as cases

VARIANT_LIMIT = 10_000      # connections: the variants and the reference binary run on the cases below


def _bytes(outputs):
    nnz, *arrays = outputs
    return (int(nnz),) + tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _by_name():
    return {case.name: case for case in cases.BUILD_CASES}


def _hit(x):
    return cases.find(x.spins, x.other_spins) >= 0


def test_case_names_are_unique_and_every_case_states_its_purpose():
    table = cases.BUILD_CASES + (cases.LARGE_CASE,) + cases.SIGN_CASES
    assert len({case.name for case in table}) == len(table)
    assert all(case.reaches and all(case.reaches) for case in table)


def test_the_constants_are_the_kernels():
    """mix64 is the splitmix64 finaliser (its published first output for seed 0 is mix64 of the
    golden-ratio increment); 3153 of the integers below 200 000 have the last of 64 buckets as
    their home."""
    assert int(cases.mix64(0)[0]) == 0
    assert int(cases.mix64(0x9E3779B97F4A7C15)[0]) == 0xE220A8397B1DCDAF
    assert [cases.slot_count(k) for k in (0, 1, 32, 33, 64, 65, 200, 3001)] == [64, 64, 64, 128, 128, 256, 512, 8192]
    candidates, home = cases._integers_by_home()
    assert home.min() == 0 and home.max() == 63 and int(np.sum(home == 63)) == 3153
    assert (cases.GROUP, cases.CHUNK, cases.SUPER, cases.BUCKET) == (64, 2048, 131072, 8)
    assert cases.ROWS_PER_BLOCK * cases.ROW_LANES == 256


def test_find_agrees_with_python_integers():
    """`find` orders 64-byte strings; the same look-up with tuples of Python integers."""
    for name in ("20 keys differ in word 7 only", "keys with bit 63, 2^64-1", "handle upload B",
                 "key (0, tail) and needle 0"):
        x = _by_name()[name].make()
        keys = [tuple(int(w) for w in row) for row in x.spins]
        assert keys == sorted(set(keys)), name
        position = {key: i for i, key in enumerate(keys)}
        some = np.random.default_rng(1).permutation(x.num_other)[:300]
        got = cases.find(x.spins, x.other_spins[some])
        assert got.tolist() == [position.get(tuple(int(w) for w in x.other_spins[e]), -1) for e in some], name


def test_build_restatement_equals_the_oracle_on_every_case():
    for case in cases.BUILD_CASES:
        x = case.make()
        assert not any(np.isnan(a).any() or np.isinf(a).any() for a in (x.psi, x.other_coeffs, x.other_psi))
        mine = cases.build_matrix(*x.args)
        theirs = cases.build_oracle(case)
        assert mine[1].dtype == np.uint32 and mine[3].dtype == np.float64
        assert not np.isnan(theirs[3]).any() and not np.isnan(theirs[4]).any(), case.name
        assert np.all(np.isfinite(theirs[3])) and np.all(np.isfinite(theirs[4])), case.name
        assert _bytes(mine) == _bytes(theirs), case.name


def test_oracle_equals_the_reference_binary_on_the_small_cases():
    if oracle.ref_lib() is None:
        pytest.skip("the reference binary (oracle/_ref) is not built here")
    checked = 0
    for case in cases.BUILD_CASES:
        x = case.make()
        if x.num_other < VARIANT_LIMIT:
            assert _bytes(oracle.ref_build_matrix(*x.args)) == _bytes(cases.build_oracle(case)), case.name
            checked += 1
    assert checked >= 30
    for case in cases.SIGN_CASES:
        psi = case.make()
        assert np.array_equal(oracle.ref_extract_signs(psi), oracle.extract_signs(psi)), case.name


def test_every_wrong_build_variant_is_told_apart_by_a_named_case():
    told = {name: [] for name in cases.BUILD_VARIANTS}
    for case in cases.BUILD_CASES:
        x = case.make()
        if x.num_other >= VARIANT_LIMIT:
            continue
        right = _bytes(cases.build_oracle(case))
        for name, switches in cases.BUILD_VARIANTS.items():
            if _bytes(cases.build_matrix(*x.args, **switches)) != right:
                told[name].append(case.name)
    print("\n".join("%s: %s" % item for item in told.items()))
    assert all(told.values()), "variants no case tells apart: %r" % [n for n, w in told.items() if not w]
    # the tail, key 0 and -0.0: by the case written for it
    assert "tails on a single-word table" in told["compares word 0 only"]
    assert "tails on a single-word table" in told["ignores a needle's tail when the table is single-word"]
    assert "20 keys differ in word 7 only" in told["compares word 0 only"]
    assert "20 keys differ in word 7 only" not in told["ignores a needle's tail when the table is single-word"]
    assert "key 0 in the table" in told["treats key 0 as absent"]
    assert "needle 0, key 0 absent" in told["treats an absent needle 0 as present at index 0"]
    assert "key (0, tail) and needle 0" in told["treats an absent needle 0 as present at index 0"]
    assert "rows of -0.0 misses" in told["field starts from its first term (-0.0 survives)"]
    assert "cancelling row" in told["field by np.sum (pairwise)"]
    assert "wide values" in told["counts through int32"] and "wide values" in told["counts through float32"]


def test_summation_order_shows_in_the_leading_digits():
    case = _by_name()["cancelling row"]
    x = case.make()
    right = cases.build_oracle(case)[4][1]
    other = cases.build_matrix(*x.args, pairwise_field=True)[4][1]
    misses = int(x.other_counts[1]) - int(np.sum(cases.build_oracle(case)[1] == 1))
    assert misses >= 200
    assert abs(right - other) > 1e-3 * max(abs(right), abs(other)), (right, other)


def test_values_reach_what_they_name():
    x = _by_name()["wide values"].make()
    assert set(x.counts.tolist()) == set(cases.COUNT_VALUES)
    for values in (x.psi, x.other_psi):
        mag = np.abs(values[values != 0])
        assert np.log10(mag.max()) - np.log10(mag.min()) > 12       # more than twelve decades
        assert np.any(values == 0) and np.any(np.signbit(values) & (values == 0))
        assert np.any(mag < 2.2250738585072014e-308)                     # subnormal inputs
    _, _, _, elements, field = cases.build_oracle(_by_name()["wide values"])
    tiny = np.abs(elements[elements != 0]) < 2.2250738585072014e-308
    assert tiny.sum() >= 5, "no product lands in the subnormal range"
    assert np.any(elements == 0) and np.any(np.abs(elements) > 1e10)
    assert np.any(field != 0)
    # rows of -0.0 misses: every term of the marked rows is -0.0 and the field is +0.0
    case = _by_name()["rows of -0.0 misses"]
    x = case.make()
    hit = _hit(x)
    row_of = np.repeat(np.arange(x.spins.shape[0]), x.other_counts)
    head = (x.counts[row_of].astype(np.float64) * x.other_coeffs) * np.abs(x.psi[row_of])
    terms = head * x.other_psi
    field = cases.build_oracle(case)[4]
    assert len(x.marks["minus_zero_rows"]) >= 5
    for r in x.marks["minus_zero_rows"]:
        mine = terms[(row_of == r) & ~hit]
        assert mine.size >= 2 and np.all(mine == 0) and np.all(np.signbit(mine)), r
        assert field[r] == 0 and not np.signbit(field[r]), r


def test_search_cases_reach_the_stated_structure():
    by_name = _by_name()
    assert [by_name["search N=%d" % n].make().num_other for n in cases.SEARCH_N] == list(cases.SEARCH_N)
    assert all(by_name["search N=%d" % n].make().spins.shape[0] == 200 for n in cases.SEARCH_N)
    assert [by_name["search K=%d" % k].make().spins.shape[0] for k in (1, 32, 33)] == [1, 32, 33]
    assert cases.slot_count(32) == 64 and cases.slot_count(33) == 128
    # key 0
    x = by_name["key 0 in the table"].make()
    zero = ~x.other_spins.any(axis=1)
    assert not x.spins[0].any() and zero.sum() >= 20 and np.all(cases.find(x.spins, x.other_spins)[zero] == 0)
    x = by_name["needle 0, key 0 absent"].make()
    zero = ~x.other_spins.any(axis=1)
    assert x.spins[0].any() and zero.sum() >= 20 and np.all(cases.find(x.spins, x.other_spins)[zero] == -1)
    x = by_name["key (0, tail) and needle 0"].make()
    zero = ~x.other_spins.any(axis=1)
    assert np.sum(x.spins[:, 0] == 0) == 2 and zero.sum() >= 20 and not np.any(_hit(x)[zero])
    # high keys
    x = by_name["keys with bit 63, 2^64-1"].make()
    assert x.spins[-1, 0] == cases.U64_MAX and np.sum(x.spins[:, 0] >> np.uint64(63)) >= 26
    assert np.any((x.other_spins[:, 0] == cases.U64_MAX) & _hit(x))
    assert np.any((x.other_spins[:, 0] == cases.U64_MAX - np.uint64(1)) & ~_hit(x))
    # the crowded last bucket
    for name, crowd, strangers in (("9 keys at home in the last bucket", 9, False),
                                   ("17 keys at home in the last bucket", 17, False),
                                   ("absent needles into the full last bucket", 9, True),
                                   ("absent needles into two full buckets", 17, True)):
        x = by_name[name].make()
        assert x.spins.shape[0] == 200 and not x.spins[:, 1:].any()
        home = cases.home_bucket(x.spins[:, 0], 200)
        occupancy = np.bincount(home, minlength=64)
        assert occupancy[63] == crowd >= cases.BUCKET + 1, name
        assert occupancy[:3].sum() == 0 and occupancy[3:63].max() <= 4, name    # the overflow alone fills 0, 1
        hit = _hit(x)
        crowded = np.isin(x.other_spins[:, 0], x.marks["crowded"])
        assert set(x.other_spins[crowded, 0].tolist()) == set(x.marks["crowded"].tolist()), name
        assert np.all(hit[crowded]), name
        if strangers:
            at = x.marks["strangers"]
            assert at.shape[0] >= 30 and not np.any(hit[at]), name
            assert np.all(cases.home_bucket(x.other_spins[at, 0], 200) == 63), name
    # tails
    x = by_name["tails on a single-word table"].make()
    tailed = x.marks["tailed"]
    assert not x.spins[:, 1:].any()
    assert np.all(np.isin(x.other_spins[:, 0], x.spins[:, 0]))                      # word 0 is always a key
    assert np.all(np.count_nonzero(x.other_spins[tailed, 1:], axis=1) == 1)         # exactly one tail word
    assert {int(w) for w in np.nonzero(x.other_spins[tailed, 1:])[1] + 1} == set(range(1, 8))
    assert np.array_equal(_hit(x), ~tailed) and tailed.sum() >= 80
    for which in (7, 1):
        x = by_name["20 keys differ in word %d only" % which].make()
        same = [w for w in range(8) if np.all(x.spins[:, w] == x.spins[0, w])]
        assert x.spins.shape[0] == 20 and same == [w for w in range(8) if w != which]
        others = [w for w in range(8) if w != which]
        assert np.all(x.other_spins[:, others] == x.spins[0, others])
    x = by_name["only the last key has a tail"].make()
    assert not x.spins[:-1, 1:].any() and x.spins[-1, 1:].any()
    tailed = x.other_spins[:, 1:].any(axis=1)
    assert np.sum(tailed & ~_hit(x) & np.isin(x.other_spins[:, 0], x.spins[:-1, 0])) >= 30
    assert np.any(tailed & _hit(x))


def _block_parts(x):
    """Per block of eight rows: its first needle o and the four partial sums of :326-345."""
    hit = _hit(x)
    offsets = np.concatenate([[0], np.cumsum(x.other_counts)])
    out = []
    for o in offsets[:-1][::cases.ROWS_PER_BLOCK].tolist():
        g0 = o // cases.GROUP
        c0 = g0 // (cases.CHUNK // cases.GROUP)
        s0 = c0 // (cases.SUPER // cases.CHUNK)
        out.append((o, (int(hit[:s0 * cases.SUPER].sum()), int(hit[s0 * cases.SUPER:c0 * cases.CHUNK].sum()),
                        int(hit[c0 * cases.CHUNK:g0 * cases.GROUP].sum()), int(hit[g0 * cases.GROUP:o].sum()))))
    return out


def test_emission_cases_reach_the_stated_structure():
    by_name = _by_name()
    # the pairs at (even, odd) rows, under every pattern
    for pattern in cases.MISS_PATTERNS:
        x = by_name["row pairs, %s" % pattern].make()
        lengths = x.other_counts.tolist()
        assert tuple(zip(lengths[0::2], lengths[1::2])) == cases.ROW_PAIRS
        hit = _hit(x)
        row_of = np.repeat(np.arange(len(lengths)), x.other_counts)
        j = np.arange(hit.shape[0]) - np.repeat(np.cumsum(x.other_counts) - x.other_counts, x.other_counts)
        if pattern == "all hit":
            assert hit.all()
        elif pattern == "all miss":
            assert not hit.any()
        elif pattern == "alternating":
            assert np.array_equal(hit, j % 2 == 0)
        elif pattern == "only lane 31 misses":
            assert np.array_equal(~hit, j % 32 == 31) and (~hit).sum() >= 60
        else:
            assert np.array_equal(hit, row_of % 2 == (1 if pattern.startswith("even row all-miss") else 0))
    assert {(0, 0), (0, 1), (1, 0), (32, 0), (0, 32), (31, 32), (32, 33), (33, 1), (64, 65), (65, 64), (1000, 0),
            (0, 1000)} == set(cases.ROW_PAIRS)
    assert [by_name["rows K=%d" % k].make().spins.shape[0] for k in cases.PARTIAL_K] == [1, 7, 8, 9, 15, 17]
    # the block offsets and the four partial sums
    units = []
    for n, k in zip(cases.TRAILING_N, (88, 85, 88)):
        x = by_name["block offsets, N=%d K=%d" % (n, k)].make()
        parts = _block_parts(x)
        assert [o for o, _ in parts] == list(cases.BLOCK_OFFSETS) + [n] and x.num_other == n
        assert x.spins.shape[0] == k and not x.other_counts[80:].any()
        sums = np.array([p for _, p in parts])
        for level in range(4):
            assert np.any(sums[:, level] > 0), (n, level)
            others = np.delete(sums, level, axis=1).sum(axis=1)
            assert np.any((sums[:, level] == 0) & (others > 0)), (n, level)      # zero beside non-zero others
            assert np.any((sums[:, level] > 0) & (others == 0)), (n, level)      # ... and alone
        units.append(max(u for u in (cases.GROUP, cases.CHUNK, cases.SUPER) if n % u == 0))
    assert units == [cases.GROUP, cases.CHUNK, cases.SUPER]
    # the handle's uploads: the same shape, three super-chunks, the search instantiation changes
    a, b = by_name["handle upload A"].make(), by_name["handle upload B"].make()
    assert a.num_other == b.num_other == 2 * cases.SUPER + cases.CHUNK + 5
    assert np.array_equal(a.other_counts, b.other_counts) and a.spins.shape == b.spins.shape
    assert not a.spins[:, 1:].any() and b.spins[:, 1:].any()
    assert abs(_hit(a).mean() - _hit(b).mean()) > 0.1
    # the large case (its inputs are not made here: 550 MB)
    lengths = cases.large_lengths()
    n = int(lengths.sum())
    assert n == cases.LARGE_N == 65 * 131072 + 2048 + 77 and lengths.shape[0] == cases.LARGE_K == 3001
    assert -(-n // cases.SUPER) > 64
    firsts = np.concatenate([[0], np.cumsum(lengths)])[:-1][::cases.ROWS_PER_BLOCK]
    assert np.sum(firsts // cases.SUPER > 64) == 3, "no block adds a 65th super-chunk total"
    assert lengths.max() > 2 * cases.SUPER and np.sum(lengths == 0) >= 100


def test_mixed_cases_keep_both_branches_busy():
    shares = {}
    for case in cases.BUILD_CASES:
        x = case.make()
        if x.mixed:
            shares[case.name] = float(_hit(x).mean())
    print(shares)
    assert len(shares) >= 30
    assert all(0.3 <= share <= 0.7 for share in shares.values()), shares


# -- extract_signs ---------------------------------------------------------------------------------
def test_sign_restatement_equals_the_oracle_and_every_wrong_variant_is_told_apart():
    told = {name: [] for name in cases.SIGN_VARIANTS}
    assert [case.make().shape[0] for case in cases.SIGN_CASES] == list(cases.SIGN_N)
    for case in cases.SIGN_CASES:
        psi = case.make()
        n = psi.shape[0]
        right = oracle.extract_signs(psi)
        mine = cases.extract_signs(psi)
        assert mine.dtype == np.uint64 and np.array_equal(mine, right), case.name
        assert psi[-1] == 5e-324 and (int(right[-1]) >> ((n - 1) % 64)) == 1, case.name   # nothing above bit n - 1
        if n >= 63:
            for kind in (np.isnan(psi), np.isposinf(psi), np.isneginf(psi), (psi == 0) & np.signbit(psi),
                         (psi == 0) & ~np.signbit(psi), psi == 5e-324, psi == -5e-324):
                assert kind.any(), case.name
            assert np.any(np.isnan(psi) & np.signbit(psi)) and np.any(np.isnan(psi) & ~np.signbit(psi)), case.name
        for name, switches in cases.SIGN_VARIANTS.items():
            if not np.array_equal(cases.extract_signs(psi, **switches), right):
                told[name].append(case.name)
    print("\n".join("%s: %s" % item for item in told.items()))
    assert all(told.values()), told
