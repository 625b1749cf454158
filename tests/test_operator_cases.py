"""The table of tests/operator_cases.py still does what it is there for — asserted on the CPU (no
GPU, nothing compiled besides the oracle): the numpy restatements of the action, the coupling build
and the extension equal `Operator.batched_apply`, `helpers.reference_route_ising`, `np.unique` and the
oracle bit for bit on every case; every named WRONG variant is told apart from the right answer by
at least one named case; and the structure the cases name is really in their inputs — home slots
and fingerprints, the wrapped chain, bond counts, row widths, connection counts, rows beyond
`max_connections`, cancelled and reverse-only entries.  tests/test_gpu_operator_edges.py then
compares the kernels of csrc/operator_apply.hip with the same laws on the same cases."""
import numpy as np

import oracle
from helpers import reference_route_ising

import operator_cases as cases


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _details(name, **switches):
    x = cases.BY_NAME[name].make()
    return cases.ising(x.table, x.keys, x.psi, details=True, **switches)[3]


def _widths(name):
    e = cases.expected(name)
    return np.diff(e.indptr)


def test_case_names_are_unique_and_every_case_states_its_purpose():
    assert len(cases.BY_NAME) == len(cases.CASES) >= 40
    assert all(case.reaches and all(case.reaches) for case in cases.CASES)
    assert set(cases.END_TO_END) | set(cases.RAW) <= set(cases.BY_NAME)


def test_the_constants_are_the_kernels():
    """mix64 is the splitmix64 finaliser (its published first output for seed 0 is mix64 of the
    golden-ratio increment), unmix64 its inverse, and the table has max(1024, pow2 >= 2 K) slots."""
    assert cases.mix64(0) == 0 and cases.unmix64(0) == 0
    assert cases.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    rng = np.random.default_rng(1)
    for x in [1, 2, cases.MASK64, 1 << 63] + rng.integers(0, 1 << 63, size=200).tolist():
        assert cases.unmix64(cases.mix64(x)) == x and cases.mix64(cases.unmix64(x)) == x
    assert [cases.slot_count(k) for k in (0, 1, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 2048, 2048, 4096]
    key = cases.key_with(0xDEADBEEF, 12345, 1023)
    assert cases.fingerprint(key) == 0xDEADBEEF and cases.home(key, 6) == 1023
    # the package's own mix64 (numpy, tests/build_cases.py) is the same function
    import build_cases

    assert int(build_cases.mix64(key)[0]) == cases.mix64(key)


def test_the_restatements_equal_the_host_laws_on_every_case():
    """`action` is Operator.batched_apply, `ising` is the reference route (numpy + scipy), `extend`
    is np.unique of the targets."""
    for case in cases.CASES:
        x, e = case.make(), cases.expected(case.name)
        assert not any(np.isnan(a).any() or np.isinf(a).any() for a in (x.psi, x.table[2])), case.name
        other, coeffs, counts = x.operator.batched_apply(x.keys)
        assert not np.any(coeffs.imag)
        assert _same(other[:, 0], e.other) and _same(coeffs.real, e.coeffs) and _same(counts, e.counts), case.name
        ref = reference_route_ising(x.operator, x.keys, x.psi)
        assert np.array_equal(ref.row, e.row) and np.array_equal(ref.col, e.col) and _same(ref.data, e.val), case.name
        assert np.all(np.isfinite(e.val)) and np.all(np.isfinite(e.coeffs)), case.name
        targets = x.operator.batched_apply(x.extend_keys)[0][:, 0]
        assert _same(np.unique(targets), e.extension), case.name
        assert e.indptr[-1] == e.val.shape[0] and e.indptr.shape[0] == x.keys.shape[0] + 1


def test_the_restatements_equal_the_oracle_on_every_case():
    for case in cases.CASES:
        x, e = case.make(), cases.expected(case.name)
        other, coeffs, counts = oracle.operator_apply(x.table, x.keys)
        assert _same(other, e.other) and _same(coeffs, e.coeffs) and _same(counts, e.counts), case.name
        row, col, val = oracle.operator_ising(x.table, x.keys, x.psi)
        assert _same(row, e.row) and _same(col, e.col) and _same(val, e.val), case.name
        assert _same(oracle.operator_extend(x.table, x.extend_keys), e.extension), case.name


def test_the_walk_of_the_hash_table_is_the_search():
    """`probe` on `hash_slots` (no switch) finds what np.searchsorted finds, on every needle of the
    hash cases and of a case with 513 keys."""
    for name in [c.name for c in cases.CASES if c.name.startswith("hash")] + ["rows K=257"]:
        x, e = cases.BY_NAME[name].make(), cases.expected(name)
        slots, listed = cases.hash_slots(x.keys), x.keys.tolist()
        assert sum(1 for s in slots if s) == x.keys.shape[0] and len(slots) == cases.slot_count(x.keys.shape[0])
        needles = np.unique(e.other)
        walked = [cases.probe(slots, listed, t)[0] for t in needles.tolist()]
        assert walked == cases.find(x.keys, needles).tolist(), name


# -- every case reaches what it names -----------------------------------------------------------------
def test_hash_cases_have_the_chains_they_name():
    x = cases.BY_NAME["hash: three keys at home in the last slot"].make()
    crowded = x.marks["crowded"]
    assert all(k ^ 2 in x.keys.tolist() for k in crowded)         # the partners whose rows probe them
    assert [cases.home(k, 6) for k in crowded] == [cases.LAST_SLOT] * 3
    slots, listed = cases.hash_slots(x.keys), x.keys.tolist()
    assert [at for at, s in enumerate(slots) if s and at in (1023, 0, 1)] == [0, 1, 1023] and slots[2] == 0
    reads = sorted(len(cases.probe(slots, listed, k)[1]) for k in crowded)
    assert reads == [1, 2, 3]                                   # one at home, two past the end
    targets = set(cases.expected("hash: three keys at home in the last slot").other.tolist())
    assert set(crowded) <= targets                              # ... and rows Yi do probe them
    assert all(cases.probe(slots, listed, k, chain_stops_at_end=True)[0] == -1 for k in crowded
               if len(cases.probe(slots, listed, k)[1]) > 1)

    x = cases.BY_NAME["hash: one fingerprint, two keys"].make()
    k1, t, k2 = x.marks["k1"], x.marks["t"], x.marks["k2"]
    assert k1 != t and cases.fingerprint(k1) == cases.fingerprint(t) and cases.home(k1, 4) == cases.home(t, 4)
    listed = x.keys.tolist()
    assert k1 in listed and k2 in listed and t not in listed
    slots = cases.hash_slots(x.keys)
    index, read = cases.probe(slots, listed, t)
    assert index == -1 and len(read) == 2                       # k1's slot (fingerprint equal), then an empty one
    assert cases.probe(slots, listed, t, fingerprint_trusted=True)[0] == listed.index(k1)
    e = cases.expected("hash: one fingerprint, two keys")
    row_k2 = slice(int(np.cumsum(e.counts)[listed.index(k2)] - e.counts[listed.index(k2)]),
                   int(np.cumsum(e.counts)[listed.index(k2)]))
    assert t in e.other[row_k2].tolist()
    assert x.psi[listed.index(k1)] != 0 and x.psi[listed.index(k2)] != 0

    for name, present in (("hash: key 0 present", True), ("hash: key 0 absent but probed", False)):
        x, e = cases.BY_NAME[name].make(), cases.expected(name)
        assert (0 in x.keys.tolist()) == present
        assert int(np.sum(e.other == 0)) >= 3 + int(present)     # rows 1, 2, 3 (and 0 itself) reach key 0
        slots = cases.hash_slots(x.keys)
        assert (slots[0] == 1) == present and (present or slots[0] == 0)
    assert cases.slot_count(512) == 2 * 512 and cases.slot_count(513) == 2048
    assert cases.BY_NAME["hash: K=512"].make().keys.shape[0] == 512
    assert cases.BY_NAME["hash: K=513"].make().keys.shape[0] == 513


def test_bond_counts_diagonal_and_row_widths():
    for b in cases.BOND_COUNTS:
        x = cases.BY_NAME["bonds B=%d" % b].make()
        assert x.num_bonds == b and 12 <= x.number_spins <= 17 and cases.flip_owner(x.table) is not None
        assert cases.expected("bonds B=%d" % b).val.shape[0] > x.keys.shape[0]      # couplings inside the cluster
    x = cases.BY_NAME["diagonal across the chunk boundary"].make()
    assert x.marks["d"][62:66].tolist() == [cases.BIG, 1.0, -cases.BIG, 1.0] and x.num_bonds == 70
    right = cases.action(x.table, x.keys)[1]
    for switch in ("diagonal_per_chunk", "diagonal_tree"):
        wrong = cases.action(x.table, x.keys, **{switch: True})[1]
        starts = np.cumsum(cases.expected("diagonal across the chunk boundary").counts) - cases.expected(
            "diagonal across the chunk boundary").counts
        assert np.all(wrong[starts] != right[starts]), switch   # every row's diagonal shows it
    for name, n, width in (("rows of 82 entries (18 sites)", 18, 82), ("rows of 145 entries (24 sites)", 24, 145)):
        x, widths = cases.BY_NAME[name].make(), _widths(name)
        centre = x.keys.tolist().index(x.marks["centre"])
        assert x.num_bonds == n * (n - 1) // 2 and x.keys.shape[0] == width
        assert widths[centre] == width == widths.max() and np.sum(widths > 1) == width
        assert np.all(np.delete(widths, centre) == n)           # neighbours of the centre are neighbours of each other
    for name, bonds in (("full matrices, 3 bonds, whole space", 3), ("full matrices, 32 bonds, 64 sites", 32)):
        x, e = cases.BY_NAME[name].make(), cases.expected(name)
        assert x.num_bonds == bonds and np.all(e.counts == 1 + 3 * bonds) and cases.flip_owner(x.table) is not None
        ones = np.uint64((1 << x.number_spins) - 1)
        assert ones in e.extension and ones in x.keys
    x = cases.BY_NAME["full matrices, 32 bonds, 64 sites"].make()
    assert np.uint64(cases.MASK64) not in x.extend_keys         # the extension REACHES the all-ones key
    # three kept entries on one lane: a key of the 3-bond case whose three partners through bond 0 are all present
    assert _widths("full matrices, 3 bonds, whole space").max() >= 1 + 3


def test_reverse_only_cancellation_and_minus_zero():
    for sites in (6, 8):
        name = "reverse-only, %d sites" % sites
        x, e = cases.BY_NAME[name].make(), cases.expected(name)
        k, most = x.keys.shape[0], cases.max_connections(x.table)
        assert k == 1 << sites and most == 1 + sites // 2
        assert e.val.shape[0] > k * most                          # the retry loop of DeviceOperator.ising runs
        assert np.diff(e.indptr).max() == 3 * (sites // 2) + 1 > most
        assert 3 * x.num_bonds + 2 > most                         # cap_all is what sizes the LDS
        assert _details(name)["reverse_only"] > 0
    assert _details("cancelling pairs")["cancelled"] > 0
    x, e = cases.BY_NAME["-0.0 matrix elements"].make(), cases.expected("-0.0 matrix elements")
    assert np.signbit(x.table[2][x.table[2] == 0]).any()
    assert not np.any((e.coeffs == 0) & np.signbit(e.coeffs) & (np.arange(e.coeffs.shape[0]) > 0)
                      & ~np.isin(np.arange(e.coeffs.shape[0]), np.cumsum(e.counts) - e.counts))
    assert cases.action(x.table, x.keys, minus_zero_counts=True)[0].shape[0] > e.other.shape[0]


def test_duplicate_target_cases():
    name = "duplicates: star rows of 1, 64, 65, 129"
    x, e = cases.BY_NAME[name].make(), cases.expected(name)
    assert cases.flip_owner(x.table) is None                       # unique_targets is false: the merge route
    listed = x.keys.tolist()
    for width in cases.STAR_WIDTHS:
        rows = [listed.index(x.marks["bases"][width] | low) for low in range(8)]
        assert e.counts[rows].tolist() == [width] * 8
    lonely = listed.index(x.marks["lonely"])
    details = _details(name)
    stored_rows = details["stored"] // x.keys.shape[0]
    assert np.sum(stored_rows == lonely) == 1 and e.counts[lonely] > 1      # only its diagonal is inside
    assert details["has_mirror"].all()
    assert details["pruned"] >= 16 and details["cancelled"] == 0   # the "order" and the "cancel" groups: Mhat itself is 0
    widths = np.diff(e.indptr)
    cancel = listed.index(x.marks["bases"]["cancel"])
    assert e.col[e.indptr[cancel]:e.indptr[cancel + 1]].tolist() == [cancel, cancel + 1, cancel + 4]   # + 2 pruned
    assert cases.max_connections(x.table) == 131 and widths.max() <= 4

    name = "duplicates: merged row of 65 columns"
    x, e = cases.BY_NAME[name].make(), cases.expected(name)
    centre = x.keys.tolist().index(x.marks["centre"])
    assert cases.flip_owner(x.table) is None and _details(name)["has_mirror"].all()
    assert np.diff(e.indptr)[centre] == 65 and e.counts[centre] == 85

    name = "duplicates: one one-directional element"
    x = cases.BY_NAME[name].make()
    details = _details(name)
    assert cases.flip_owner(x.table) is None and not details["has_mirror"].all()
    assert x.refusal == (-3, "no mirror")


def test_sizes_and_extension_inputs():
    for k in cases.ROW_COUNTS:
        x = cases.BY_NAME["rows K=%d" % k].make()
        assert x.keys.shape[0] == k and x.num_bonds == 32
    totals = {}
    for case in cases.CASES:
        totals.setdefault(int(cases.expected(case.name).counts.sum()), case.name)
    for n in (255, 256, 257, 2047, 2048, 2049):
        assert n in totals, n
    assert totals[256] and cases.expected("one full bond, N=2048").counts.sum() == cases.SCAN_TILE
    for n in cases.CONNECTION_COUNTS:
        x = cases.BY_NAME["no bonds, N=n=%d" % n].make()
        assert x.num_bonds == 0 and x.keys.shape[0] == n and not np.array_equal(x.extend_keys, x.keys)
    x = cases.BY_NAME["extension: unsorted input with repeats"].make()
    assert np.unique(x.extend_keys).shape[0] == 300 and x.extend_keys.shape[0] == 360
    assert np.any(np.diff(x.extend_keys.astype(np.float64)) < 0)
    assert cases.BY_NAME["extension: 2 sites"].make().extend_keys.tolist() == [3, 0, 3, 1]
    x = cases.BY_NAME["extension: 33 sites"].make()
    high = x.keys >> np.uint64(32)
    assert x.number_spins == 33 and 0 < high.sum() < x.keys.shape[0]
    assert np.any(np.diff(x.extend_keys.astype(np.float64)) < 0)
    e = cases.expected("full matrices, 32 bonds, 64 sites")
    assert np.any(e.extension >> np.uint64(63) == 1) and np.any(e.extension >> np.uint64(63) == 0)


def test_the_largest_model_is_beyond_the_lds_limit():
    x = cases.BY_NAME["2016 bonds, 64 sites"].make()
    assert x.num_bonds == 2016 == 64 * 63 // 2 and x.number_spins == 64
    capacity = (3 * x.num_bonds + 2 + 1) & ~1
    assert 4 * capacity * 12 > cases.LDS_BYTES and x.refusal == (-4, "bytes of LDS")
    # the limit lies between 1136 and 1137 bonds; all-to-all on 48 sites fits, on 49 it does not
    assert 4 * ((3 * 1136 + 3) & ~1) * 12 <= cases.LDS_BYTES < 4 * ((3 * 1137 + 3) & ~1) * 12
    assert 48 * 47 // 2 <= 1136 < 49 * 48 // 2


# -- the wrong variants --------------------------------------------------------------------------------
def _told_apart(variants, compute, right):
    told = {name: [] for name in variants}
    for case in cases.CASES:
        x = case.make()
        for name, switches in variants.items():
            if not all(_same(a, b) for a, b in zip(compute(x, **switches), right(case.name))):
                told[name].append(case.name)
    return told


def test_every_wrong_variant_is_told_apart_by_a_named_case():
    action = _told_apart(cases.ACTION_VARIANTS, lambda x, **s: cases.action(x.table, x.keys, **s),
                         lambda n: (cases.expected(n).other, cases.expected(n).coeffs, cases.expected(n).counts))
    ising = _told_apart(cases.ISING_VARIANTS, lambda x, **s: cases.ising(x.table, x.keys, x.psi, **s),
                        lambda n: (cases.expected(n).row, cases.expected(n).col, cases.expected(n).val))
    extend = _told_apart(cases.EXTEND_VARIANTS,
                         lambda x, **s: (cases.extend(x.table, x.extend_keys, x.number_spins, **s),),
                         lambda n: (cases.expected(n).extension,))
    for what, told in (("action", action), ("ising", ising), ("extend", extend)):
        print("\n".join("%s | %s: %s" % (what, name, found) for name, found in told.items()))
        assert all(told.values()), "%s variants no case tells apart: %r" % (what, [n for n, w in told.items() if not w])
    # ... each by the case written for it
    assert "diagonal across the chunk boundary" in action["diagonal summed per chunk of 64 bonds"]
    assert "diagonal across the chunk boundary" in action["diagonal summed as a tree"]
    assert "diagonal across the chunk boundary" in ising["diagonal summed per chunk of 64 bonds"]
    assert "-0.0 matrix elements" in action["-0.0 counted as an element"]
    assert "-0.0 matrix elements" in extend["-0.0 counted as an element"]
    assert "hash: one fingerprint, two keys" in ising["fingerprint trusted"]
    assert "hash: three keys at home in the last slot" in ising["chain stops at the table's end"]
    assert "hash: key 0 present" in ising["key 0 treated as empty"]
    assert "hash: key 0 absent but probed" in ising["an absent needle 0 found at index 0"]
    assert "cancelling pairs" in ising["cancelled pairs kept"]
    assert "duplicates: star rows of 1, 64, 65, 129" in ising["cancelled pairs kept"]
    assert {"reverse-only, 6 sites", "reverse-only, 8 sites"} <= set(ising["reverse-only entries dropped"])
    assert "rows of 82 entries (18 sites)" in ising["rows sorted only within the first 64 entries"]
    assert "rows of 145 entries (24 sites)" in ising["rows sorted only within the first 64 entries"]
    assert "duplicates: star rows of 1, 64, 65, 129" in ising["duplicates summed in another order"]
    assert "rows K=257" in ising["zero diagonal kept"] and "rows K=257" in ising["coeff * (psi_j * psi_r)"]
    for name in ("full matrices, 3 bonds, whole space", "full matrices, 32 bonds, 64 sites"):
        assert name in extend["all-ones target dropped"]
    assert "extension: unsorted input with repeats" in extend["duplicates unique-d without sorting"]
    # ... and the hash variants change nothing where the table holds no such chain
    assert "rows K=5" not in ising["fingerprint trusted"] and "rows K=5" not in ising["chain stops at the table's end"]
