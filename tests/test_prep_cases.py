"""The table of tests/prep_cases.py still does what it is there for — asserted on the CPU (no GPU,
nothing compiled): the right restatement completes on every case, every named WRONG variant is told
apart from it by at least one named case, the cases that are about the cut neither keep nor drop
nearly everything, and the sizes still cross the boundaries of csrc/sparsify.hip,
csrc/ising_elements.hip, csrc/key_table.hip and the scan of csrc/asp_common.hip that they name.
tests/test_gpu_prep_edges.py then compares the kernels with the same restatements."""
import bisect

import numpy as np

import prep_cases as cases


def _bytes(outputs):
    return tuple(np.ascontiguousarray(o).tobytes() for o in outputs)


def _separating(variants, table, run):
    """{variant: [names of the cases on which it differs from the right answer]}."""
    told = {name: [] for name in variants}
    for case in table:
        right = run(case, {})
        for name, switches in variants.items():
            if run(case, switches) != right:
                told[name].append(case.name)
    return told


def test_case_names_are_unique_and_every_case_states_its_purpose():
    table = cases.SPARSIFY_CASES + cases.ISING_CASES + cases.TABLE_CASES
    assert len({case.name for case in table}) == len(table)
    assert all(case.reaches and all(case.reaches) for case in table)


# -- asp_ising_elements ----------------------------------------------------------------------------
def test_ising_restatement_completes_and_is_consistent_on_every_case():
    for case in cases.ISING_CASES:
        x = case.make()
        index, member, elements, offsets = cases.ising_elements(*x.args)
        k, n = x.keys.shape[0], x.other_keys.shape[0]
        assert index.dtype == np.int64 and member.dtype == bool and elements.dtype == np.float64
        assert offsets.dtype == np.int64 and offsets.shape == (k + 1,) and offsets[-1] == n, case.name
        assert index.shape == member.shape == elements.shape == (n,), case.name
        assert np.all(np.isfinite(elements)), case.name
        if n:
            assert index.min() >= 0 and index.max() <= k - 1, case.name
            # first position with keys[i] >= needle, in Python integers (no numpy comparison at all)
            keys = x.keys.tolist()
            for e in np.random.default_rng(0).integers(0, n, size=min(n, 40)):
                needle = int(x.other_keys[e])
                first = bisect.bisect_left(keys, needle)
                assert index[e] == min(first, k - 1) and member[e] == (keys[index[e]] == needle), case.name


def test_every_wrong_ising_variant_is_told_apart_by_a_named_case():
    def run(case, switches):
        return _bytes(cases.ising_elements(*case.make().args, **switches))

    told = _separating(cases.ISING_VARIANTS, cases.ISING_CASES, run)
    print("\n".join("%s: %s" % item for item in told.items()))
    assert all(told.values()), "variants no case tells apart: %r; told apart: %r" % (
        [name for name, where in told.items() if not where], told)
    # the smallest case with an empty row already tells the row lookup apart
    assert "ising K=2 counts=(0, 5)" in told["empty rows mishandled in the row lookup"]


def test_ising_cases_reach_the_stated_structure():
    sizes = sorted({case.make().keys.shape[0] for case in cases.ISING_CASES})
    assert sizes == [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 70001, cases.SCAN_TOTALS_CHUNK + 713]
    degenerate = [(x.keys.shape[0], x.other_keys.shape[0]) for x in (c.make() for c in cases.ISING_CASES)
                  if x.other_keys.shape[0] == 0]
    assert degenerate == [(0, 0), (1, 0)]
    for case in cases.ISING_CASES:
        x = case.make()
        k, n = x.keys.shape[0], x.other_keys.shape[0]
        assert np.all(x.keys[1:] >= x.keys[:-1]), case.name
        if k < 3:
            continue
        counts = x.other_counts
        assert n % 256 != 0, case.name
        assert counts[0] == 0 and counts[1] == 0 and counts[-1] == 0, case.name      # empty first and last rows
        assert 0.15 < np.mean(counts == 0) < 0.27 and counts.max() >= 700, case.name
        assert np.sum(x.keys[1:] == x.keys[:-1]) == 1, case.name                     # one repeated key
        assert np.any(x.keys >> np.uint64(63)) and not np.all(x.keys >> np.uint64(63)), case.name
        index, member, elements, _ = cases.ising_elements(*x.args)
        needles = x.other_keys
        assert np.any(needles == 0) and np.any(needles == cases.U64_MAX), case.name
        assert np.any(needles < x.keys[0]) and np.any(needles > x.keys[-1]), case.name  # below, above: the clip
        assert np.any(needles == x.keys[0]) and np.any(needles == x.keys[-1]), case.name
        assert np.any(needles == x.keys[k // 2]), case.name                           # the repeated key
        assert 0.3 < member.mean() < 0.7, case.name                                   # present and absent
        assert np.any(x.psi == 0) and np.any(x.psi > 0) and np.any(x.psi < 0), case.name
        nonzero = np.abs(x.psi[x.psi != 0])
        assert nonzero.max() / nonzero.min() > 1e6, case.name                          # many decades
        assert np.any(np.signbit(elements) & (elements == 0)), case.name               # -0.0
        assert np.any(elements > 0) and np.any(elements < 0), case.name
    largest = cases.ISING_CASES[-1].make()
    assert largest.keys.shape[0] > cases.SCAN_TOTALS_CHUNK
    assert 0.75 < largest.other_keys.shape[0] / largest.keys.shape[0] < 1.25   # about one per row


# -- asp_table_index -------------------------------------------------------------------------------
def test_table_restatement_completes_and_is_consistent_on_every_case():
    for case in cases.TABLE_CASES:
        x = case.make()
        position = {int(key): i for i, key in enumerate(x.keys)}
        for queries in x.queries:
            out = cases.table_index(x.keys, queries)
            assert out.dtype == np.int64 and out.shape == queries.shape
            assert out.tolist() == [position.get(int(q), -1) for q in queries], case.name


def test_every_wrong_table_variant_is_told_apart_by_a_named_case():
    def run(case, switches):
        x = case.make()
        return _bytes(cases.table_index(x.keys, q, **switches) for q in x.queries)

    told = _separating(cases.TABLE_VARIANTS, cases.TABLE_CASES, run)
    print("\n".join("%s: %s" % item for item in told.items()))
    assert all(told.values()), "variants no case tells apart: %r; told apart: %r" % (
        [name for name, where in told.items() if not where], told)


def test_table_cases_reach_the_stated_structure():
    assert [case.make().keys.shape[0] for case in cases.TABLE_CASES] == [0, 1, 2, 3, 1000, 300_000]
    singles = set()
    for case in cases.TABLE_CASES:
        x = case.make()
        n = x.keys.shape[0]
        assert [q.shape[0] for q in x.queries] == [1, 255, 256, 257]
        assert np.all(x.keys[1:] > x.keys[:-1]), case.name
        if n >= 1000:
            assert 0.4 < np.mean(x.keys >> np.uint64(63)) < 0.6, case.name    # bit 63 in about half
        for queries in x.queries[1:]:
            assert np.any(queries == 0) and np.any(queries == cases.U64_MAX), case.name
            if n:
                assert np.any(queries < x.keys[0]) and np.any(queries > x.keys[-1]), case.name
                assert np.any(queries == x.keys[0]) and np.any(queries == x.keys[-1]), case.name
                out = cases.table_index(x.keys, queries)
                assert np.any(out < 0) and np.any(out >= 0), case.name
                between = (queries > x.keys[0]) & (queries < x.keys[-1]) & (out < 0)
                assert n < 2 or np.any(between), case.name
        singles.add((n, int(x.queries[0][0])))
    assert len({q for _, q in singles}) >= 5       # the single query of m = 1 is another probe each time
    assert any(np.any(case.make().keys >> np.uint64(63)) for case in cases.TABLE_CASES[1:4])


# -- asp_sparsify_component ------------------------------------------------------------------------
def _runs():
    return [(case, reltol) for case in cases.SPARSIFY_CASES for reltol in case.make().reltols]


def test_sparsify_oracle_completes_and_the_restatements_agree_with_it():
    """oracle.sparsify_component raises nowhere; `sparsify_keep` (whose switches are the wrong
    variants) and `block_of` restate it: same mask, same block, stored zeros included."""
    for case, reltol in _runs():
        x = case.make()
        m = x.matrix
        assert m.has_canonical_format and m.shape[0] == x.frozen.shape[0], case.name
        assert x.frozen[x.anchor], case.name
        keep, block = cases.sparsify_oracle(case, reltol)
        assert keep[x.anchor] and np.all(keep[x.frozen]), case.name
        mine = cases.sparsify_keep(m, x.frozen, reltol, x.anchor)
        assert np.array_equal(mine, keep), (case.name, reltol)
        indptr, indices, data = cases.block_of(m, keep)
        assert np.array_equal(block.indptr, indptr) and np.array_equal(block.indices, indices), (case.name, reltol)
        assert block.data.tobytes() == data.tobytes(), (case.name, reltol)


def test_every_wrong_sparsify_variant_is_told_apart_by_a_named_case():
    told = {name: [] for name in cases.SPARSIFY_VARIANTS}
    for case, reltol in _runs():
        x = case.make()
        keep, _ = cases.sparsify_oracle(case, reltol)
        for name, switches in cases.SPARSIFY_VARIANTS.items():
            try:
                wrong = cases.sparsify_keep(x.matrix, x.frozen, reltol, x.anchor, **switches)
            except AssertionError:
                told[name].append("%s at reltol %g (raises)" % (case.name, reltol))
                continue
            if wrong.tobytes() != keep.tobytes():
                told[name].append("%s at reltol %g (%d spins differ)" % (case.name, reltol,
                                                                         int(np.sum(wrong != keep))))
    print("\n".join("%s: %s" % item for item in told.items()))
    assert all(told.values()), "variants no case tells apart: %r; told apart: %r" % (
        [name for name, where in told.items() if not where], told)
    # each variant by the case written for it
    assert any(w.startswith("frozen bridges") for w in told["two frozen ends are pruned like any others"])
    assert any(w.startswith("directed pairs") for w in told["a link whenever either direction survives"])
    assert any(w.startswith("directed pairs") for w in told["<= in the cutoff"])


def test_cases_about_the_cut_keep_between_a_tenth_and_nine_tenths():
    shares = {}
    for case in cases.SPARSIFY_CASES:
        x = case.make()
        for reltol in x.cutting:
            assert reltol in x.reltols
            keep, _ = cases.sparsify_oracle(case, reltol)
            shares[case.name, reltol] = float(keep.mean())
    print(shares)
    assert {name for name, _ in shares} == {"frozen bridges", "directed pairs", "large"}
    assert all(0.1 <= share <= 0.9 for share in shares.values()), shares


def test_sparsify_cases_reach_the_stated_structure():
    by_name = {case.name: case for case in cases.SPARSIFY_CASES}
    # frozen bridges: weak couplings between two frozen spins and between a frozen and a free one
    x = by_name["frozen bridges"].make()
    coo = x.matrix.tocoo()
    weak = np.abs(coo.data) < 1e-3 * np.abs(coo.data).max()
    both = x.frozen[coo.row] & x.frozen[coo.col]
    one = x.frozen[coo.row] ^ x.frozen[coo.col]
    keep, _ = cases.sparsify_oracle(by_name["frozen bridges"], 1e-3)
    assert np.sum(weak & both) == 10 and np.sum(weak & one) == 2 and x.frozen.sum() == 6
    assert np.all(keep[coo.row[weak & both]] & keep[coo.col[weak & both]])
    assert not np.any(keep[coo.row[weak & one]] & keep[coo.col[weak & one]])
    # directed pairs: the five kinds, the maximum on the diagonal, stored zeros, a -0.0
    x = by_name["directed pairs"].make()
    m = x.matrix
    assert m.shape[0] >= 400 and x.reltols == (0.0, 1e-3, 0.5)
    largest = np.abs(m.data).max()
    assert np.abs(m.diagonal()).max() == largest and np.sum(np.abs(m.data) == largest) == 1
    assert np.sum(m.data == 0) > 100 and np.sum(np.signbit(m.data) & (m.data == 0)) == 1
    dense = m.toarray()
    i, j = np.nonzero(np.triu(dense != 0, 1) | np.triu(dense.T != 0, 1))
    a, b = dense[i, j], dense[j, i]
    assert np.sum((a == -b)) >= 70                                   # (v, -v) and (weak, -weak)
    assert np.sum((a == -b) & (np.abs(a) < 1e-4)) >= 35              # ... of which weak
    assert np.sum((a == 0) ^ (b == 0)) >= 50                         # one direction absent
    for reltol in (1e-3, 0.5):
        assert np.sum(np.abs(m.data) == reltol * largest) >= 15      # exactly on the threshold
    # hub rows
    x = by_name["hub rows"].make()
    lengths = np.diff(x.matrix.indptr)
    hubs = sorted(lengths[lengths > 3].tolist())
    assert hubs == [63, 64, 65, 127, 128, 129, 300] == list(cases.HUB_DEGREES)
    assert np.sum(lengths > 128) == 2 and np.all(lengths >= 1)
    keep, block = cases.sparsify_oracle(by_name["hub rows"], 1e-3)
    for row in np.nonzero(lengths > 3)[0]:
        cols = x.matrix.indices[x.matrix.indptr[row]:x.matrix.indptr[row + 1]]
        per_chunk = [int(keep[cols[s:s + 64]].sum()) for s in range(0, cols.shape[0], 64)]
        full = per_chunk[:cols.shape[0] // 64]
        assert keep[row] and all(0 < c < 64 for c in full) and sum(per_chunk) > 0, per_chunk
        assert any(c < min(64, cols.shape[0] - 64 * t) for t, c in enumerate(per_chunk))   # kept and cut interleave
        assert len(full) < 2 or len(set(full)) > 1, per_chunk               # the chunks emit different counts
    assert np.diff(block.indptr).max() > 128                         # ... and a kept row beyond two chunks
    # tile edges
    assert [by_name["tile edge K=%d" % k].make().matrix.shape[0] for k in (1, 2, 2047, 2048, 2049, 4097)] == \
        [1, 2, 2047, 2048, 2049, 4097]
    keep, _ = cases.sparsify_oracle(by_name["tile edge K=4097"], 1e-3)
    assert keep.sum() > cases.SCAN_TILE and keep[-1] and not keep[2]
    # large
    x = by_name["large"].make()
    k, nnz = x.matrix.shape[0], x.matrix.nnz
    assert k > cases.SCAN_TOTALS_CHUNK and nnz > cases.ABS_MAX_STRIDE == 2 ** 20
    where = np.nonzero(np.abs(x.matrix.data) == np.abs(x.matrix.data).max())[0]
    assert where.tolist() == [nnz - 4] and where[0] >= cases.ABS_MAX_STRIDE
    assert np.diff(x.matrix.indptr).max() < 64                       # hub-free
    keep, block = cases.sparsify_oracle(by_name["large"], 0.0)
    assert keep.sum() > cases.SCAN_TOTALS_CHUNK and block.nnz > cases.ABS_MAX_STRIDE
    cut, _ = cases.sparsify_oracle(by_name["large"], 1e-2)
    assert 0.1 * k <= cut.sum() <= 0.9 * k
