"""CPU: the two restatements of the sector route's law (tests/sector_bond_cases.py; include/asp.h,
DESIGN.md §3.6) against each other, the wrong readings of the law that the named cases tell apart
through what a handle exposes, the two readings that are symmetries of the law, and the conditions the
cases must meet for tests/test_gpu_sector_bonds.py to mean something."""
import numpy as np
import pytest

import bond_cases
import sector_bond_cases as cases

SUMMARY = ("num_spins", "stored", "bonds", "frustrated", "rows_with_bonds", "strongest_frustrated", "max_abs",
           "min_abs")


def _observables(name, variant=None):
    """What a handle built from the case would show under `variant`: the summary, rows(), the sorted
    magnitudes, the histogram over the edges the GPU test uses (those of the law), and `frustrated` again
    after set_signs(all plus).  Floats as bit patterns, so that == is exact."""
    from annealing_sign_problem_amd.bonds import log_edges

    idx, val, psi = cases.CASES[name]
    row_rule = "tie_largest_col" if variant == "tie_largest_col" else None
    csr = cases.sector_law_rows(idx, val, psi, variant=variant)
    seen = bond_cases.bond_law(*csr, bond_cases.pack(cases.sector_signs(psi, variant=variant)), variant=row_rule)
    out = [seen[field] for field in SUMMARY[:6]] + [np.float64(seen[field]).tobytes() for field in SUMMARY[6:]]
    out += [seen[field].tobytes() for field in ("strongest", "strongest_col", "strongest_frustrated_rows")]
    out.append(bond_cases.magnitudes_law(seen).tobytes())
    right = _bonds(name)
    if right["bonds"]:
        normal, frustrated, below, above = bond_cases.histogram_law(seen, cases.histogram_edges(right, log_edges))
        out += [normal.tobytes(), frustrated.tobytes(), below, above]
    plus = bond_cases.bond_law(*csr, bond_cases.pack(np.ones(psi.shape[0])), variant=row_rule)
    out.append(plus["frustrated"])
    return out


def _bonds(name):
    psi = cases.CASES[name][2]
    return bond_cases.bond_law(*cases.law(name), bond_cases.pack(cases.sector_signs(psi)))


def _row_sets(indptr, indices, data):
    return [sorted(zip(indices[a:b].tolist(), data[a:b].view(np.uint64).tolist()))
            for a, b in zip(indptr[:-1], indptr[1:])]


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_two_laws_agree(name):
    idx, val, psi = cases.CASES[name]
    fast, slow = cases.law(name), cases.sector_law_rows(idx, val, psi)
    assert fast[0].shape == (psi.shape[0] + 1,) and np.array_equal(fast[0], slow[0])
    assert _row_sets(*fast) == _row_sets(*slow)
    for indptr, indices, _ in (fast, slow):  # what the row pass is promised: unique columns, no diagonal
        for i, (a, b) in enumerate(zip(indptr[:-1], indptr[1:])):
            assert len(set(indices[a:b].tolist())) == b - a and i not in indices[a:b]


def test_the_loop_law_stores_in_first_slot_order():
    indptr, indices, _ = cases.sector_law_rows(*cases.CASES["tie"])
    assert indices[indptr[0]:indptr[1]].tolist() == [2, 1]
    indptr, indices, _ = cases.sector_law_rows(*cases.CASES["order"])
    assert indices[indptr[0]:indptr[1]].tolist() == [1, 2, 3] and indices[indptr[3]:indptr[4]].tolist() == [1, 0, 2]
    assert any(np.any(np.diff(indices[a:b]) < 0) for a, b in zip(indptr[:-1], indptr[1:]))


FIRST_SIX = cases.VARIANTS[:6]
_TOLD_APART = ([(v, n) for n in ("n63", "n64", "n65") for v in cases.VARIANTS[:7]]
               + [(v, n) for n in ("n255", "n257", "order") for v in FIRST_SIX]
               + [("cancel_kept", "cancel"), ("symmetric_assumed", "cancel"), ("cancel_kept", "underflow"),
                  ("other_association", "subnormal"), ("tie_largest_col", "tie"),
                  ("symmetric_assumed", "one_sided"), ("symmetric_assumed", "n2")])


@pytest.mark.parametrize("variant,name", _TOLD_APART, ids=["%s-%s" % pair for pair in _TOLD_APART])
def test_named_case_tells_the_wrong_reading_apart(variant, name):
    assert variant not in cases.SYMMETRIES
    assert _observables(name, variant) != _observables(name)


def test_every_wrong_reading_is_told_apart_by_some_case():
    wrong = [v for v in cases.VARIANTS if v not in cases.SYMMETRIES]
    assert wrong == ["first_slot_only", "adjacent_dedupe", "symmetric_assumed", "hji_from_first_slot",
                     "other_association", "sum_then_scale", "diagonal_kept", "cancel_kept", "tie_largest_col"]
    assert {v for v, _ in _TOLD_APART} == set(wrong)


@pytest.mark.parametrize("name", cases.SMALL)
def test_zero_rows_and_the_sign_of_zero_cannot_show(name):
    """Keeping the rows and partners of amplitude 0 changes nothing: all their products are +-0 and are
    dropped.  Nor does `psi > 0` for `psi >= 0`: the two differ at +-0.0 only, states without bonds, and
    the sign of a state without bonds enters no statistic."""
    right = _observables(name)
    for variant in cases.SYMMETRIES:
        assert _observables(name, variant) == right, variant


def test_the_sign_readings_do_differ_where_the_symmetry_says_they_may():
    _, _, psi = cases.CASES["n65"]
    zero = psi == 0
    assert np.any(zero & ~np.signbit(psi)) and np.any(zero & np.signbit(psi))
    differ = cases.sector_signs(psi) != cases.sector_signs(psi, variant="sign_gt")
    assert np.array_equal(differ, zero)  # at both zeros: -0.0 >= 0 holds as well
    assert np.all(cases.sector_signs(psi)[zero] == 1)


def test_the_small_cases_are_what_their_names_say():
    for name in ("n0", "n1", "width0", "all_zero_psi", "cancel", "underflow"):
        assert cases.law(name)[0][-1] == 0, name
    shapes = {name: cases.CASES[name][0].shape for name in cases.CASES}
    assert shapes["n0"] == (0, 0) and shapes["n1"] == (1, 1) and shapes["width0"] == (0, 65)
    assert shapes["wide"] == (70, 130) and shapes["large"] == (5, 20000)
    assert {s[1] for s in shapes.values()} >= {0, 1, 2, 63, 64, 65, 255, 256, 257, 2049}
    idx, val, psi = cases.CASES["n1"]
    assert idx[0, 0] == 0 and val[0, 0] != 0 and psi[0] != 0
    # n2: one pair with Ĥ_01 != Ĥ_10
    idx, val, psi = cases.CASES["n2"]
    indptr, indices, data = cases.law("n2")
    assert indptr.tolist() == [0, 1, 2] and indices.tolist() == [1, 0]
    assert data[0] == data[1] == 0.5 * ((0.75 * 0.8) * 0.6 + (-1.25 * 0.6) * 0.8) < 0
    assert _bonds("n2")["frustrated"] == 2  # (s_0 != s_1 and J < 0: J s_0 s_1 > 0)
    idx, val, psi = cases.CASES["all_zero_psi"]
    assert np.all(psi == 0) and np.any(np.signbit(psi)) and not np.all(np.signbit(psi))
    assert np.count_nonzero(val) > 100
    # cancel and underflow have candidates on both sides, and every product is +-0 or cancels
    idx, val, psi = cases.CASES["cancel"]
    assert (val[0, 0] * abs(psi[1])) * abs(psi[0]) == -((val[0, 1] * abs(psi[0])) * abs(psi[1])) != 0
    idx, val, psi = cases.CASES["underflow"]
    assert np.all(psi != 0) and np.all(val == 1) and (1.0 * abs(psi[0])) * abs(psi[1]) == 0
    indptr, indices, data = cases.law("subnormal")
    assert indptr[-1] == 2 and np.all(data != 0) and np.all(np.abs(data) < np.finfo(float).tiny)
    # order: the sum towards state 1 is 0 in slot order and is not in another
    idx, val, psi = cases.CASES["order"]
    mine = val[idx[:, 0] == 1, 0]
    assert mine.tolist() == [1e16, 1.0, -1e16] and (mine[0] + mine[1]) + mine[2] == 0 != (mine[0] + mine[2]) + mine[1]
    assert np.flatnonzero(idx[:, 0] == 1).tolist() == [0, 2, 4]
    # tie: bit-equal magnitudes, opposite frustration, the larger column in the earlier slot
    idx, val, psi = cases.CASES["tie"]
    assert idx[:, 0].tolist() == [2, 1]
    bonds = _bonds("tie")
    indptr, indices, data = cases.law("tie")
    assert indices[:2].tolist() == [1, 2] and data[0] == data[1] == 0.25
    assert bonds["is_frustrated"][:2].tolist() == [True, False]
    assert bonds["strongest_col"][0] == 1 and bonds["strongest_frustrated_rows"][0]
    # one_sided: no pair is coupled from both rows, and every entry (i, j) lacks its (j, i)
    idx, val, psi = cases.CASES["one_sided"]
    n = psi.shape[0]
    held = {(i, int(j)) for i in range(n) for j in idx[:, i] if j != i}
    assert len(held) > n and not any((j, i) in held for i, j in held)
    indptr, indices, _ = cases.law("one_sided")
    assert {(i, int(j)) for i in range(n) for j in indices[indptr[i]:indptr[i + 1]]} == held


def _non_adjacent_duplicate(column):
    """Does the row reach a target through two slots with another slot between them?"""
    column = column.tolist()
    return any(column[a] == column[b] and b - a > 1 and column[a] not in column[a + 1:b]
               for a in range(len(column)) for b in range(a + 2, len(column)))


@pytest.mark.parametrize("name", cases.RANDOM)
def test_conditions_on_the_random_cases(name):
    idx, val, psi = cases.CASES[name]
    width, n = idx.shape
    assert np.all(idx < n)
    own = np.arange(n, dtype=np.uint32)
    bonds = _bonds(name)
    assert bonds["bonds"] > 0 and bonds["bonds"] == bonds["stored"]
    assert 0.1 < bonds["frustrated"] / bonds["bonds"] < 0.9
    used = idx != own[None, :]
    assert 0.6 < np.count_nonzero(used) / idx.size < 0.8
    assert np.any((val == 0) & ~used & np.roll(used, 1, axis=0) & np.roll(used, -1, axis=0))  # padding inside
    assert any(_non_adjacent_duplicate(np.where(used[:, i], idx[:, i], -1 - np.arange(width)))
               for i in range(n) if psi[i] != 0)
    assert np.any(~used & (val != 0) & (psi != 0)[None, :])  # a diagonal slot with a value
    held = set(zip(*(a.tolist() for a in np.nonzero(used.T))))  # (row, slot)
    pairs = {(i, int(idx[k, i])) for i, k in held}
    lonely = [(i, j) for i, j in pairs if (j, i) not in pairs and psi[i] != 0 and psi[j] != 0]
    if n % 2:
        assert len(lonely) > len(pairs) // 8  # one-sided Ĥ
    elif name != "wide":
        assert not lonely
    zero = psi == 0
    assert 0.05 < np.count_nonzero(zero) / n < 0.3
    assert np.any(np.signbit(psi[zero])) and not np.all(np.signbit(psi[zero]))
    assert np.any(psi[~zero] > 0) and np.any(psi[~zero] < 0)
    if name == "wide":
        duplicates = sum(np.count_nonzero(used[:, i]) - np.unique(idx[used[:, i], i]).shape[0] for i in range(n))
        assert width > 64 and 0.25 < duplicates / np.count_nonzero(used) < 0.45


def test_some_random_case_has_a_one_sided_pair_and_the_large_case_strides():
    assert any(cases.CASES[name][2].shape[0] % 2 for name in cases.RANDOM)
    idx, val, psi = cases.CASES["large"]
    assert psi.shape[0] > 256 * 16 * 4  # more rows than wavefronts in the row pass's largest grid
    assert np.all(idx < psi.shape[0])
    indptr, _, data = cases.law("large")
    assert indptr[-1] > 20000 and np.all(data != 0)
