"""CPU: the restatements of tests/lanczos_cases.py and the conditions its cases must meet for
tests/test_gpu_sector_product.py and tests/test_gpu_lanczos.py to mean something: the product law against
numpy where numpy is exact and against a direct evaluation in fractions, each wrong reading of the law
told apart by the case named for it, the sizes and slot patterns of the product table, the spectra of the
Lanczos matrices, and the convergence of the restated drivers on every case meant to converge."""
import math
from fractions import Fraction

import numpy as np
import pytest

import lanczos_cases as cases
from lanczos_cases import LANCZOS_CASES, PRODUCT_CASES

RANDOM = ["n%d_w%d" % (n, w) for n in cases.PRODUCT_SIZES for w in cases.PRODUCT_WIDTHS]


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------
# the product law
# ---------------------------------------------------------------------------------------------------

def test_the_law_equals_numpy_where_every_step_is_exact():
    """Small integers: every product and partial sum is a double, so any order and any fusing agree."""
    rng = np.random.default_rng(8)
    for n, width in ((1, 0), (1, 3), (5, 0), (37, 4), (70, 9)):
        idx = rng.integers(0, n, size=(width, n)).astype(np.uint32)
        val = rng.integers(-64, 65, size=(width, n)).astype(np.float64)
        diag = rng.integers(-64, 65, size=n).astype(np.float64)
        x = rng.integers(-64, 65, size=n).astype(np.float64)
        want = diag * x
        for k in range(width):
            want = want + val[k] * x[idx[k]]
        assert np.array_equal(cases.ell_product_law(idx, val, diag, x), want)
        for variant in ("unfused", "slots_reversed", "diagonal_last", "pairwise"):
            assert np.array_equal(cases.ell_product_law(idx, val, diag, x, variant=variant), want), variant


def test_the_law_equals_a_direct_evaluation_of_a_three_term_row():
    d, x0, v0, x1, v1, x2 = 0.1, 0.7, 1.0 / 3.0, -0.9, 2.0 ** 0.5, 1e-3
    idx = np.array([[1, 0, 0], [2, 0, 0]], dtype=np.uint32)
    val = np.array([[v0, 0.0, 0.0], [v1, 0.0, 0.0]])
    got = cases.ell_product_law(idx, val, np.array([d, 0.0, 0.0]), np.array([x0, x1, x2]))
    first = d * x0                                                    # one rounding
    second = float(Fraction(v0) * Fraction(x1) + Fraction(first))     # one rounding
    third = float(Fraction(v1) * Fraction(x2) + Fraction(second))     # one rounding
    assert got[0] == third and got[1] == 0 and got[2] == 0
    assert third != (first + v0 * x1) + v1 * x2 or third != first + (v0 * x1 + v1 * x2)


def test_fused_zeros_are_signed_as_the_hardware_signs_them():
    fma = cases._fma
    for v, x, acc, want in ((0.0, 1.0, -0.0, 0.0), (-0.0, 1.0, -0.0, -0.0), (0.0, -1.0, 0.0, 0.0),
                            (1.0, 1.0, -1.0, 0.0), (-1.0, 1.0, 1.0, 0.0), (-0.0, -0.0, -0.0, 0.0),
                            (1e-200, -1e-200, 0.0, -0.0), (1e-200, -1e-200, -0.0, -0.0),
                            (5e-324, 0.5, 0.0, 0.0), (5e-324, 0.75, 0.0, 5e-324), (3.0, 0.5, -0.0, 1.5)):
        assert _bits(fma(v, x, acc)) == _bits(want), (v, x, acc)
    assert _bits(cases.product_law("signed_zeros")) == _bits([-0.0, 0.0, -0.0, 0.0, 0.0, 0.0])
    y = cases.product_law("subnormal")
    tiny = np.finfo(np.float64).tiny
    assert 0 < y[0] < tiny and y[1] == 2e-160 and -tiny < y[2] < 0


@pytest.mark.parametrize("variant,name", cases.TOLD_APART, ids=["%s-%s" % pair for pair in cases.TOLD_APART])
def test_named_case_tells_the_wrong_reading_apart(variant, name):
    wrong = cases.ell_product_law(*PRODUCT_CASES[name], variant=variant)
    assert _bits(wrong) != _bits(cases.product_law(name))


def test_every_wrong_reading_has_a_named_case_and_the_values_the_names_claim():
    assert {v for v, _ in cases.TOLD_APART} == set(cases.VARIANTS)
    assert cases.product_law("cancel")[0] == -2.0 ** -60 and cases.product_law("cancel")[2] == 2.0 ** -60
    assert cases.ell_product_law(*PRODUCT_CASES["cancel"], variant="unfused")[0] == 0
    assert cases.product_law("order").tolist() == [0.0, 0.0, 9.0]
    assert cases.ell_product_law(*PRODUCT_CASES["order"], variant="slots_reversed").tolist() == [1.0, 0.0, 7.0]
    assert cases.ell_product_law(*PRODUCT_CASES["order"], variant="diagonal_last").tolist() == [0.0, 1.0, 9.0]
    assert cases.ell_product_law(*PRODUCT_CASES["order"], variant="pairwise").tolist() == [0.0, 0.0, 8.0]


@pytest.mark.parametrize("name", ["n65_w7", "n257_w7", "n4097_w7", "n64_w2", "dense300"])
def test_random_cases_tell_every_wrong_reading_apart_too(name):
    right = _bits(cases.product_law(name))
    for variant in cases.VARIANTS:
        assert _bits(cases.ell_product_law(*PRODUCT_CASES[name], variant=variant)) != right, variant


def test_the_product_table_reaches_every_size_and_width():
    shapes = {name: PRODUCT_CASES[name][0].shape for name in PRODUCT_CASES}
    assert {(n, w) for w, n in shapes.values()} >= {(n, w) for n in (1, 2, 63, 64, 65, 255, 256, 257, 513, 4097)
                                                   for w in (0, 1, 2, 7)}
    assert shapes["dense300"] == (299, 300)
    for name in PRODUCT_CASES:
        idx, val, diag, x = PRODUCT_CASES[name]
        width, n = idx.shape
        assert idx.dtype == np.uint32 and val.dtype == diag.dtype == x.dtype == np.float64
        assert val.shape == (width, n) and diag.shape == x.shape == (n,)
        assert idx.flags.c_contiguous and val.flags.c_contiguous
        assert n >= 1 and (width == 0 or idx.max() < n)
        assert all(np.all(np.isfinite(a)) for a in (val, diag, x))
        assert np.all(np.isfinite(cases.product_law(name)))


@pytest.mark.parametrize("name", [n for n in RANDOM if n.endswith("_w7")] + ["n65_w2", "n4097_w2"])
def test_slot_patterns_of_the_random_cases(name):
    idx, val, diag, x = PRODUCT_CASES[name]
    width, n = idx.shape
    own = np.arange(n, dtype=np.uint32)
    assert np.all(np.any(idx == 0, axis=0)) and np.all(np.any(idx == n - 1, axis=0))  # from every row
    if width < 7:
        return
    padding = (idx == own[None, :]) & (val == 0) & ~np.signbit(val)
    assert np.all(padding.any(axis=0))
    if n > 2:
        used_after = np.flip(np.cumsum(np.flip(~padding, axis=0), axis=0), axis=0) - ~padding > 0
        used_before = np.cumsum(~padding, axis=0) - ~padding > 0
        assert np.count_nonzero((padding & used_after & used_before).any(axis=0)) > n // 2   # in the middle
        assert np.any(padding[width - 1])                                                    # and at the tail
        assert np.any((idx == own[None, :]) & (val != 0))                                    # a self-index with a value
        # the same column twice, both slots with a value
        twice = 0
        for i in range(n):
            held = idx[val[:, i] != 0, i]
            twice += np.unique(held).shape[0] < held.shape[0]
        assert twice > n // 2
        # not the transpose of anything: some entry (i, j) has no slot (j, i) at all
        pairs = {(i, int(j)) for i in range(n) for j in idx[:, i]}
        assert any((j, i) not in pairs for i, j in pairs)
    if n >= 63:
        for a in (val,) + ((diag, x) if n >= 255 else ()):
            zero = a == 0
            assert np.any(zero & np.signbit(a)) and np.any(zero & ~np.signbit(a))
        tiny = np.finfo(np.float64).tiny
        assert np.any((val != 0) & (np.abs(val) < tiny)) and (n < 255 or np.any((x != 0) & (np.abs(x) < tiny)))


def test_width_zero_cases_produce_zeros_of_both_signs():
    y = np.concatenate([cases.product_law("n%d_w0" % n) for n in (255, 256, 257, 513, 4097)])
    zero = y == 0
    assert np.any(zero & np.signbit(y)) and np.any(zero & ~np.signbit(y)) and np.any(~zero)
    for n in (1, 2, 63):
        idx, val, diag, x = PRODUCT_CASES["n%d_w0" % n]
        assert _bits(cases.product_law("n%d_w0" % n)) == _bits(diag * x)


# ---------------------------------------------------------------------------------------------------
# the matrices for the drivers
# ---------------------------------------------------------------------------------------------------

def test_the_ell_form_of_spectrum_matrix_reassembles_to_its_dense_form():
    for n, seed in ((1, 1), (2, 2), (7, 3), (65, 4)):
        lam = np.random.default_rng(seed).uniform(-3, 3, size=n)
        idx, val, diag, h = cases.spectrum_matrix(n, lam, seed)
        assert idx.shape == val.shape == (n - 1, n) and idx.dtype == np.uint32
        assert np.array_equal(h, h.T)
        assert _bits(cases.ell_to_dense(idx, val, diag)) == _bits(h)
        assert np.allclose(np.linalg.eigvalsh(h), np.sort(lam), rtol=0, atol=1e-13)
        assert all(sorted(idx[:, i].tolist()) == [j for j in range(n) if j != i] for i in range(n))
    for name in ("random300", "three_levels_1_100_99_times_2^30", "zero50", "tiny1", "ladder601_two_pass_cap"):
        idx, val, diag, h = cases.lanczos_matrix(name)
        assert _bits(cases.ell_to_dense(idx, val, diag)) == _bits(h), name
    idx, val, diag, h = cases.lanczos_matrix("banded4097")
    assert idx.shape == (4, 4097) and (idx.astype(np.int64) - np.arange(4097)[None, :]).min() == -2
    dense = cases.ell_to_dense(idx, val, diag)
    assert np.array_equal(dense, h.toarray()) and np.array_equal(dense, dense.T)
    assert np.count_nonzero((idx == np.arange(4097)[None, :]) & (val == 0)) == 6  # padding at the two ends only


def test_the_scaled_case_is_the_unscaled_one_times_a_power_of_two():
    small, large = (cases.lanczos_matrix(name) for name in ("three_levels_1_100_99",
                                                            "three_levels_1_100_99_times_2^30"))
    for a, b in zip(small[1:], large[1:]):
        assert np.array_equal(a * 2.0 ** 30, b)
    assert np.array_equal(small[0], large[0])
    assert LANCZOS_CASES["three_levels_1_100_99_times_2^30"].scale_of == "three_levels_1_100_99"
    # every operation of the recurrence scales exactly, and breakdown is judged relative to the matrix:
    # the restated drivers take the same steps and return the same vector
    for reorthogonalise in (True, False):
        a = cases.lanczos_reference("three_levels_1_100_99")[reorthogonalise]
        b = cases.lanczos_reference("three_levels_1_100_99_times_2^30")[reorthogonalise]
        assert a["iterations"] == b["iterations"] == 3
        assert np.linalg.norm(a["vector"] - b["vector"]) <= 1e-15


@pytest.mark.parametrize("name", list(LANCZOS_CASES))
def test_lanczos_case_has_the_level_structure_its_name_claims(name):
    case, ref = LANCZOS_CASES[name], cases.lanczos_reference(name)
    assert ref["degeneracy"] == case.degeneracy
    assert ref["gap"] >= case.gap_at_least
    p, space = ref["vector"], ref["space"]
    assert abs(np.linalg.norm(p) - 1) < 1e-14 and p[np.argmax(np.abs(p))] > 0
    assert space.shape == (p.shape[0], case.degeneracy) and cases.sine_to_level(space, p) < 1e-14
    h = cases.lanczos_matrix(name)[3]
    assert cases.eigen_residual(h, p) <= 64 * np.finfo(float).eps * max(ref["norm"], 1e-300) * math.sqrt(p.shape[0])
    if case.degeneracy > 1 and not math.isinf(ref["gap"]):
        values = np.linalg.eigvalsh(h)
        assert values[case.degeneracy - 1] - values[0] < 1e-12 * max(1.0, ref["norm"])


def test_the_named_spectra():
    ref = cases.lanczos_reference
    for n in range(1, 8):
        assert abs(ref("tiny%d" % n)["energy"] + 2.5) < 1e-14
    assert ref("zero50")["energy"] == 0 and ref("zero1")["energy"] == 0 and ref("minus3_identity50")["energy"] == -3
    assert abs(ref("three_levels_3_100_97")["energy"] + 4) < 1e-13
    assert abs(ref("three_levels_1_100_99_times_2^30")["energy"] + 2.0 ** 32) < 1e-4
    assert ref("diagonal_30_fold")["energy"] == -5 and ref("diagonal_30_fold")["gap"] == 1
    assert abs(ref("random300_second_at_1e-6")["gap"] - 1e-6) < 1e-12
    assert ref("random300_plus_100")["energy"] > 60
    assert abs(ref("random300_plus_100")["energy"] - 100 - ref("random300")["energy"]) < 1e-12
    assert abs(ref("cluster500_outliers")["norm"] - 50) < 1e-12
    assert abs(ref("ladder601_two_pass_cap")["gap"] - 1e-4) < 1e-12


CONVERGING = [(name, d) for name, case in LANCZOS_CASES.items() if case.converges for d in case.drivers]


@pytest.mark.parametrize("name,reorthogonalise", CONVERGING,
                         ids=["%s-%s" % (n, "full" if d else "two_pass") for n, d in CONVERGING])
def test_the_restated_driver_converges(name, reorthogonalise):
    """The condition that keeps the GPU test from hiding a failure behind "unconverged": the reference
    recurrence alone converges on these inputs, within the budget and within n steps, to the reference."""
    case, ref = LANCZOS_CASES[name], cases.lanczos_reference(name)
    law = ref[reorthogonalise]
    n = ref["vector"].shape[0]
    assert law["iterations"] <= min(case.max_iterations, n)
    scale = max(1.0, abs(ref["energy"]))
    assert law["ritz_residual"] < case.tol * scale or law["iterations"] == n <= 7 or law["ritz_residual"] < 1e-13 * scale
    assert abs(law["energy"] - ref["energy"]) <= 1e-9 * scale
    if case.max_steps:
        assert law["iterations"] <= case.max_steps[0 if reorthogonalise else 1]
    if case.exact_steps:
        assert law["iterations"] == case.exact_steps
    gap = ref["gap"]
    h = cases.lanczos_matrix(name)[3]
    r = cases.eigen_residual(h, law["vector"])
    eps = np.finfo(float).eps
    assert cases.sine_to_level(ref["space"], law["vector"]) <= 2 * r / gap + 64 * eps
    assert law["distance"] <= 1e-6
    assert abs(law["residual"] - r) <= 1e-12 * ref["norm"] + 0.5 * r


def test_the_restated_drivers_report_an_exhausted_budget():
    for name in ("random300_budget20", "ladder601_two_pass_cap"):
        case, ref = LANCZOS_CASES[name], cases.lanczos_reference(name)
        assert not case.converges
        for d in case.drivers:
            law = ref[d]
            assert law["iterations"] == case.exact_steps
            assert law["ritz_residual"] > 1e3 * case.tol * max(1.0, abs(law["energy"]))  # far from the criterion
            assert law["energy"] >= ref["energy"] - 1e-9
            assert law["residual"] >= 0.5 * law["ritz_residual"]
    # ... where full reorthogonalisation would have converged within the same budget
    h = cases.lanczos_matrix("ladder601_two_pass_cap")[3]
    _, _, info = cases.lanczos_law(h, 0, 1e-9, 1000, True)
    assert info["iterations"] < 601 and info["ritz_residual"] < 1e-9


def test_expected_ground_state_follows_the_convention_of_operator_ground_state():
    """On a matrix with a three-fold lowest level the projection does not depend on the basis an
    eigensolver returns for the level, and a start vector inside the level is returned itself."""
    h = cases.lanczos_matrix("random300_three_equal")[3]
    energy, p, degeneracy, gap, space = cases.expected_ground_state(h, seed=5)
    assert degeneracy == 3
    start = np.random.default_rng(5).standard_normal(300)
    rotation = np.linalg.qr(np.random.default_rng(6).standard_normal((3, 3)))[0]
    other = (space @ rotation) @ ((space @ rotation).T @ start)
    other = other / np.linalg.norm(other)
    assert np.linalg.norm(other * np.sign(other[np.argmax(np.abs(other))]) - p) < 1e-14
    assert np.linalg.norm(h @ p - energy * p) < 1e-12
