"""The last two links of the sector route (annealing_sign_problem_amd/sector_ed.py, csrc/sector_basis.hip),
restated without the package and with named inputs that no real operator gives:

* the ELL product ``asp_sector_matvec``: its law is exact (``ell_product_law``: the diagonal product, then
  one fused multiply-add per slot in slot order), ``VARIANTS`` names plausible wrong readings of it and
  ``PRODUCT_CASES`` the synthetic inputs ``(idx u32[width, n], val f64[width, n], diag f64[n], x f64[n])``,
  slot-major as asp_sector_rows writes them (slot k of row i at ``[k, i]``, an unused slot holds
  ``(i, 0.0)``);
* the two Lanczos drivers: ``lanczos_law`` restates both recurrences in numpy float64 (same start vector,
  same check cadence, same stopping rule), ``expected_ground_state`` is the dense reference with the
  convention of Operator.ground_state for a degenerate lowest level, and ``LANCZOS_CASES`` are matrices
  with prescribed spectra, stored as ELL so that the device product runs inside the device drivers.

tests/test_lanczos_cases.py proves the restatements and the case tables on the CPU,
tests/test_gpu_sector_product.py and tests/test_gpu_lanczos.py compare the device with them."""
import collections.abc
import dataclasses
import functools
import math
from fractions import Fraction
from typing import Callable, Optional

import numpy as np

VARIANTS = ("unfused", "slots_reversed", "diagonal_last", "row_major", "pairwise")


# ---------------------------------------------------------------------------------------------------
# the product law
# ---------------------------------------------------------------------------------------------------

def _fma(v, xj, acc):
    """fma(v, xj, acc) of finite doubles: one rounding of the exact v * xj + acc, zeros signed as
    IEEE 754 signs them under round-to-nearest."""
    exact = Fraction(v) * Fraction(xj) + Fraction(acc)
    if exact != 0:
        rounded = float(exact)  # correctly rounded, subnormal results included
        return rounded if rounded != 0 else math.copysign(0.0, exact)
    if v != 0 and xj != 0:
        return 0.0  # an exact cancellation: +0
    negative_product = (math.copysign(1.0, v) < 0) != (math.copysign(1.0, xj) < 0)
    negative_acc = math.copysign(1.0, acc) < 0
    return -0.0 if (negative_product and negative_acc) else 0.0


def _pairwise(terms):
    if len(terms) == 1:
        return terms[0]
    half = (len(terms) + 1) // 2
    return _pairwise(terms[:half]) + _pairwise(terms[half:])


def ell_product_law(idx, val, diag, x, variant=None):
    """y of asp_sector_matvec, exactly: ``acc = diag[i] * x[i]``, then ``acc = fma(val[k, i],
    x[idx[k, i]], acc)`` for k = 0 .. width-1.  ``variant``: one of VARIANTS, that reading instead."""
    assert variant is None or variant in VARIANTS
    width, n = idx.shape
    assert val.shape == (width, n) and diag.shape == (n,) and x.shape == (n,)
    assert all(np.all(np.isfinite(a)) for a in (val, diag, x))
    flat_idx = [int(j) for j in idx.ravel()]
    flat_val = [float(v) for v in val.ravel()]
    d = [float(v) for v in diag]
    xs = [float(v) for v in x]
    if variant == "row_major":
        slot = lambda i, k: i * width + k  # noqa: E731
    else:
        slot = lambda i, k: k * n + i  # noqa: E731
    order = range(width - 1, -1, -1) if variant == "slots_reversed" else range(width)
    y = np.empty(n)
    for i in range(n):
        if variant == "pairwise":
            terms = [d[i] * xs[i]] + [flat_val[slot(i, k)] * xs[flat_idx[slot(i, k)]] for k in order]
            y[i] = _pairwise(terms)
            continue
        acc = 0.0 if variant == "diagonal_last" else d[i] * xs[i]
        for k in order:
            v, xj = flat_val[slot(i, k)], xs[flat_idx[slot(i, k)]]
            acc = acc + v * xj if variant == "unfused" else _fma(v, xj, acc)
        if variant == "diagonal_last":
            acc = _fma(d[i], xs[i], acc)
        y[i] = acc
    return y


# ---------------------------------------------------------------------------------------------------
# inputs of the product
# ---------------------------------------------------------------------------------------------------

PRODUCT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 4097)
PRODUCT_WIDTHS = (0, 1, 2, 7)
SUBNORMAL = 5e-324


def _vector(rng, n):
    """Standard normal with both zeros and a few subnormals sprinkled in (none when n is tiny)."""
    out = rng.standard_normal(n)
    draw = rng.random(n)
    out[draw < 0.06] = 0.0
    out[draw < 0.03] = -0.0
    tiny = (draw > 0.97) & (n > 2)
    out[tiny] = (rng.integers(1, 1 << 20, size=n) * SUBNORMAL * np.where(rng.random(n) < 0.5, 1, -1))[tiny]
    return out


def _product_case(n, width, seed):
    """Random columns and values; with width >= 2 every row reaches columns 0 and n-1; with width 7
    every row also holds one column twice and a padding slot ``(i, 0.0)`` at a random position (so
    mostly with used slots after it), every third row a self-index with a value; some values are
    +0.0, -0.0 or subnormal.  Nothing is symmetric."""
    rng = np.random.default_rng(seed)
    own = np.arange(n)
    idx = rng.integers(0, n, size=(width, n)).astype(np.uint32)
    val = rng.standard_normal((width, n))
    if width:
        draw = rng.random((width, n))
        val[draw < 0.04] = 0.0
        val[draw < 0.02] = -0.0
        tiny = draw > 0.98
        val[tiny] = (rng.integers(1, 1 << 20, size=(width, n)) * SUBNORMAL)[tiny] * np.sign(val[tiny])
    if width == 1:
        idx[0] = np.where(own % 2 == 0, 0, n - 1)
    if width >= 2:
        place = rng.permuted(np.tile(np.arange(width), (n, 1)), axis=1)  # per row, distinct slots
        if width >= 7:  # every fourth row keeps its last slot free for padding at the tail
            rows = np.flatnonzero(own % 4 == 1)
            last = np.argmax(place[rows] == width - 1, axis=1)
            place[rows, last] = place[rows, 6]
            place[rows, 6] = width - 1
        idx[place[:, 0], own] = 0
        idx[place[:, 1], own] = n - 1
    if width >= 7:
        twice = rng.integers(0, n, size=n)
        idx[place[:, 2], own] = twice
        idx[place[:, 3], own] = twice
        val[place[:, 2], own] = rng.standard_normal(n)  # both with a value
        val[place[:, 3], own] = rng.standard_normal(n)
        idx[place[:, 4], own] = own
        val[place[:, 4], own] = 0.0
        third = own % 3 == 0
        idx[place[third, 5], own[third]] = own[third]
        val[place[third, 5], own[third]] = rng.standard_normal(int(third.sum()))
        fourth = own % 4 == 1  # ... and padding at the tail as asp_sector_rows leaves it
        idx[width - 1, fourth] = own[fourth]
        val[width - 1, fourth] = 0.0
    return idx, val, _vector(rng, n), _vector(rng, n)


def dense_to_ell(h):
    """``(idx, val, diag)`` of a square matrix: row i's slots are its other columns, ascending."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    k, i = np.meshgrid(np.arange(n - 1), np.arange(n), indexing="ij")
    col = k + (k >= i)
    return col.astype(np.uint32), np.ascontiguousarray(h[i, col]), np.ascontiguousarray(np.diagonal(h))


def ell_to_dense(idx, val, diag):
    """The matrix of an ELL triple (slots of one row towards one column add up)."""
    width, n = idx.shape
    h = np.zeros((n, n))
    for k in range(width):
        np.add.at(h, (np.arange(n), idx[k].astype(np.int64)), val[k])
    h[np.arange(n), np.arange(n)] += diag
    return h


def _dense_product():
    rng = np.random.default_rng(300)
    h = rng.standard_normal((300, 300))  # (not symmetric)
    return dense_to_ell(h) + (rng.standard_normal(300),)


def _small(rows, diag, x):
    """rows: per row a list of (column, value) slots of equal length."""
    width, n = len(rows[0]), len(rows)
    idx = np.array([[rows[i][k][0] for i in range(n)] for k in range(width)], dtype=np.uint32).reshape(width, n)
    val = np.array([[rows[i][k][1] for i in range(n)] for k in range(width)], dtype=np.float64).reshape(width, n)
    return idx, val, np.array(diag, dtype=np.float64), np.array(x, dtype=np.float64)


def _cancel():
    """(1 + 2^-30)(1 - 2^-30) = 1 - 2^-60 needs 60 bits; on top of -1 the fused sum is -2^-60 and the
    twice-rounded one 0.  Row 1 has exact terms only, row 2 is row 0 with the signs turned and the
    padding first."""
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    rows = [[(1, a), (0, 0.0)], [(2, 1.0), (0, a)], [(2, 0.0), (1, -a)]]
    return _small(rows, [-1.0, -2.0, 1.0], [1.0, b, 1.0])


def _order():
    """x = 1.  Row 0: 0, then +1, +1e16, -1e16 in slot order gives 0 (1 + 1e16 rounds to 1e16), from
    the last slot down 1.  Row 1: the diagonal term 1 first is absorbed (0), added last it survives (1).
    Row 2: 3, 1e16, -1e16, 5 — in slot order 4 + 5 = 9, as a tree (0 + 3) + ... differs."""
    rows = [[(1, 1.0), (2, 1e16), (0, -1e16), (0, 0.0)],
            [(0, 1e16), (2, -1e16), (1, 0.0), (1, 0.0)],
            [(0, 3.0), (1, 1e16), (2, -1e16), (0, 5.0)]]
    return _small(rows, [0.0, 1.0, 0.0], [1.0, 1.0, 1.0])


def _signed_zeros():
    """Every row's result is a zero, x = (1, 1, 1, 1, -1, -0):
    row 0: (-0)(1), then (-0)(1) twice: -0;       row 1: (-0)(1), then (+0)(1) twice: +0;
    row 2: (-0)(1) + (+0)(-1) + (+0)(-0): -0;     row 3: (+0)(1) + (+0)(-1) twice: +0;
    row 4: (-1)(-1) + (-1)(1) cancels to +0, then + (+0)(-1): +0;
    row 5: (+0)(-0) = -0, + (-0)(-0) = +0, + (+0)(-0): +0."""
    rows = [[(0, -0.0), (0, -0.0)], [(1, 0.0), (1, 0.0)], [(4, 0.0), (5, 0.0)], [(4, 0.0), (4, 0.0)],
            [(0, -1.0), (4, 0.0)], [(5, -0.0), (5, 0.0)]]
    return _small(rows, [-0.0, -0.0, -0.0, 0.0, -1.0, 0.0], [1.0, 1.0, 1.0, 1.0, -1.0, -0.0])


def _subnormal():
    """Products that land among the subnormals and leave them again; a product that underflows to a
    signed zero; the smallest subnormal halved (ties to even: 0)."""
    rows = [[(1, 1e-160), (2, 3.0)], [(1, -1e-200), (0, 1.0)], [(2, 0.5), (1, -1e-160)]]
    return _small(rows, [1e-160, -0.0, 0.5], [2e-160, 1e-160, SUBNORMAL])


def _product_builders():
    out = {}
    for n in PRODUCT_SIZES:
        for width in PRODUCT_WIDTHS:
            out["n%d_w%d" % (n, width)] = functools.partial(_product_case, n, width, 1000 * width + n)
    out["dense300"] = _dense_product
    out["cancel"] = _cancel
    out["order"] = _order
    out["signed_zeros"] = _signed_zeros
    out["subnormal"] = _subnormal
    return out


class _Cases(collections.abc.Mapping):
    """name -> tuple of read-only arrays, each case built on first use."""

    def __init__(self, builders):
        self._builders, self._built = builders, {}

    def __getitem__(self, name):
        if name not in self._built:
            arrays = self._builders[name]()
            for a in arrays:
                a.flags.writeable = False
            self._built[name] = arrays
        return self._built[name]

    def __iter__(self):
        return iter(self._builders)

    def __len__(self):
        return len(self._builders)


PRODUCT_CASES = _Cases(_product_builders())
# which named case tells which wrong reading from the law
TOLD_APART = (("unfused", "cancel"), ("slots_reversed", "order"), ("diagonal_last", "order"),
              ("pairwise", "order"), ("row_major", "n65_w7"), ("row_major", "n2_w2"))


@functools.lru_cache(maxsize=None)
def product_law(name):
    """ell_product_law of a named case, computed once."""
    out = ell_product_law(*PRODUCT_CASES[name])
    out.flags.writeable = False
    return out


# ---------------------------------------------------------------------------------------------------
# references of the ground state
# ---------------------------------------------------------------------------------------------------

def spectrum_matrix(n, eigenvalues, seed):
    """``(idx, val, diag, dense)``: the symmetric ``Q diag(eigenvalues) Q^T`` with Q from the QR
    factorisation of a seeded normal matrix, as ELL of width n - 1 plus diag and as the dense float64
    matrix the ELL form holds (the reference)."""
    lam = np.asarray(eigenvalues, dtype=np.float64)
    assert lam.shape == (n,)
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0]
    h = (q * lam[None, :]) @ q.T
    h = 0.5 * (h + h.T)
    return dense_to_ell(h) + (h,)


def _sign_fixed(p):
    p = p / np.linalg.norm(p)
    return p * np.sign(p[np.argmax(np.abs(p))])


def _projection(values, vectors, seed, rtol):
    level = values <= values[0] + rtol * max(1.0, abs(values[0]))
    degeneracy = int(level.sum())
    space = vectors[:, :degeneracy]
    start = np.random.default_rng(seed).standard_normal(vectors.shape[0])
    gap = float(values[degeneracy] - values[0]) if degeneracy < values.shape[0] else math.inf
    return float(values[0]), _sign_fixed(space @ (space.T @ start)), degeneracy, gap, space


def expected_ground_state(h, seed, rtol=1e-8):
    """``(E0, p, degeneracy, gap, space)`` by numpy.linalg.eigh: the lowest level is every eigenvalue
    within ``rtol * max(1, |E0|)`` of the lowest; p is the normalised projection of
    ``default_rng(seed).standard_normal(n)`` onto it with the largest amplitude positive (the convention
    of Operator.ground_state); gap is the distance to the next level (inf if there is none); space the
    level's orthonormal basis."""
    values, vectors = np.linalg.eigh(np.asarray(h, dtype=np.float64))
    return _projection(values, vectors, seed, rtol)


def lanczos_law(h, seed, tol, max_iterations, reorthogonalise):
    """``(energy, vector, info)`` of sector_ed.lanczos_ground_state (``reorthogonalise=True``) or
    sector_ed.lanczos_two_pass (False) restated in numpy float64 with ``h @ v`` as the product
    (``h``: a dense or scipy.sparse matrix)."""
    import scipy.linalg

    n = h.shape[0]
    start = np.random.default_rng(seed).standard_normal(n)
    start = start / np.linalg.norm(start)

    def lowest(alphas, betas):
        if len(alphas) == 1:
            return float(alphas[0]), np.ones(1)
        theta, s = scipy.linalg.eigh_tridiagonal(np.asarray(alphas), np.asarray(betas), select="i",
                                                 select_range=(0, 0))
        return float(theta[0]), s[:, 0]

    def converged(residual, energy):
        return residual < tol * max(1.0, abs(energy))

    if reorthogonalise:
        steps = min(max_iterations, n)
        basis = np.empty((steps, n))
        v = start.copy()
        alphas, betas = [], []
        scale = 1.0
        for j in range(steps):
            basis[j] = v
            w = h @ v
            alphas.append(float(v @ w))
            for _ in range(2):
                w = w - basis[: j + 1].T @ (basis[: j + 1] @ w)
            beta = float(np.linalg.norm(w))
            used = j + 1
            scale = max(scale, abs(alphas[-1]), beta)
            done = beta < 1e-13 * scale or used == steps
            if used % 5 == 0 or done:
                energy, ritz = lowest(alphas, betas)
                residual = abs(beta * ritz[-1])
                if converged(residual, energy) or done:
                    break
            betas.append(beta)
            v = w / beta
        vector = basis[:used].T @ ritz
    else:
        def recurrence(steps, combine=None):
            v, previous = start.copy(), np.zeros(n)
            total = np.zeros(n) if combine is not None else None
            alphas, betas, beta, scale = [], [], 0.0, 1.0
            for j in range(steps):
                if total is not None:
                    total = total + float(combine[j]) * v
                    if j + 1 == steps:
                        break
                w = h @ v
                alpha = float(v @ w)
                w = w - alpha * v
                if j > 0:
                    w = w - beta * previous
                alphas.append(alpha)
                beta = float(np.linalg.norm(w))
                if combine is None:
                    scale = max(scale, abs(alpha), beta)
                    done = beta < 1e-13 * scale or j + 1 == steps
                    if (j + 1) % 10 == 0 or done:
                        energy, ritz = lowest(alphas, betas)
                        residual = abs(beta * ritz[-1])
                        if converged(residual, energy) or done:
                            return alphas, ritz, float(residual)
                betas.append(beta)
                previous, v = v, w / beta
            return total

        alphas, ritz, residual = recurrence(min(max_iterations, n))
        used = len(alphas)
        vector = recurrence(used, combine=ritz)
    vector = vector / np.linalg.norm(vector)
    hv = h @ vector
    energy = float(vector @ hv)
    true_residual = float(np.linalg.norm(hv - energy * vector))
    if vector[np.argmax(np.abs(vector))] < 0:
        vector = -vector
    return energy, vector, {"iterations": used, "ritz_residual": float(residual), "residual": true_residual}


# ---------------------------------------------------------------------------------------------------
# matrices for the drivers
# ---------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class LanczosCase:
    name: str
    build: Callable[[], tuple]              # -> (idx, val, diag, h): h dense, or scipy.sparse for `banded`
    degeneracy: int                         # of the lowest level, as the name claims
    gap_at_least: float                     # ... and its distance to the next level
    tol: float = 1e-11
    max_iterations: int = 400
    seed: int = 0                           # of the start vector (the Q of spectrum_matrix has its own)
    converges: bool = True                  # False: the step budget runs out
    drivers: tuple = (True, False)          # reorthogonalise = True / False
    max_steps: Optional[tuple] = None       # (full reorthogonalisation, two-pass): iterations <= this
    exact_steps: Optional[int] = None       # iterations == this
    scale_of: Optional[str] = None          # this case is that one times 2**30
    banded: bool = False


def _random_levels():
    return np.sort(np.random.default_rng(2024).uniform(-30.0, 10.0, size=300))


def _random300(change=None):
    lam = _random_levels()
    if change == "degenerate":
        lam[1] = lam[2] = lam[0]
    elif change == "near":
        lam[1] = lam[0] + 1e-6
    elif change == "positive":
        lam = lam + 100.0
    return spectrum_matrix(300, lam, seed=4300)


def _three_levels(multiplicity, scale=1.0):
    lam = np.repeat([-4.0, 1.0, 2.5], multiplicity)
    idx, val, diag, h = spectrum_matrix(200, lam, seed=4200)
    return idx, val * scale, diag * scale, h * scale  # (a power of two: exact)


def _cluster_levels(degenerate):
    """500 levels in [-1, -0.9]: the lowest at -1, the others spread over [-0.98, -0.9]; far above them
    10, 20 and 50, which the recurrence finds first and, without reorthogonalisation, finds again."""
    rng = np.random.default_rng(503)
    lam = np.concatenate([[-1.0], np.sort(rng.uniform(-0.98, -0.9, size=499)), [10.0, 20.0, 50.0]])
    if degenerate:
        lam[1] = lam[2] = lam[0]
    return spectrum_matrix(503, lam, seed=4503)


def _ladder():
    """601 states: the lowest level at -1, a gap of 1e-4, then a geometric ladder of 600 levels from
    -1 + 1e-4 to 99.  Without reorthogonalisation the recurrence is still far from converged at its cap of
    n steps (the restatement: Ritz residual 4e-3 after 601 steps; with full reorthogonalisation it
    converges in 455)."""
    ratio = (100.0 / 1e-4) ** (1.0 / 599.0)
    lam = -1.0 + np.concatenate([[0.0], 1e-4 * ratio ** np.arange(600)])
    return spectrum_matrix(601, lam, seed=4601)


BAND_ROWS = 4097
BAND_SLOPE = 0.001


def band_arrays():
    """``(diagonal, first, second)``: 0.001 i on the diagonal, couplings to i +- 1 and i +- 2 that vary
    along the band.  The slope decides the step count, and a steeper one lengthens the run (the spectrum
    widens faster than the lowest gap): at tol 1e-9 the restatement needs 165 / 170 steps (full
    reorthogonalisation / two-pass) with 0.001 i, 210 / 210 with 0.01 i, 240 / 240 with 0.03 i and
    295 / 300 with 0.1 i.  So the band is flatter than 0.01 i, to converge within 200 steps."""
    i = np.arange(BAND_ROWS, dtype=np.float64)
    return BAND_SLOPE * i, -1.0 - 0.25 * np.cos(0.37 * i[:-1]), 0.5 + 0.125 * np.sin(0.11 * i[:-2])


def _banded():
    import scipy.sparse

    n = BAND_ROWS
    diagonal, first, second = band_arrays()
    own = np.arange(n, dtype=np.uint32)
    idx = np.tile(own, (4, 1))
    val = np.zeros((4, n))
    # slots: i-1, i+1, i-2, i+2; the rows at the two ends keep padding (i, 0.0) in their first slots
    idx[0, 1:], val[0, 1:] = own[:-1], first
    idx[1, :-1], val[1, :-1] = own[1:], first
    idx[2, 2:], val[2, 2:] = own[:-2], second
    idx[3, :-2], val[3, :-2] = own[2:], second
    h = scipy.sparse.diags([second, first, diagonal, first, second], [-2, -1, 0, 1, 2], format="csr")
    return idx, val, diagonal, h


def _tiny(n):
    return LanczosCase("tiny%d" % n, lambda: spectrum_matrix(n, np.arange(n) - 2.5, seed=4000 + n), 1, 1.0 - 1e-9,
                       max_steps=(n, n))


def _exact(h):
    return lambda: dense_to_ell(h) + (np.asarray(h, dtype=np.float64),)


_LANCZOS = [_tiny(n) for n in range(1, 8)] + [
    LanczosCase("zero1", _exact(np.zeros((1, 1))), 1, math.inf, exact_steps=1),
    LanczosCase("zero50", _exact(np.zeros((50, 50))), 50, math.inf, exact_steps=1),
    LanczosCase("minus3_identity50", _exact(-3.0 * np.eye(50)), 50, math.inf, exact_steps=1),
    LanczosCase("three_levels_1_100_99", lambda: _three_levels((1, 100, 99)), 1, 5.0 - 1e-9, max_steps=(5, 10)),
    LanczosCase("three_levels_3_100_97", lambda: _three_levels((3, 100, 97)), 3, 5.0 - 1e-9, max_steps=(5, 10)),
    LanczosCase("three_levels_1_100_99_times_2^30", lambda: _three_levels((1, 100, 99), 2.0 ** 30), 1,
                (5.0 - 1e-9) * 2.0 ** 30, max_steps=(5, 10), scale_of="three_levels_1_100_99"),
    LanczosCase("diagonal_30_fold", _exact(np.diag(np.repeat(np.arange(-5.0, 5.0), 30))), 30, 1.0,
                max_steps=(10, 10)),
    LanczosCase("random300", _random300, 1, 0.01),
    LanczosCase("random300_three_equal", lambda: _random300("degenerate"), 3, 0.01),
    LanczosCase("random300_second_at_1e-6", lambda: _random300("near"), 1, 0.99e-6),
    LanczosCase("random300_plus_100", lambda: _random300("positive"), 1, 0.01),
    LanczosCase("cluster500_outliers", lambda: _cluster_levels(False), 1, 0.02 - 1e-9),
    LanczosCase("cluster500_outliers_three_equal", lambda: _cluster_levels(True), 3, 0.02 - 1e-9),
    LanczosCase("random300_budget20", _random300, 1, 0.01, max_iterations=20, converges=False, exact_steps=20),
    LanczosCase("ladder601_two_pass_cap", _ladder, 1, 0.99e-4, tol=1e-9, max_iterations=1000, converges=False,
                drivers=(False,), exact_steps=601),
    LanczosCase("banded4097", _banded, 1, 1e-3, tol=1e-9, max_iterations=200, banded=True),
]
LANCZOS_CASES = {case.name: case for case in _LANCZOS}


@functools.lru_cache(maxsize=None)
def lanczos_matrix(name):
    """``(idx, val, diag, h)`` of a named case, built once, read-only."""
    arrays = LANCZOS_CASES[name].build()
    for a in arrays[:3]:
        a.flags.writeable = False
    if isinstance(arrays[3], np.ndarray):
        arrays[3].flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def lanczos_reference(name):
    """Everything the tests compare with, computed once per case: ``energy``, ``vector`` (the
    projection p), ``degeneracy``, ``gap``, ``space``, ``norm`` (the spectral norm of H) and per driver
    (key ``True``: full reorthogonalisation, ``False``: two-pass) the result of lanczos_law with
    ``distance = |vector_law - p|``."""
    case = LANCZOS_CASES[name]
    h = lanczos_matrix(name)[3]
    if case.banded:
        import scipy.linalg

        diagonal, first, second = band_arrays()
        bands = np.zeros((3, BAND_ROWS))
        bands[0], bands[1, :-1], bands[2, :-2] = diagonal, first, second
        values = scipy.linalg.eig_banded(bands, lower=True, eigvals_only=True, select="i", select_range=(0, 1))
        top = scipy.linalg.eig_banded(bands, lower=True, eigvals_only=True, select="i",
                                      select_range=(BAND_ROWS - 1, BAND_ROWS - 1))
        # the lowest level's vector by inverse iteration just below it (eig_banded's own vectors take
        # seconds at this size): each solve shrinks the other components by 1e-3 or more
        shifted = np.zeros((5, BAND_ROWS))
        shifted[2] = diagonal - (values[0] - 1e-3 * (values[1] - values[0]))
        shifted[1, 1:], shifted[3, :-1], shifted[0, 2:], shifted[4, :-2] = first, first, second, second
        vector = np.random.default_rng(case.seed).standard_normal(BAND_ROWS)
        for _ in range(8):
            vector = scipy.linalg.solve_banded((2, 2), shifted, vector)
            vector /= np.linalg.norm(vector)
        energy, p, degeneracy, gap, space = _projection(values, vector[:, None], case.seed, 0.0)
        gap = float(values[1] - values[0])
        norm = float(max(abs(values[0]), abs(top[0])))
    else:
        values = np.linalg.eigvalsh(h)
        energy, p, degeneracy, gap, space = expected_ground_state(h, case.seed)
        norm = float(np.abs(values).max())
    out = {"energy": energy, "vector": p, "degeneracy": degeneracy, "gap": gap, "space": space, "norm": norm}
    for reorthogonalise in case.drivers:
        e, v, info = lanczos_law(h, case.seed, case.tol, case.max_iterations, reorthogonalise)
        out[reorthogonalise] = dict(info, energy=e, vector=v, distance=float(np.linalg.norm(v - p)))
    return out


def eigen_residual(h, v):
    """``|H v - (v.Hv) v|`` in float64 with the reference matrix."""
    hv = h @ v
    return float(np.linalg.norm(hv - float(v @ hv) * v))


def sine_to_level(space, v):
    """Sine of the angle between v and the span of the orthonormal columns of `space`."""
    v = v / np.linalg.norm(v)
    return float(np.linalg.norm(v - space @ (space.T @ v)))
