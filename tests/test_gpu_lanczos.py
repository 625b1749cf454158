"""The two Lanczos drivers of annealing_sign_problem_amd/sector_ed.py (lanczos_ground_state: full
reorthogonalisation; lanczos_two_pass: three vectors), ground_state() and main() — on matrices with
prescribed spectra handed over as ELL arrays (tests/lanczos_cases.py; the device product runs inside the
device drivers) and on the models whose routes nothing else takes: sectors of 1 to 7 states, a
one-dimensional Krylov space, breakdown, the checks at multiples of 5 and 10 steps, an exhausted budget,
the ``representatives=`` route of Operator.ground_state, the matrix-free switch inside ground_state() and
main's refusal to write an unconverged state.

What is compared is the returned VECTOR, three ways:

* rigorously: with r = |H v - (v.Hv) v| recomputed in float64 with the reference matrix, the sine of the
  angle between v and the reference's lowest level is at most r / gap (Davis-Kahan); asserted with
  2 r / gap + 64 eps (the factor 2 for the reference's own rounding);
* against p, the projection of the start vector onto the level (lanczos_cases.expected_ground_state, the
  convention of Operator.ground_state): inside a degenerate level no bound can be derived, so the distance
  is measured against the numpy restatement of the same recurrence, d_ref = |lanczos_law(...) - p|, and
  |v - p| <= max(16 d_ref, 2 r / gap + 64 eps sqrt(n)) is asserted, and never more than 1e-6 (the margin
  of 16: torch.mv and torch.dot sum in another order than numpy, which a Krylov recurrence amplifies);
* norm 1 to 1e-12 and the largest amplitude positive.

Measured |v - p| (numpy restatement / MI355X), full reorthogonalisation and two-pass:

    case                               full reorthogonalisation   two-pass
    tiny1, zero1                       0       / 0                0       / 0
    tiny2                              2.2e-16 / 2.5e-16          3.5e-16 / 2.6e-15
    tiny3                              3.0e-16 / 3.7e-16          2.3e-16 / 2.5e-16
    tiny4                              4.8e-16 / 4.3e-16          4.1e-16 / 3.6e-16
    tiny5                              7.4e-16 / 6.5e-16          7.7e-16 / 6.4e-16
    tiny6                              5.5e-16 / 5.1e-16          4.8e-16 / 6.6e-16
    tiny7                              6.4e-16 / 5.4e-16          6.2e-16 / 6.9e-16
    zero50, minus3_identity50          2.3e-16 / 1.4e-16          2.3e-16 / 1.4e-16
    three_levels_1_100_99 (and x 2^30) 1.7e-15 / 1.7e-15          1.7e-15 / 1.7e-15
    three_levels_3_100_97              9.3e-16 / 9.4e-16          9.2e-16 / 9.3e-16
    diagonal_30_fold                   5.6e-16 / 4.5e-16          5.5e-16 / 6.1e-16
    random300                          4.5e-12 / 4.5e-12          4.5e-12 / 4.5e-12
    random300_three_equal              3.1e-11 / 3.1e-11          3.1e-11 / 3.1e-11
    random300_second_at_1e-6           2.8e-09 / 4.4e-09          1.8e-09 / 2.4e-09
    random300_plus_100                 4.5e-12 / 4.5e-12          4.7e-12 / 4.9e-12
    cluster500_outliers                5.1e-12 / 5.1e-12          1.3e-11 / 1.3e-11
    cluster500_outliers_three_equal    2.0e-12 / 2.0e-12          1.5e-11 / 1.5e-11
    banded4097                         2.5e-09 / 2.5e-09          1.3e-09 / 1.3e-09
    kagome_18, representatives= route  3.1e-09 / 3.1e-09          -
    sk_16_1 (resident / matrix-free)   2.4e-10 / 2.4e-10          3.8e-11 / 3.8e-11
    chain18 (resident / matrix-free)   2.6e-10 / 2.6e-10          1.5e-11 / 1.5e-11

The times-2^30 run takes the unscaled run's 3 steps and returns its vector bit for bit.  It did not before
this test: the drivers judged breakdown by ``beta < 1e-13`` whatever the size of the matrix, so the scaled
run missed the breakdown at step 3, divided by a beta of rounding noise and went on to its next check
(5 steps with full reorthogonalisation, 10 in two passes); breakdown is now judged relative to the largest
alpha or beta seen so far, with a floor of 1.

sk_16_1 and the 18-site chain have ground states that are odd under a symmetry of their model: the two
largest amplitudes are +a and -a, the sign convention decides nothing and rounding picks the sign.  For
them (and only where the reference shows that tie) the distance is taken up to the global sign.
"""
import math

import numpy as np
import pytest

import lanczos_cases
from lanczos_cases import LANCZOS_CASES

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
_RUNS = {}


class _Ell:
    """What the drivers need of a matrix: n and matvec; and what sector_ed.SectorMatrix.matvec reads of
    its object: n, width, idx, val and diag on the device."""

    def __init__(self, idx, val, diag):
        import torch

        self.width, self.n = idx.shape
        self.idx = torch.tensor(idx.view(np.int32), device="cuda")  # (the device array holds the u32 as i32)
        self.val = torch.tensor(val, device="cuda")
        self.diag = torch.tensor(diag, device="cuda")

    def matvec(self, x, out=None):
        from annealing_sign_problem_amd import sector_ed

        return sector_ed.SectorMatrix.matvec(self, x, out=out)


def _run(name, reorthogonalise):
    """(energy, vector on the host, info) of the device driver on a named case, run once."""
    from annealing_sign_problem_amd import sector_ed

    key = (name, reorthogonalise)
    if key not in _RUNS:
        case = LANCZOS_CASES[name]
        matrix = _Ell(*lanczos_cases.lanczos_matrix(name)[:3])
        driver = sector_ed.lanczos_ground_state if reorthogonalise else sector_ed.lanczos_two_pass
        energy, vector, info = driver(matrix, tol=case.tol, max_iterations=case.max_iterations, seed=case.seed)
        _RUNS[key] = (energy, vector.cpu().numpy(), info)
    return _RUNS[key]


def _sign_is_a_tie(p):
    """The sign convention (largest amplitude positive) decides nothing where the two largest amplitudes
    are equal and opposite — the ground state is odd under a symmetry of the matrix; rounding then picks
    the sign."""
    if p.shape[0] < 2:
        return False
    first, second = np.argsort(-np.abs(p))[:2]
    return p[first] * p[second] < 0 and abs(abs(p[first]) - abs(p[second])) <= 1e-12


def _vector_checks(label, v, h, p, space, gap, norm, d_ref, info=None):
    """The three comparisons of the module docstring; returns (r, |v - p|).  ``d_ref`` is a distance or,
    to measure it here, the restatement's vector; where the sign convention is a tie, both distances are
    taken up to the sign."""
    n = v.shape[0]
    if not isinstance(d_ref, float):
        d_ref = float(min(np.linalg.norm(d_ref - p), np.linalg.norm(d_ref + p)) if _sign_is_a_tie(p)
                      else np.linalg.norm(d_ref - p))
    assert v.dtype == np.float64 and v.shape == p.shape and np.all(np.isfinite(v))
    assert abs(np.linalg.norm(v) - 1.0) < 1e-12
    assert v[np.argmax(np.abs(v))] > 0
    r = lanczos_cases.eigen_residual(h, v)
    sine = lanczos_cases.sine_to_level(space, v)
    distance = float(np.linalg.norm(v - p))
    if _sign_is_a_tie(p):
        distance = min(distance, float(np.linalg.norm(v + p)))
    allowed = min(max(16.0 * d_ref, 2.0 * r / gap + 64.0 * EPS * math.sqrt(n)), 1e-6)
    print("%s: d_ref %.3e, device |v - p| %.3e (allowed %.3e), r %.3e, gap %.3g, sine %.3e"
          % (label, d_ref, distance, allowed, r, gap, sine))
    assert sine <= 2.0 * r / gap + 64.0 * EPS, (sine, r, gap)
    if info is not None:
        assert abs(info["residual"] - r) <= 1e-12 * norm + 0.5 * r, (info, r)
    assert distance <= allowed, (distance, allowed, d_ref)
    return r, distance


CONVERGING = [(name, d) for name, case in LANCZOS_CASES.items() if case.converges for d in case.drivers]
_IDS = ["%s-%s" % (n, "full" if d else "two_pass") for n, d in CONVERGING]


@pytest.mark.parametrize("name,reorthogonalise", CONVERGING, ids=_IDS)
def test_driver_returns_the_reference_ground_state(name, reorthogonalise):
    case, ref = LANCZOS_CASES[name], lanczos_cases.lanczos_reference(name)
    law = ref[reorthogonalise]
    h = lanczos_cases.lanczos_matrix(name)[3]
    energy, v, info = _run(name, reorthogonalise)
    n = v.shape[0]
    scale = max(1.0, abs(ref["energy"]))
    print("%s: %d steps (restatement %d), E - E_ref = %.3e, info %s"
          % (name, info["iterations"], law["iterations"], energy - ref["energy"], info))
    assert abs(energy - ref["energy"]) <= 1e-9 * scale
    # converged, by the criterion of the iteration or by a Krylov space that is complete or broke down
    assert info["iterations"] <= min(case.max_iterations, n)
    assert info["ritz_residual"] < case.tol * max(1.0, abs(energy)) or info["iterations"] == n
    if case.max_steps:
        assert info["iterations"] <= case.max_steps[0 if reorthogonalise else 1]
    if case.exact_steps:
        assert info["iterations"] == case.exact_steps
    _vector_checks("%s %s" % (name, "full" if reorthogonalise else "two-pass"), v, h, ref["vector"], ref["space"],
                   ref["gap"], ref["norm"], law["distance"], info)


@pytest.mark.parametrize("reorthogonalise", [True, False], ids=["full", "two_pass"])
def test_a_matrix_times_two_to_the_thirtieth_gives_the_same_vector_in_the_same_steps(reorthogonalise):
    scaled, = [name for name, case in LANCZOS_CASES.items() if case.scale_of]
    energy, v, info = _run(scaled, reorthogonalise)
    small_energy, small_v, small_info = _run(LANCZOS_CASES[scaled].scale_of, reorthogonalise)
    print("scaled: %d steps, unscaled: %d steps, |v - v'| = %.3e" % (
        info["iterations"], small_info["iterations"], np.linalg.norm(v - small_v)))
    assert np.linalg.norm(v - small_v) <= 1e-12
    assert abs(energy - small_energy * 2.0 ** 30) <= 1e-9 * abs(energy)
    assert info["iterations"] == small_info["iterations"]


EXHAUSTED = [(name, d) for name, case in LANCZOS_CASES.items() if not case.converges for d in case.drivers]


@pytest.mark.parametrize("name,reorthogonalise", EXHAUSTED,
                         ids=["%s-%s" % (n, "full" if d else "two_pass") for n, d in EXHAUSTED])
def test_an_exhausted_budget_is_reported_as_unconverged(name, reorthogonalise):
    case, ref = LANCZOS_CASES[name], lanczos_cases.lanczos_reference(name)
    energy, v, info = _run(name, reorthogonalise)
    print("%s: %s, E = %.12f (reference %.12f)" % (name, info, energy, ref["energy"]))
    assert info["iterations"] == case.exact_steps
    assert info["ritz_residual"] > case.tol * max(1.0, abs(energy))
    assert energy >= ref["energy"] - 1e-9          # a Ritz value is an upper bound
    assert info["residual"] >= 0.5 * info["ritz_residual"]
    assert abs(np.linalg.norm(v) - 1.0) < 1e-12 and v[np.argmax(np.abs(v))] > 0
    h = lanczos_cases.lanczos_matrix(name)[3]
    r = lanczos_cases.eigen_residual(h, v)
    assert abs(info["residual"] - r) <= 1e-12 * ref["norm"] + 0.5 * r


def test_main_refuses_to_write_an_unconverged_state(tmp_path, capsys):
    import os

    from annealing_sign_problem_amd import common, sector_ed

    path = str(tmp_path / "kagome_16.h5")
    arguments = ["--model", "heisenberg_kagome_16", "--max-iterations", "5", "--output", path]
    with pytest.raises(SystemExit) as err:
        sector_ed.main(arguments)
    assert "did not converge" in str(err.value) and "after 5 steps" in str(err.value)
    assert not os.path.exists(path) and os.listdir(str(tmp_path)) == []
    sector_ed.main(arguments + ["--allow-unconverged"])
    psi, energy, representatives = common.load_ground_state(path)
    assert psi.shape == representatives.shape == (12870,) and representatives.dtype == np.uint64
    assert np.all(np.diff(representatives.astype(np.int64)) > 0)
    assert all(bin(int(s)).count("1") == 8 for s in representatives[::97])
    assert abs(np.linalg.norm(psi) - 1.0) < 1e-12 and psi[np.argmax(np.abs(psi))] > 0
    assert ("E0 = %.12f" % energy) in capsys.readouterr().out
    # five steps from a random vector: a Ritz value above the ground state (-32.83... for this model)
    assert -33.0 < energy < 0.0


def _sparse_reference(h, seed):
    """(E0, p, space, gap, spectral norm) of a sparse symmetric matrix the way Operator.ground_state finds its level:
    the six lowest pairs by eigsh, the level within 1e-8, p the projection of the start vector."""
    import scipy.sparse.linalg

    start = np.random.default_rng(seed).standard_normal(h.shape[0])
    values, vectors = scipy.sparse.linalg.eigsh(h, k=6, which="SA", v0=start, tol=1e-13)
    order = np.argsort(values)
    values, vectors = values[order], vectors[:, order]
    level = np.abs(values - values[0]) <= 1e-8 * max(1.0, abs(values[0]))
    assert not level.all()
    space = np.linalg.qr(vectors[:, level])[0]
    p = space @ (space.T @ start)
    p /= np.linalg.norm(p)
    top = scipy.sparse.linalg.eigsh(h, k=1, which="LA", tol=1e-6, return_eigenvectors=False)[0]
    return (float(values[0]), p * np.sign(p[np.argmax(np.abs(p))]), space,
            float(values[int(level.sum())] - values[0]), float(max(abs(values[0]), abs(top))))


def test_operator_ground_state_above_the_host_limit_returns_the_stored_kagome_18_state(models):
    """The ``representatives=`` route (sector_norms instead of the enumeration), on the three-fold
    degenerate lowest level of heisenberg_kagome_18: the device starts from the same vector as the host
    route, so it returns the same state of the level — the stored one."""
    from conftest import golden

    from annealing_sign_problem_amd import operators, sector_ed

    stored = golden("heisenberg_kagome_18_ground_state.npz")
    operator = operators.Operator.from_config(models["heisenberg_kagome_18"])
    operator.basis.build()
    states = operator.basis.states
    assert np.array_equal(states, stored["representatives"]) and states.shape == (24310,)
    norms = sector_ed.sector_norms(operator, states)
    assert norms.cpu().numpy().tobytes() == operator.basis.group.state_info(states)[2].tobytes()
    calls = []
    original = sector_ed.ground_state

    def spy(*args, **kwargs):
        calls.append(kwargs.get("representatives"))
        return original(*args, **kwargs)

    operator.HOST_ED_LIMIT = 1000  # (instance attribute: this operator only)
    sector_ed.ground_state = spy
    try:
        energy, psi = operator.ground_state()
    finally:
        sector_ed.ground_state = original
    assert len(calls) == 1 and calls[0] is states
    assert abs(energy - float(stored["energy"])) <= 1e-9
    h = operator.to_sparse().real.tocsr()
    want_energy, p, space, gap, norm = _sparse_reference(h, seed=0)
    assert space.shape[1] == 3 and abs(want_energy - float(stored["energy"])) <= 1e-9
    golden_psi = stored["psi"]
    assert np.linalg.norm(golden_psi - p) <= 1e-9  # the stored state is the projection
    law_energy, law_vector, law_info = lanczos_cases.lanczos_law(h, 0, 1e-9, 400, True)
    assert law_info["ritz_residual"] < 1e-9 * abs(law_energy)
    assert not _sign_is_a_tie(golden_psi)
    d_ref = float(np.linalg.norm(law_vector - golden_psi))
    _vector_checks("kagome_18 representatives route", psi, h, golden_psi, space, gap, norm, d_ref)


def _chain18():
    from annealing_sign_problem_amd import operators

    return operators.Operator(operators.SpinBasis(18, 7), [
        operators.Term(operators.SIGMA_DOT_SIGMA, [(i, (i + 1) % 18) for i in range(18)]),
        operators.Term(0.37 * operators.SIGMA_DOT_SIGMA, [(i, (i + 5) % 18) for i in range(18)])])


@pytest.mark.parametrize("name", ["sk_16_1", "chain18"])
def test_ground_state_switches_to_the_matrix_free_route_when_memory_is_short(name, models, monkeypatch):
    import torch

    from annealing_sign_problem_amd import operators, sector_ed

    operator = _chain18() if name == "chain18" else operators.Operator.from_config(models[name])
    taken = []
    for driver in ("lanczos_ground_state", "lanczos_two_pass"):
        def spy(*args, _driver=driver, _original=getattr(sector_ed, driver), **kwargs):
            taken.append(_driver)
            return _original(*args, **kwargs)
        monkeypatch.setattr(sector_ed, driver, spy)
    resident = sector_ed.ground_state(operator, tol=1e-10)
    assert taken == ["lanczos_ground_state"]
    total = torch.cuda.mem_get_info()[1]
    with monkeypatch.context() as patch:
        patch.setattr(torch.cuda, "mem_get_info", lambda *args, **kwargs: (1 << 20, total))
        matrix_free = sector_ed.ground_state(operator, tol=1e-10)
    assert taken == ["lanczos_ground_state", "lanczos_two_pass"]
    operator.basis.build()
    h = operator.to_sparse().real.tocsr()
    want_energy, p, space, gap, norm = _sparse_reference(h, seed=0)
    # both ground states are odd under a symmetry of their model: +a and -a are the two largest amplitudes
    assert space.shape[1] == 1 and _sign_is_a_tie(p)
    for label, reorthogonalise, (energy, psi, states, info) in (("resident", True, resident),
                                                                 ("matrix-free", False, matrix_free)):
        assert states.dtype == np.uint64 and np.array_equal(states, operator.basis.states)
        assert info["dimension"] == states.shape[0] == h.shape[0]
        assert abs(energy - want_energy) <= 1e-9 * max(1.0, abs(want_energy))
        assert info["ritz_residual"] < 1e-10 * max(1.0, abs(energy))
        _, law_vector, law_info = lanczos_cases.lanczos_law(h, 0, 1e-10, 400 if reorthogonalise else 1000,
                                                            reorthogonalise)
        assert law_info["ritz_residual"] < 1e-10 * max(1.0, abs(want_energy))
        _vector_checks("%s %s" % (name, label), psi, h, p, space, gap, norm, law_vector, info)
    assert abs(resident[0] - matrix_free[0]) <= 1e-9 * max(1.0, abs(want_energy))
