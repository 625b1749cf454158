"""Bond statistics on the GPU (csrc/bond_stats.hip, annealing_sign_problem_amd/bonds.py):
every named case of tests/bond_cases.py against the sequential numpy law, exactly; signs replaced on a
resident matrix; handles read twice and side by side; the refusals; and the three analyses of
common.py on a whole basis and on a sampled cluster against the reference's formulas in numpy."""
import ctypes

import numpy as np
import pytest

import bond_cases

pytestmark = pytest.mark.gpu

SUMMARY_FIELDS = ("num_spins", "stored", "bonds", "frustrated", "rows_with_bonds", "strongest_frustrated")


def _open(name, bits=None):
    from annealing_sign_problem_amd.bonds import BondStatistics

    indptr, indices, data, case_bits = bond_cases.cases()[name]
    return BondStatistics((indptr, indices, data), case_bits if bits is None else bits)


def _check_summary_and_rows(stats, law):
    summary = stats.summary
    for field in SUMMARY_FIELDS:
        assert summary[field] == law[field], field
    for field in ("max_abs", "min_abs"):  # exact: extrema of bit patterns
        assert np.float64(summary[field]).view(np.uint64) == np.float64(law[field]).view(np.uint64), field
    strongest, col, frustrated = stats.rows()
    assert np.array_equal(strongest.view(np.uint64), law["strongest"].view(np.uint64))
    assert np.array_equal(col, law["strongest_col"])
    assert np.array_equal(frustrated, law["strongest_frustrated_rows"])


def _check_histogram(stats, law, edges):
    normal, frustrated, below, above = stats.histogram(edges)
    want = bond_cases.histogram_law(law, edges)
    assert normal.dtype == frustrated.dtype == np.uint64
    assert np.array_equal(normal, want[0]) and np.array_equal(frustrated, want[1])
    assert (below, above) == want[2:]


@pytest.mark.parametrize("name", list(bond_cases.cases()))
def test_case_equals_the_law(name):
    law = bond_cases.law(name)
    with _open(name) as stats:
        _check_summary_and_rows(stats, law)
        for _, case, edges in bond_cases.HISTOGRAMS:
            if case == name:
                _check_histogram(stats, law, edges)
        if law["bonds"]:  # every case: one bin around everything, and the edges at the extrema themselves
            _check_histogram(stats, law, np.array([0.0, 1e300]))
            if law["min_abs"] < law["max_abs"]:
                _check_histogram(stats, law, np.array([law["min_abs"], law["max_abs"]]))
        else:
            _check_histogram(stats, law, np.array([0.5, 1.0, 2.0]))
        magnitudes = stats.magnitudes()
        want = bond_cases.magnitudes_law(law)
        assert magnitudes.shape == want.shape
        assert np.array_equal(magnitudes.view(np.uint64), want.view(np.uint64))


def test_set_signs_equals_a_fresh_handle():
    bits = bond_cases.cases()["k129"][3]
    other = bond_cases.cases()["k129_alternating"][3]
    edges = bond_cases.HISTOGRAMS[2][2]
    with _open("k129") as stats:
        _check_summary_and_rows(stats, bond_cases.law("k129"))
        assert stats.set_signs(other) is stats
        law = bond_cases.law("k129_alternating")
        assert law["frustrated"] != bond_cases.law("k129")["frustrated"]
        _check_summary_and_rows(stats, law)
        _check_histogram(stats, law, edges)
        with _open("k129", bits=other) as fresh:
            assert fresh.summary == stats.summary
            for a, b in zip(fresh.rows(), stats.rows()):
                assert np.array_equal(a, b)
            for a, b in zip(fresh.histogram(edges), stats.histogram(edges)):
                assert np.array_equal(a, b)
        stats.set_signs(bits)  # and back
        _check_summary_and_rows(stats, bond_cases.law("k129"))


def test_one_handle_read_twice_and_two_handles_alive():
    edges = bond_cases.HISTOGRAMS[3][2]
    with _open("row_lengths") as first, _open("tie") as second:
        for _ in range(2):
            _check_summary_and_rows(first, bond_cases.law("row_lengths"))
            _check_histogram(first, bond_cases.law("row_lengths"), edges)
            _check_summary_and_rows(second, bond_cases.law("tie"))
            assert np.array_equal(first.magnitudes(), bond_cases.magnitudes_law(bond_cases.law("row_lengths")))
            assert np.array_equal(second.magnitudes(), bond_cases.magnitudes_law(bond_cases.law("tie")))
    with pytest.raises(ValueError):
        first.summary  # released


def test_refusals():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd.bonds import BondStatistics

    indptr, indices, data, bits = bond_cases.cases()["k65"]
    for bad in (np.nan, np.inf, -np.inf):
        broken = data.copy()
        broken[3] = bad
        with pytest.raises(_lib.AspError) as err:
            BondStatistics((indptr, indices, broken), bits)
        assert err.value.code == -3 and "not finite" in str(err.value)
    for column in (65, -1):
        broken = indices.copy()
        broken[5] = column
        with pytest.raises(_lib.AspError) as err:
            BondStatistics((indptr, broken, data), bits)
        assert err.value.code == -3
    broken = indptr.copy()
    broken[4] = broken[5] + 1
    with pytest.raises(_lib.AspError) as err:
        BondStatistics((broken, indices, data), bits)
    assert err.value.code == -3
    with _open("k65") as stats:
        for edges in ([1.0], [1.0, 1.0], [1.0, 2.0, 2.0], [2.0, 1.0], [1.0, np.nan], [1.0, np.inf],
                      np.arange(4098, dtype=np.float64)):
            with pytest.raises(_lib.AspError) as err:
                stats.histogram(edges)
            assert err.value.code == -3, edges
        stats.histogram(np.arange(4097, dtype=np.float64))  # 4096 bins are accepted
        bonds = stats.summary["bonds"]
        out = np.zeros(bonds)
        lib = _lib.load()
        assert lib.asp_bonds_magnitudes(stats._handle, ctypes.c_uint64(bonds - 1), _lib.ptr(out)) == -3
        assert b"do not fit" in lib.asp_last_error() and not out.any()
        assert lib.asp_bonds_magnitudes(stats._handle, ctypes.c_uint64(bonds), _lib.ptr(out)) == 0
        assert np.array_equal(out, bond_cases.magnitudes_law(bond_cases.law("k65")))
        _check_summary_and_rows(stats, bond_cases.law("k65"))  # the refusals left the handle intact


@pytest.fixture(scope="module")
def kagome_16(models):
    from annealing_sign_problem_amd import common, operators

    operator = operators.Operator.from_config(models["heisenberg_kagome_16"])
    operator.basis.build()
    _, ground_state = operator.ground_state()
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, operator.basis)
    model = common.make_ising_model(operator.basis.states, operator, log_psi_fn=log_coeff_fn)
    return operator, ground_state, model


def _reference_analysis(exchange, x0, n):
    """common.py:975-1001 and 955-959 of the reference on a scipy matrix."""
    signs = 2.0 * np.unpackbits(np.ascontiguousarray(x0, dtype="<u8").view(np.uint8), bitorder="little")[:n] - 1.0
    matrix = exchange.tocoo()
    keep = (matrix.row != matrix.col) & (matrix.data != 0)  # setdiag(0); eliminate_zeros()
    row, col, data = matrix.row[keep], matrix.col[keep], matrix.data[keep]
    is_frustrated = signs[row] * signs[col] * data > 0
    max_coupling = np.log(np.max(np.abs(data)))
    min_coupling = max(max_coupling - 20, np.log(np.min(np.abs(data))))
    frustrated = np.log(np.abs(data[is_frustrated]))
    frustrated = frustrated[(min_coupling <= frustrated) & (frustrated <= max_coupling)]
    normal = np.log(np.abs(data[np.invert(is_frustrated)]))
    normal = normal[(min_coupling <= normal) & (normal <= max_coupling)]
    bins = np.linspace(min_coupling, max_coupling, 50)
    frustrated_pdf, _ = np.histogram(frustrated, bins=bins, density=False)
    normal_pdf, _ = np.histogram(normal, bins=bins, density=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = normal_pdf / (normal_pdf + frustrated_pdf)
    y[normal_pdf + frustrated_pdf < 100] = float("nan")
    x = np.exp(0.5 * (bins[:-1] + bins[1:]))
    couplings = np.sort(np.abs(data))[::-1]
    return x, y, normal_pdf, frustrated_pdf, couplings, is_frustrated, row, col, data


def test_whole_basis_analyses_equal_the_reference_formulas(kagome_16):
    from annealing_sign_problem_amd import common

    operator, _, model = kagome_16
    assert model.size == 12870
    exchange = model.ising_hamiltonian.exchange
    x, y, normal_pdf, frustrated_pdf, couplings, is_frustrated, _, _, data = _reference_analysis(
        exchange, model.initial_signs, model.size)
    got_x, got_y, normal, frustrated = common.probability_of_frustration(model)
    populated = int(np.count_nonzero(normal_pdf + frustrated_pdf >= 100))
    inside = int(normal_pdf.sum() + frustrated_pdf.sum())
    print("kagome_16: %d bonds, %.4f frustrated, %d below the lower cut, %d of 49 bins hold 100 bonds or more"
          % (data.shape[0], is_frustrated.mean(), data.shape[0] - inside, populated))
    assert np.array_equal(normal, normal_pdf) and np.array_equal(frustrated, frustrated_pdf)
    assert np.array_equal(got_x, x)
    assert np.array_equal(np.isnan(got_y), np.isnan(y)) and np.array_equal(got_y[~np.isnan(y)], y[~np.isnan(y)])
    assert got_y.shape == (49,) and populated >= 40 and 0.0 < is_frustrated.mean() < 0.5
    got = common.coupling_distribution(model)
    assert np.array_equal(got.view(np.uint64), couplings.view(np.uint64))
    # other signs than the model's own: all +1
    ones = np.full_like(model.initial_signs, np.uint64(0xFFFFFFFFFFFFFFFF))
    _, _, normal_pdf, frustrated_pdf, _, _, _, _, _ = _reference_analysis(exchange, ones, model.size)
    _, _, normal, frustrated = common.probability_of_frustration(model, signs=ones)
    assert np.array_equal(normal, normal_pdf) and np.array_equal(frustrated, frustrated_pdf)


def test_cluster_statistics_equal_the_numpy_fractions(kagome_16):
    from annealing_sign_problem_amd import common, synthetic

    operator, ground_state, _ = kagome_16
    start = int(operator.basis.states[np.argmax(np.abs(ground_state))])
    spins = synthetic.grow_cluster(operator, start, 500, seed=3)
    assert spins.shape[0] == 500
    got = common.cluster_statistics(spins, operator, ground_state)
    log_coeff_fn = common.ground_state_to_log_coeff_fn(ground_state, operator.basis)
    model = common.make_ising_model(spins, operator, log_psi_fn=log_coeff_fn)
    _, _, _, _, _, is_frustrated, row, col, data = _reference_analysis(
        model.ising_hamiltonian.exchange, model.initial_signs, model.size)
    # the strongest bond of a row: largest magnitude, smallest column on a tie
    strongest_frustrated = np.zeros(model.size, dtype=bool)
    for i in range(model.size):
        mine = np.flatnonzero(row == i)
        if mine.size:
            top = mine[np.abs(data[mine]) == np.abs(data[mine]).max()]
            strongest_frustrated[i] = is_frustrated[top[np.argmin(col[top])]]
    assert got == {"spins": 500, "bonds": data.shape[0], "frustrated": np.count_nonzero(is_frustrated) / data.shape[0],
                   "largest_frustrated": np.count_nonzero(strongest_frustrated) / 500}
    assert 0 < got["bonds"] and 0.0 < got["frustrated"] < 1.0


def test_driver_writes_what_the_functions_return(kagome_16, tmp_path, capsys):
    from annealing_sign_problem_amd import common, coupling_analysis

    _, _, model = kagome_16
    couplings_file, curve_file = tmp_path / "couplings.csv", tmp_path / "is_frustrated.csv"
    assert coupling_analysis.main(["--model", "heisenberg_kagome_16", "--couplings", str(couplings_file),
                                   "--is-frustrated", str(curve_file)]) == 0
    assert "bonds=%d," % common.coupling_distribution(model).shape[0] in capsys.readouterr().out
    couplings = np.loadtxt(couplings_file)
    assert np.array_equal(couplings, common.coupling_distribution(model))  # (%.18e round-trips a double)
    x, y, _, _ = common.probability_of_frustration(model)
    curve = np.loadtxt(curve_file, delimiter=",", ndmin=2)
    assert curve.shape == (49, 2)
    assert np.array_equal(curve[:, 0], x) and np.array_equal(curve[:, 1], y, equal_nan=True)
