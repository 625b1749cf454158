"""The Ising model of a whole symmetry sector, built on the device from the sector's ELL matrix and a
state vector (asp_sector_bonds_create, BondStatistics.from_sector): the law is restated in
numpy (tests/sector_bond_cases.py) and the handle's statistics must equal it exactly — on the whole sector
of heisenberg_kagome_18 with its ground state, on two small sectors of tests/sector_cases.py with
vectors that have zeros and both signs, and on the synthetic ELL inputs of tests/sector_bond_cases.py,
which reach the sizes, slot patterns and roundings that no real operator gives
(tests/test_sector_bond_cases.py shows which wrong reading of the law each of them would catch).  Against
the CSR route on the same basis (make_ising_model + BondStatistics) the two roundings may differ, so only
the number of bonds and the frustration of the bonds that are not tiny are compared."""
import numpy as np
import pytest

import bond_cases
import sector_bond_cases
import sector_cases
from sector_bond_cases import sector_law

pytestmark = pytest.mark.gpu

SUMMARY = ("num_spins", "stored", "bonds", "frustrated", "rows_with_bonds", "strongest_frustrated")


def _sector(operator):
    from annealing_sign_problem_amd import sector_ed

    representatives, norms = sector_ed.enumerate_sector(operator)
    return sector_ed.SectorMatrix(operator, representatives, norms)


def _check(matrix, psi, may_be_empty=False):
    """The handle of (matrix, psi) against the restated law; returns (stats, law's CSR, law)."""
    from annealing_sign_problem_amd.bonds import BondStatistics, log_edges

    idx = matrix.idx.cpu().numpy()
    val = matrix.val.cpu().numpy()
    host_psi = psi.cpu().numpy()
    indptr, indices, data = sector_law(idx, val, host_psi)
    law = bond_cases.bond_law(indptr, indices, data, bond_cases.pack(np.where(host_psi >= 0, 1, -1)))
    assert (may_be_empty or law["bonds"] > 0) and law["bonds"] == law["stored"]
    stats = BondStatistics.from_sector(matrix, psi)
    _equals(stats, law)
    if law["bonds"] == 0:
        return stats, (indptr, indices, data), law
    edges = sector_bond_cases.histogram_edges(law, log_edges)
    got, want = stats.histogram(edges), bond_cases.histogram_law(law, edges)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    assert got[3] == 0 and int(got[0].sum() + got[1].sum()) + got[2] == law["bonds"]
    return stats, (indptr, indices, data), law


def _equals(stats, law):
    """Summary, rows() and magnitudes() of the handle against a bond_cases.bond_law result."""
    summary = stats.summary
    for field in SUMMARY:
        assert summary[field] == law[field], field
    assert summary["max_abs"] == law["max_abs"] and summary["min_abs"] == law["min_abs"]
    strongest, col, frustrated = stats.rows()
    assert np.array_equal(strongest, law["strongest"]) and np.array_equal(col, law["strongest_col"])
    assert np.array_equal(frustrated, law["strongest_frustrated_rows"])
    assert np.array_equal(stats.magnitudes(), bond_cases.magnitudes_law(law))


class _Ell:
    """What from_sector reads of a sector_ed.SectorMatrix: n, width and the two device arrays."""

    def __init__(self, idx, val):
        import torch

        self.width, self.n = idx.shape
        self.idx = torch.tensor(idx.view(np.int32), device="cuda")  # (the device array holds the u32 as i32)
        self.val = torch.tensor(val, device="cuda")


def _upload(name):
    import torch

    idx, val, psi = sector_bond_cases.CASES[name]
    return _Ell(idx, val), torch.tensor(psi, device="cuda")


def _same_bits(tensor, array):
    host = tensor.cpu().numpy()
    return host.shape == array.shape and host.tobytes() == array.tobytes()


@pytest.mark.parametrize("name", list(sector_bond_cases.CASES))
def test_synthetic_case_equals_the_restated_law(name):
    idx, val, psi = sector_bond_cases.CASES[name]
    matrix, device_psi = _upload(name)
    n = psi.shape[0]
    stats, (indptr, indices, data), law = _check(matrix, device_psi, may_be_empty=True)
    with stats:
        assert law["stored"] == sector_bond_cases.law(name)[0][-1] == stats.summary["stored"]
        # the inputs are only read
        assert _same_bits(matrix.idx, idx.view(np.int32)) and _same_bits(matrix.val, val)
        assert _same_bits(device_psi, psi)
        # other signs on the device-built matrix: all plus, a bond is frustrated iff its coupling is positive
        first = stats.summary
        rows = stats.rows()
        plus = bond_cases.bond_law(indptr, indices, data, bond_cases.pack(np.ones(n)))
        assert plus["frustrated"] == np.count_nonzero(data > 0)
        assert stats.set_signs(bond_cases.pack(np.ones(n))) is stats
        assert stats.summary["frustrated"] == np.count_nonzero(data > 0)
        _equals(stats, plus)
        stats.set_signs(bond_cases.pack(sector_bond_cases.sector_signs(psi)))  # and back
        assert stats.summary == first
        assert all(np.array_equal(a, b) for a, b in zip(stats.rows(), rows))
        _equals(stats, law)


def _coupled_slot(idx, val, psi):
    """(slot, row) of a used slot with a value whose two states both have an amplitude."""
    width, n = idx.shape
    for i in range(n):
        for k in range(width):
            j = int(idx[k, i])
            if j != i and val[k, i] != 0 and psi[i] != 0 and psi[j] != 0:
                return k, i
    raise AssertionError("no coupled slot")


def test_non_finite_input_is_refused_and_the_repaired_input_is_not():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd.bonds import BondStatistics

    idx, val, psi = sector_bond_cases.CASES["n65"]
    slot, state = _coupled_slot(idx, val, psi)
    matrix, device_psi = _upload("n65")
    for where, bad in (("psi", np.nan), ("psi", np.inf), ("psi", -np.inf), ("val", np.nan)):
        target = device_psi if where == "psi" else matrix.val
        at = (state,) if where == "psi" else (slot, state)
        good = target[at].item()
        target[at] = bad
        with pytest.raises(_lib.AspError) as err:
            BondStatistics.from_sector(matrix, device_psi)
        assert err.value.code == -3 and "not finite" in str(err.value), (where, bad)  # ASP_ERR_INVALID
        target[at] = good
        assert _same_bits(device_psi, psi) and _same_bits(matrix.val, val)
        stats, _, _ = _check(matrix, device_psi)  # the same inputs, repaired: the law again
        stats.release()


def test_from_sector_checks_its_state_vector():
    import torch

    from annealing_sign_problem_amd.bonds import BondStatistics

    idx, val, psi = sector_bond_cases.CASES["n65"]
    matrix, device_psi = _upload("n65")
    strided = torch.tensor(np.repeat(psi, 2), device="cuda")[::2]
    assert strided.shape == device_psi.shape and torch.equal(strided, device_psi) and not strided.is_contiguous()
    for bad in (device_psi.to(torch.float32), device_psi.cpu(), strided, device_psi[:64],
                torch.cat([device_psi, device_psi[:1]]), device_psi.reshape(1, -1)):
        with pytest.raises(ValueError):
            BondStatistics.from_sector(matrix, bad)
    stats, _, _ = _check(matrix, device_psi)
    stats.release()


@pytest.mark.parametrize("name", ["ring12 any magnetisation, field on all bonds",
                                  "ring22 half filling, inversion +1"])
def test_small_sector_equals_the_restated_law(name):
    import torch

    case, = [c for c in sector_cases.SECTOR_CASES if c.name == name]
    matrix = _sector(case.make())
    rng = np.random.default_rng(11)
    psi = rng.standard_normal(matrix.n)
    psi[rng.random(matrix.n) < 0.1] = 0.0  # states without amplitude have no bonds
    psi /= np.linalg.norm(psi)
    idx = matrix.idx.cpu().numpy()
    # the duplicate-keeping law is exercised: some row reaches one target through several slots
    own = np.arange(matrix.n)
    assert any(np.unique(idx[:, i][idx[:, i] != own[i]]).shape[0] < np.count_nonzero(idx[:, i] != own[i])
               for i in range(matrix.n))
    stats, _, law = _check(matrix, torch.from_numpy(psi).cuda())
    stats.release()
    assert 0.1 < law["frustrated"] / law["bonds"] < 0.9


def test_kagome_18_sector_equals_the_law_and_the_csr_route(models):
    from annealing_sign_problem_amd import common, operators, sector_ed
    from annealing_sign_problem_amd.bonds import BondStatistics

    operator = operators.Operator.from_config(models["heisenberg_kagome_18"])
    matrix = _sector(operator)
    assert matrix.n == 24310
    _, psi, _ = sector_ed.lanczos_ground_state(matrix, tol=1e-10, max_iterations=200)
    stats, (indptr, indices, data), law = _check(matrix, psi)
    with stats:
        host_psi = psi.cpu().numpy()
        operator.basis.build()
        log_coeff_fn = common.ground_state_to_log_coeff_fn(host_psi, operator.basis)
        model = common.make_ising_model(operator.basis.states, operator, log_psi_fn=log_coeff_fn)
        with BondStatistics(model.ising_hamiltonian, model.initial_signs) as other:
            theirs = other.summary
        mine = stats.summary
        assert mine["bonds"] == theirs["bonds"]
        # frustration may differ only where |J| < 1e-12 max|J|: the two routes round differently
        threshold = 1e-12 * law["max_abs"]
        exchange = model.ising_hamiltonian.exchange
        n = matrix.n
        csr_law = bond_cases.bond_law(exchange.indptr, exchange.indices, exchange.data, model.initial_signs)
        coo = exchange.tocoo()
        keep = (coo.row != coo.col) & (coo.data != 0)
        their_key = coo.row[keep].astype(np.int64) * n + coo.col[keep]
        my_key = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) * n + indices
        strong = law["magnitude"] >= threshold
        at = np.minimum(np.searchsorted(their_key, my_key[strong]), their_key.shape[0] - 1)
        assert np.array_equal(their_key[at], my_key[strong])
        assert np.array_equal(csr_law["is_frustrated"][at], law["is_frustrated"][strong])
        weak = int(np.count_nonzero(~strong))
        print("kagome_18 sector: %d bonds, frustrated %d (sector route) and %d (CSR route), %d bonds below 1e-12 max|J|"
              % (mine["bonds"], mine["frustrated"], theirs["frustrated"], weak))
        assert abs(mine["frustrated"] - theirs["frustrated"]) <= weak
