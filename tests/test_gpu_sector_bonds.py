"""The Ising model of a whole symmetry sector, built on the device from the sector's ELL matrix and a
state vector (asp_sector_bonds_create, BondStatistics.from_sector): the law is restated in
numpy on the downloaded arrays and the handle's statistics must equal it exactly — on the whole sector
of heisenberg_kagome_18 with its ground state, and on two small sectors of tests/sector_cases.py with
vectors that have zeros and both signs.  Against the CSR route on the same basis (make_ising_model +
BondStatistics) the two roundings may differ, so only the number of bonds and the frustration of the
bonds that are not tiny are compared."""
import numpy as np
import pytest

import bond_cases
import sector_cases

pytestmark = pytest.mark.gpu


def sector_law(idx, val, psi):
    """CSR ``(indptr, indices, data)`` of the sector's Ising model, columns ascending.
    H_ij = sum in slot order, from +0.0, of val over the slots of row i with idx == j;
    M_ij = (H_ij |psi_j|) |psi_i|; J_ij = 0.5 (M_ij + M_ji); kept iff J_ij != 0, j != i."""
    width, n = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), width)
    cols = idx.T.astype(np.int64).ravel()     # row i's slots, in slot order
    vals = val.T.ravel()
    key = rows * n + cols
    order = np.argsort(key, kind="stable")    # (slot order survives within a pair)
    key, vals = key[order], vals[order]
    pairs, start, count = np.unique(key, return_index=True, return_counts=True)
    group = np.repeat(np.arange(pairs.shape[0]), count)
    rank = np.arange(key.shape[0]) - start[group]
    h = np.zeros(pairs.shape[0])              # +0.0
    for r in range(int(count.max())):         # one addition per pair and pass: strictly in slot order
        now = rank == r
        h[group[now]] = h[group[now]] + vals[now]
    i, j = pairs // n, pairs % n
    off = i != j
    pairs, i, j, h_ij = pairs[off], i[off], j[off], h[off]
    at = np.searchsorted(pairs, j * n + i)
    found = (at < pairs.shape[0]) & (pairs[np.minimum(at, pairs.shape[0] - 1)] == j * n + i)
    h_ji = np.where(found, h_ij[np.minimum(at, pairs.shape[0] - 1)], 0.0)
    a = np.abs(psi)
    m_ij = (h_ij * a[j]) * a[i]
    m_ji = (h_ji * a[i]) * a[j]
    coupling = 0.5 * (m_ij + m_ji)
    keep = coupling != 0
    indptr = np.concatenate([[0], np.cumsum(np.bincount(i[keep], minlength=n))]).astype(np.int64)
    return indptr, j[keep].astype(np.int32), coupling[keep]


def _sector(operator):
    from annealing_sign_problem_amd import sector_ed

    representatives, norms = sector_ed.enumerate_sector(operator)
    return sector_ed.SectorMatrix(operator, representatives, norms)


def _check(matrix, psi):
    """The handle of (matrix, psi) against the restated law; returns (stats, law's CSR, law)."""
    from annealing_sign_problem_amd.bonds import BondStatistics, log_edges

    idx = matrix.idx.cpu().numpy()
    val = matrix.val.cpu().numpy()
    host_psi = psi.cpu().numpy()
    indptr, indices, data = sector_law(idx, val, host_psi)
    law = bond_cases.bond_law(indptr, indices, data, bond_cases.pack(np.where(host_psi >= 0, 1, -1)))
    assert law["bonds"] > 0 and law["bonds"] == law["stored"]
    stats = BondStatistics.from_sector(matrix, psi)
    summary = stats.summary
    for field in ("num_spins", "stored", "bonds", "frustrated", "rows_with_bonds", "strongest_frustrated"):
        assert summary[field] == law[field], field
    assert summary["max_abs"] == law["max_abs"] and summary["min_abs"] == law["min_abs"]
    strongest, col, frustrated = stats.rows()
    assert np.array_equal(strongest, law["strongest"]) and np.array_equal(col, law["strongest_col"])
    assert np.array_equal(frustrated, law["strongest_frustrated_rows"])
    hi = np.log(law["max_abs"])
    edges = log_edges(max(hi - 20.0, np.log(law["min_abs"])), hi, 50)
    got, want = stats.histogram(edges), bond_cases.histogram_law(law, edges)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    assert got[3] == 0 and int(got[0].sum() + got[1].sum()) + got[2] == law["bonds"]
    assert np.array_equal(stats.magnitudes(), bond_cases.magnitudes_law(law))
    return stats, (indptr, indices, data), law


@pytest.mark.parametrize("name", ["ring12 any magnetisation, field on all bonds",
                                  "ring22 half filling, inversion +1"])
def test_small_sector_equals_the_restated_law(name):
    import torch

    case, = [c for c in sector_cases.SECTOR_CASES if c.name == name]
    matrix = _sector(case.make())
    rng = np.random.default_rng(11)
    psi = rng.standard_normal(matrix.n)
    psi[rng.random(matrix.n) < 0.1] = 0.0  # states without amplitude have no bonds
    psi[1] = -0.0
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
