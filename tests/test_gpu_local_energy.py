"""The local energies on the device (asp_operator_local_energy: k_segment_insert, k_eloc_rows, k_eloc_list;
csrc/operator_local_energy.hip) against the sequential law of tests/eloc_cases.py, bit for bit, and through
common.local_energies / variational_energy and local_energy.sample_local_energies.  Quality is asserted nowhere."""
import itertools

import numpy as np
import pytest

import eloc_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _device(t, phi=None, rows=None):
    return t.operator.device().local_energy(t.keys, t.phi if phi is None else phi, t.offsets,
                                            t.rows if rows is None else rows)


def _equals_law(got, want):
    hphi, eloc, missing = got
    assert missing.dtype == np.uint32 and np.array_equal(missing, want[2])
    assert cases.same_bits(hphi, want[0])
    assert cases.same_bits(eloc, want[1])


# -- bond counts, table sizes, segments, bases -----------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_is_the_law_bit_for_bit(name):
    """k_eloc_rows for the plain bases (24, 64, 65 and 120 bonds; a row of 65 found connections over two chunks;
    one segment of 1 ... 4097 keys; 4097 segments of 1-3 keys; empty segments first, in the middle and last; one
    state in 300 segments; keys with bit 63), k_eloc_list for the symmetry-adapted bases (norm-0 targets) and
    single-site flips (a state reached twice)."""
    t = cases.table(name)
    device = t.operator.device()
    assert device.unique_targets == (name in cases.PLAIN)
    _equals_law(_device(t), t.law())
    assert device.last_ms > 0.0


def test_offsets_and_rows_default_to_one_segment_and_every_entry():
    t = cases.table("kagome16 K=65")
    got = t.operator.device().local_energy(t.keys, t.phi)
    _equals_law(got, t.law())
    assert got[0].shape == (65,)


@pytest.mark.parametrize("name", ["three segments", "kagome18 inversion -1"])
def test_rows_repeated_permuted_and_absent(name):
    t = cases.table(name)
    rng = np.random.default_rng(5)
    base = t.rows
    some = [rng.permutation(base),                               # any order
            np.repeat(base[:: max(1, base.size // 9)], 3),        # repeats
            base[t.row_segments != 1],                            # no row in the middle segment
            base[-1:], base[:1]]
    some.append(np.concatenate([some[1], some[0]]))
    for rows in some:
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        _equals_law(_device(t, rows=rows), t.law(rows=rows))


def test_no_rows_and_null_outputs_in_every_combination():
    from annealing_sign_problem_amd import _lib

    t = cases.table("empty segments")
    device = t.operator.device()
    hphi, eloc, missing = device.local_energy(t.keys, t.phi, t.offsets, np.zeros(0, dtype=np.uint64))
    assert hphi.shape == eloc.shape == missing.shape == (0,)
    want = t.law()
    n = t.rows.size
    for with_hphi, with_eloc, with_missing in itertools.product((False, True), repeat=3):
        hphi, eloc, missing = np.full(n, np.nan), np.full(n, np.nan), np.full(n, 77, dtype=np.uint32)
        _lib.check(device._lib.asp_operator_local_energy(
            device._handle, t.offsets.size - 1, _lib.ptr(t.offsets), _lib.ptr(t.keys), _lib.ptr(t.phi), n,
            _lib.ptr(t.rows), _lib.ptr(hphi) if with_hphi else None, _lib.ptr(eloc) if with_eloc else None,
            _lib.ptr(missing) if with_missing else None))
        assert cases.same_bits(hphi, want[0]) if with_hphi else np.isnan(hphi).all()
        assert cases.same_bits(eloc, want[1]) if with_eloc else np.isnan(eloc).all()
        assert np.array_equal(missing, want[2]) if with_missing else np.all(missing == 77)


@pytest.mark.parametrize("name", ["three segments", "sk16 one row of 65 connections", "ring20 all-to-all, inversion -1"])
def test_signed_zeros_and_subnormals_at_the_targets(name):
    """-0.0, 0.0 and subnormals of both signs everywhere but at the rows: products that vanish or are subnormal
    on the way, a sum that starts at +0.0 and stays there through -0.0 terms."""
    t = cases.table(name)
    rows = t.rows[::7] if t.rows.size > 7 else t.rows
    phi = cases.awkward_amplitudes(t.keys.size)
    phi[rows.astype(np.int64)] = t.phi[rows.astype(np.int64)]
    got = _device(t, phi=phi, rows=rows)
    _equals_law(got, t.law(phi=phi, rows=rows))
    # a zero away from the rows is legal; at a row only without eloc
    from annealing_sign_problem_amd import _lib

    zero = t.phi.copy()
    zero[int(rows[0])] = -0.0
    with pytest.raises(_lib.AspError, match="row 0 has a zero") as error:
        _device(t, phi=zero, rows=rows)
    assert error.value.code == -3
    hphi, eloc, missing = t.operator.device()._local_energy(t.keys, zero, t.offsets, rows, False)
    want = t.law(phi=zero, rows=rows)
    assert eloc is None and cases.same_bits(hphi, want[0]) and np.array_equal(missing, want[2])


@pytest.mark.parametrize("name", ["three segments", "one state in 300 segments", "4097 segments of 1-3 keys",
                                  "ring22 inversion -1", "single-site flips"])
def test_flipping_segments_on_the_device(name):
    """Negating phi over whole segments leaves eloc bit for bit and negates hphi bit for bit (a sum that is exactly
    zero stays +0.0: eloc_cases.flip_holds)."""
    t = cases.table(name)
    hphi, eloc, missing = _device(t)
    chosen = sorted(set(t.row_segments.tolist()))[::2]
    f_hphi, f_eloc, f_missing = _device(t, phi=cases.flipped(t, chosen))
    sign = np.where(np.isin(t.row_segments, chosen), -1.0, 1.0)
    assert cases.flip_holds(hphi, eloc, f_hphi, f_eloc, sign)
    assert np.array_equal(f_missing, missing) and np.count_nonzero(sign < 0) > 0


def test_a_row_key_outside_the_sector_is_refused():
    from annealing_sign_problem_amd import _lib
    import symmetry_cases

    expected = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    assert expected.outside is not None
    keys = np.union1d(expected.keys, np.array([expected.outside], dtype=np.uint64))
    at = int(np.searchsorted(keys, np.uint64(expected.outside)))
    device = expected.operator.device()
    with pytest.raises(_lib.AspError, match="outside the symmetry sector") as error:
        device.local_energy(keys, np.ones(keys.size), None, np.array([0, at], dtype=np.uint64))
    assert error.value.code == -3
    # in the table, but no row: never looked at
    rows = np.array([i for i in range(keys.size) if i != at], dtype=np.uint64)
    got = device.local_energy(keys, np.ones(keys.size), None, rows)
    _equals_law(got, cases.eloc_law(expected.operator, keys, np.ones(keys.size), None, rows))


# -- full basis ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kagome16():
    """(operator over its built basis, ground state, E0 from the host)."""
    g = golden("make_ising_kagome16_cluster.npz")
    op, states = cases.kagome16_basis()
    assert np.array_equal(states, g["basis_states"])
    vector = np.ascontiguousarray(g["ground_state"], dtype=np.float64)
    energy = op.expectation(vector)
    assert energy.imag == 0.0
    return op, vector, float(energy.real)


def test_full_basis_with_the_ground_state(kagome16):
    """`missing = 0` everywhere; the Rayleigh quotient is Operator.expectation to the bound of
    tests/test_eloc_cases.py; and `|eloc_r - E0| <= (|(H psi - E0 psi)_r| + bound_r) / |psi_r|` with the residual
    computed here on the host: eloc_r - E0 = (hphi_r - E0 psi_r) / psi_r, hphi_r is within bound_r of the exact
    row — the law spends at most half of `n_r 2^-52 sum|terms|`, which leaves the other half for the host's own
    product, the rounding of E0 psi_r (one of the terms' size) and the quotient."""
    from annealing_sign_problem_amd import common

    op, psi, e0 = kagome16
    states = op.basis.states
    hphi, eloc, missing = common.local_energies(op, states, psi)
    assert not missing.any() and missing.shape == states.shape
    _, _, _, count, magnitude = cases.eloc_law(op, states, psi, with_terms=True)
    bound = cases.derived_bound(count, magnitude)
    energy, lost = common.variational_energy(op, states, psi)
    assert lost == 0
    assert abs(energy - e0) <= cases.rayleigh_bound(psi, hphi, count, magnitude)
    residual = op.to_sparse().real.T @ psi - e0 * psi
    assert np.all(psi != 0)
    assert np.all(np.abs(eloc - e0) <= (np.abs(residual) + bound) / np.abs(psi))
    # an eigenvector: hphi = E0 psi up to the residual
    assert np.all(np.abs(hphi - e0 * psi) <= np.abs(residual) + bound)
    # rows= picks entries of the same table
    rows = np.array([5, 5, 12869, 0], dtype=np.uint64)
    part = common.local_energies(op, states, psi, rows=rows)
    assert cases.same_bits(part[1], eloc[rows.astype(np.int64)])


# -- the driver ------------------------------------------------------------------------------------------------
def _samples(op, vector, number, seed):
    rng = np.random.default_rng(seed)
    p = vector ** 2
    return op.basis.states[rng.choice(vector.size, size=number, replace=True, p=p / p.sum())]


def test_exact_signs_give_the_ground_state_energy_on_every_sample(kagome16):
    """With the exact signs the cluster's amplitudes ARE the ground state's on the sample's whole neighbourhood,
    so every E_loc is E0 within the bound of the full-basis test."""
    from annealing_sign_problem_amd import common, local_energy

    op, psi, e0 = kagome16
    samples = _samples(op, psi, 32, 1)
    log_fn = common.ground_state_to_log_coeff_fn(psi, op.basis)
    results = local_energy.sample_local_energies(op, psi, samples, log_fn, order=0, global_cutoff=1e-6, signs="exact")
    states, counts = np.unique(samples, return_counts=True)
    assert [r[0] for r in results] == states.tolist() and [r[4] for r in results] == counts.tolist()
    assert sum(r[4] for r in results) == 32 and all(r[3] == 0 for r in results)
    where = np.searchsorted(op.basis.states, states)
    _, _, _, count, magnitude = cases.eloc_law(op, op.basis.states, psi, rows=where, with_terms=True)
    residual = (op.to_sparse().real.T @ psi - e0 * psi)[where]
    bound = cases.derived_bound(count, magnitude)
    energies = np.array([r[2] for r in results])
    assert np.all(np.abs(energies - e0) <= (np.abs(residual) + bound) / np.abs(psi[where]))
    assert [r[1] for r in results] == count.tolist()  # the cluster is the neighbourhood: every connection found


def test_greedy_signs_equal_the_closed_calls_composed_by_hand(kagome16):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common, local_energy

    op, psi, _ = kagome16
    samples = _samples(op, psi, 12, 2)
    log_fn = common.ground_state_to_log_coeff_fn(psi, op.basis)

    def run():
        return local_energy.sample_local_energies(op, psi, samples, log_fn, order=1, global_cutoff=1e-4,
                                                  signs="greedy", seed=99)

    first, second = run(), run()
    assert first == second
    by_hand = []
    for state, count in zip(*np.unique(samples, return_counts=True)):
        cluster = common.extension_spins(op, np.array([state], dtype=np.uint64))
        model = common.make_ising_model(cluster, op, log_psi_fn=log_fn)
        model = common.sparsify_using_global_cutoff(common.make_hamiltonian_extension(model, log_fn), 1e-4, cluster)
        x = common.solve_ising_model(model, mode="greedy", frozen_spins=cluster)
        phi = np.exp(log_fn(cluster).real) * sa.bits_to_signs(x, count=cluster.size)
        at = np.searchsorted(cluster, state)
        _, eloc, missing = op.device().local_energy(cluster, phi, None, np.array([at], dtype=np.uint64))
        by_hand.append((int(state), int(cluster.size), float(eloc[0]), int(missing[0]), int(count)))
    assert first == by_hand
    assert all(np.isfinite(r[2]) and r[3] == 0 for r in first)
    with_field = local_energy.sample_local_energies(op, psi, samples, log_fn, order=1, global_cutoff=1e-4,
                                                    signs="greedy", external_field=True)
    assert [r[:2] for r in with_field] == [r[:2] for r in first] and all(np.isfinite(r[2]) for r in with_field)
