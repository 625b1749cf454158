"""The segmented coupling build on the device (asp_operator_ising_segments: k_row_segments, k_ising_rows_seg,
k_merge_rows_seg, k_sym_rows_seg; csrc/operator_ising_segments.hip) against the law of tests/ising_segment_cases.py
and against a loop of the existing ising_csr over the segments — indices equal, values as bits —, and through
common.make_ising_models / make_hamiltonian_extensions and sampled_components.stage_clusters(build_batch=True)."""
import ctypes

import numpy as np
import pytest

import ising_segment_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _device(c, psi=None):
    return c.operator.device().ising_csr_segments(c.keys, c.psi if psi is None else psi, c.offsets)


def _loop(c, psi=None):
    """The existing call, segment by segment."""
    psi = c.psi if psi is None else psi
    device = c.operator.device()
    offsets = c.offsets.astype(np.int64)
    parts = [device.ising_csr(c.keys[offsets[g]:offsets[g + 1]], psi[offsets[g]:offsets[g + 1]])
             for g in range(c.segments)]
    return cases.concatenate(parts, np.diff(offsets))


def _exact(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert cases.same_bits(got[2], want[2])


# -- segment sizes, segment layouts, bond counts, key edges, both variants ---------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_is_the_law_and_the_loop_bit_for_bit(name):
    """k_ising_rows_seg for the plain bases (segments of 1, 2, 3, 5, 63, 64, 65, 301 and 4097 keys; boundaries inside
    a workgroup; 4097 segments of 1-3 keys; empty segments first, in the middle and last; one state in 300 segments;
    overlapping segments; 24, 64, 65 and 120 bonds; a row of 65 found connections; keys with bit 63; ring4's full
    basis; one-directional matrix elements), k_merge_rows_seg / k_sym_rows_seg for the symmetry-adapted bases (norm-0
    targets) and single-site flips (a state reached twice)."""
    c = cases.case(name)
    device = c.operator.device()
    assert device.unique_targets == (name in cases.PLAIN)
    got = _device(c)
    _exact(got, c.law())
    assert device.last_ms > 0.0
    _exact(got, _loop(c))


@pytest.mark.parametrize("name", ["three segments", "sk16 one row of 65 connections", "segments of 2 3 5",
                                  "ring20 all-to-all, inversion -1", "kagome18 inversion -1", "single-site flips"])
def test_signed_zeros_and_subnormals_over_whole_segments(name):
    """-0.0, 0.0, subnormals of both signs and ordinary values in turn, not normalised: products that vanish or are
    subnormal on the way; an entry is present or pruned exactly as the law says."""
    c = cases.case(name)
    psi = cases.awkward_amplitudes(c.keys.size)
    want = c.law(psi=psi)
    got = _device(c, psi=psi)
    _exact(got, want)
    _exact(got, _loop(c, psi=psi))
    assert 0 < want[2].size and np.count_nonzero(np.diff(want[0]) == 0) > 0  # kept entries and emptied rows


def test_rows_longer_than_max_connections():
    """m[dst][src] != 0 == m[src][dst] in the plain variant: the row of the state 0 holds 22 couplings where
    max_connections is 8, so the first capacity of the wrapper is too small and it repeats the call."""
    c = cases.case("one-directional, wide rows")
    device = c.operator.device()
    assert device.unique_targets and device.max_connections == 1 + cases.WIDE_BONDS
    got = _device(c)
    assert np.diff(got[0])[0] == 1 + 3 * cases.WIDE_BONDS > device.max_connections
    _exact(got, c.law())
    # a table of that one row: more couplings than the first capacity T * max_connections
    near = c.keys[:int(c.offsets[1])]
    keys = np.concatenate([near, near])
    psi = np.concatenate([c.psi[:near.size], c.psi[:near.size]])
    offsets = np.array([0, near.size, 2 * near.size], dtype=np.uint64)
    twice = device.ising_csr_segments(keys, psi, offsets)
    _exact(twice, cases.ising_segments_law(c.operator, keys, psi, offsets))


def test_one_directional_elements_with_duplicates_are_refused_naming_the_segment():
    from annealing_sign_problem_amd import _lib

    c = cases.case(cases.ONE_WAY_WITH_DUPLICATES)
    device = c.operator.device()
    assert not device.unique_targets
    with pytest.raises(_lib.AspError, match="no mirror element") as error:
        _device(c)
    assert error.value.code == -3 and "the first in segment 2" in str(error.value)
    with pytest.raises(_lib.AspError, match="no mirror element"):  # as the existing call for that cluster
        device.ising_csr(c.keys[1:], c.psi[1:])
    # the single key and the empty segment alone are fine
    offsets = np.array([0, 1, 1], dtype=np.uint64)
    _exact(device.ising_csr_segments(c.keys[:1], c.psi[:1], offsets),
           cases.ising_segments_law(c.operator, c.keys[:1], c.psi[:1], offsets))


def test_a_segment_holding_a_key_outside_the_sector_is_refused():
    from annealing_sign_problem_amd import _lib
    import symmetry_cases

    expected = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    assert expected.outside is not None
    bad = np.union1d(expected.keys, np.array([expected.outside], dtype=np.uint64))
    device = expected.operator.device()
    keys = np.concatenate([expected.keys, bad])
    offsets = np.array([0, expected.keys.size, keys.size], dtype=np.uint64)
    with pytest.raises(_lib.AspError, match="outside the symmetry sector") as error:
        device.ising_csr_segments(keys, np.ones(keys.size), offsets)
    assert error.value.code == -3
    with pytest.raises(_lib.AspError, match="outside the symmetry sector"):  # the existing message
        device.ising_csr(bad, np.ones(bad.size))
    good = np.array([0, expected.keys.size], dtype=np.uint64)
    psi = np.ones(expected.keys.size)
    _exact(device.ising_csr_segments(expected.keys, psi, good),
           cases.ising_segments_law(expected.operator, expected.keys, psi, good))


@pytest.mark.parametrize("name", ["three segments", "kagome18 inversion +1"])
def test_sizing_call_a_capacity_one_too_small_and_success(name):
    from annealing_sign_problem_amd import _lib

    c = cases.case(name)
    device = c.operator.device()
    want = c.law()
    total, rows = want[2].size, c.keys.size

    def call(capacity, indptr, col, val):
        nnz = ctypes.c_uint64(0)
        rc = device._lib.asp_operator_ising_segments(
            device._handle, c.segments, _lib.ptr(c.offsets), _lib.ptr(c.keys), _lib.ptr(c.psi), capacity,
            _lib.ptr(indptr), _lib.ptr(col), _lib.ptr(val), ctypes.byref(nnz))
        return rc, int(nnz.value)

    assert call(0, None, None, None) == (0, total)
    indptr, col, val = np.full(rows + 1, -7, dtype=np.int64), np.full(total, -7, dtype=np.int32), np.full(total, 0.5)
    assert call(total - 1, indptr, col, val) == (-3, total)
    assert "do not fit capacity" in _lib.last_error()
    assert np.all(indptr == -7) and np.all(col == -7) and np.all(val == 0.5)
    assert call(total, indptr, None, val) == (-3, total)  # a missing output pointer
    assert np.all(indptr == -7) and np.all(val == 0.5)
    assert call(total, indptr, col, val) == (0, total)
    _exact((indptr, col, val), want)


# -- the Python surface ----------------------------------------------------------------------------------------
def _same_models(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.spins.dtype == b.spins.dtype and np.array_equal(a.spins, b.spins)
        x, y = a.ising_hamiltonian.exchange, b.ising_hamiltonian.exchange
        assert x.shape == y.shape and x.indptr.dtype == y.indptr.dtype and x.indices.dtype == y.indices.dtype
        assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
        assert cases.same_bits(x.data, y.data)
        assert cases.same_bits(a.ising_hamiltonian.field, b.ising_hamiltonian.field)
        assert np.array_equal(a.initial_signs, b.initial_signs)
        assert (a.basis_index is None) == (b.basis_index is None)
        assert a.basis_index is None or np.array_equal(a.basis_index, b.basis_index)
        assert a.quantum_hamiltonian is b.quantum_hamiltonian


@pytest.fixture(scope="module")
def kagome16():
    """(operator over its built basis, ground state, its log-amplitude closure, 8 grown clusters)."""
    from annealing_sign_problem_amd import common
    import eloc_cases

    g = golden("make_ising_kagome16_cluster.npz")
    op, states = eloc_cases.kagome16_basis()
    assert np.array_equal(states, g["basis_states"])
    vector = np.ascontiguousarray(g["ground_state"], dtype=np.float64)
    clusters = [cases.grow(op, size, 200 + size) for size in (1, 2, 7, 12, 20, 33, 64, 90)]
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), clusters


@pytest.fixture(scope="module")
def kagome18_sector():
    """The same for a symmetry-adapted basis (inversion -1), with a random vector as the state."""
    from annealing_sign_problem_amd import common

    op = cases.model_operator("heisenberg_kagome_18", -1)
    op.basis.build()
    rng = np.random.default_rng(18)
    vector = rng.normal(size=op.basis.states.size) * np.exp(rng.normal(size=op.basis.states.size))
    clusters = [cases.grow(op, size, 300 + size) for size in (1, 3, 5, 9, 17, 30, 41, 66)]
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), clusters


@pytest.mark.parametrize("which", ["kagome16", "kagome18_sector"])
@pytest.mark.parametrize("external_field", [False, True])
def test_make_ising_models_is_the_loop_of_make_ising_model(which, external_field, request):
    from annealing_sign_problem_amd import common

    op, vector, log_fn, clusters = request.getfixturevalue(which)
    assert op.device().unique_targets == (which == "kagome16")
    field = {"external_field": True} if external_field else {}
    want = [common.make_ising_model(c, op, log_psi_fn=log_fn, **field) for c in clusters]
    _same_models(common.make_ising_models(clusters, op, log_psi_fn=log_fn, **field), want)
    assert all(np.count_nonzero(m.ising_hamiltonian.field) > 0 for m in want[3:]) == external_field
    if not external_field:
        # given log-amplitudes instead of the closure
        given = common.make_ising_models(clusters, op, log_psis=[log_fn(c) for c in clusters])
        for m in want:
            m.basis_index = None  # (nothing was looked up)
        _same_models(given, want)


def test_make_hamiltonian_extensions_is_the_loop(kagome16):
    from annealing_sign_problem_amd import common

    op, vector, log_fn, clusters = kagome16
    models = common.make_ising_models(clusters[:6], op, log_psi_fn=log_fn)
    for field in ({}, {"external_field": True}):
        want = [common.make_hamiltonian_extension(m, log_fn, **field) for m in models]
        _same_models(common.make_hamiltonian_extensions(models, log_fn, **field), want)
        assert all(w.size > m.size for w, m in zip(want, models))


def test_the_pipeline_stages_the_same_models_and_results(kagome16):
    from annealing_sign_problem_amd import sampled_components

    op, vector, log_fn, clusters = kagome16
    some = clusters[1:7]
    for greedy_batch in ({}, {"greedy_batch": True}):
        loop = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 2, 1e-4, **greedy_batch)
        batch = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 2, 1e-4, **greedy_batch,
                                                  build_batch=True)
        assert len(batch) == len(loop) == 3 * len(some)
        assert [entry[0] for entry in batch] == [entry[0] for entry in loop]
        _same_models([entry[1] for entry in batch], [entry[1] for entry in loop])
        for a, b in zip(batch, loop):
            assert np.array_equal(a[2], b[2]) and cases.same_bits(a[3], b[3])
            assert a[4].to_csv_str() == b[4].to_csv_str()
