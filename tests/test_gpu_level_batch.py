"""The segmented cutoff and extension on the device (asp_sparsify_component_segments, asp_operator_extend_segments;
csrc/level_segments.hip) against the laws of tests/level_cases.py and against loops of the existing per-cluster calls
— integers equal, doubles as bytes —, and through common.sparsify_models_using_global_cutoff /
extend_and_sparsify_models and sampled_components.stage_clusters(build_batch=True, level_batch=True)."""
import ctypes

import numpy as np
import pytest

import ising_segment_cases as cases
import level_cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _sparsify(t):
    from annealing_sign_problem_amd import common

    return common.sparsify_component_segments(t.offsets, t.indptr, t.indices, t.data, t.frozen, t.reltol, t.anchors)


# -- asp_sparsify_component_segments ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", level_cases.SPARSIFY_NAMES)
def test_every_sparsify_case_is_the_law_and_the_loop(name):
    from annealing_sign_problem_amd import _lib, common

    t = level_cases.sparsify_table(name)
    got = _sparsify(t)
    assert got[0].dtype == bool and got[1].dtype == np.uint64 and got[2].dtype == np.int64
    assert got[3].dtype == np.int32 and got[4].dtype == np.float64
    assert level_cases.same_result(got, t.law()), name
    assert _lib.load().asp_sparsify_last_ms() > 0.0
    # the existing call, segment by segment
    for g, s in enumerate(t.segments):
        keep, ip, col, val = level_cases.rebased(got, t.offsets, g)
        if s.size == 0:
            assert keep.size == 0 and ip.tolist() == [0]
            continue
        want_keep, block = common.sparsify_component(s.matrix, s.frozen, t.reltol, s.anchor)
        assert np.array_equal(keep, want_keep), (name, g)
        assert np.array_equal(ip, block.indptr) and np.array_equal(col, block.indices), (name, g)
        assert val.tobytes() == block.data.tobytes(), (name, g)


def _raw_sparsify(t, capacity, out_indptr, out_indices, out_data, keep=None):
    from annealing_sign_problem_amd import _lib

    total = int(t.offsets[-1])
    keep = np.full(total, 9, dtype=np.uint8) if keep is None else keep
    kept_offsets = np.full(t.offsets.size, 77, dtype=np.uint64)
    frozen = np.ascontiguousarray(t.frozen, dtype=np.uint8)
    nnz = ctypes.c_uint64(991)
    rc = _lib.load().asp_sparsify_component_segments(
        t.offsets.size - 1, _lib.ptr(t.offsets), _lib.ptr(t.indptr), _lib.ptr(t.indices), _lib.ptr(t.data),
        _lib.ptr(frozen), t.reltol, _lib.ptr(t.anchors), _lib.ptr(keep), _lib.ptr(kept_offsets), capacity,
        _lib.ptr(out_indptr), _lib.ptr(out_indices), _lib.ptr(out_data), ctypes.byref(nnz))
    return rc, keep, kept_offsets, int(nnz.value)


@pytest.mark.parametrize("name", ["scaled: hub rows", "sizes 0 1 2 3 63 64 65 257"])
def test_mask_only_call_a_capacity_one_too_small_and_success(name):
    from annealing_sign_problem_amd import _lib

    t = level_cases.sparsify_table(name)
    want = t.law()
    total, rows = want[4].size, int(want[1][-1])
    rc, keep, kept_offsets, nnz = _raw_sparsify(t, 0, None, None, None)
    assert (rc, nnz) == (0, total)
    assert np.array_equal(keep.astype(bool), want[0]) and np.array_equal(kept_offsets, want[1])
    ip, col, val = np.full(rows + 1, -7, dtype=np.int64), np.full(total, -7, dtype=np.int32), np.full(total, 0.5)
    rc, keep, kept_offsets, nnz = _raw_sparsify(t, total - 1, ip, col, val)
    assert (rc, nnz) == (-3, total) and "do not fit capacity" in _lib.last_error()
    assert np.array_equal(kept_offsets, want[1])
    assert np.all(ip == -7) and np.all(col == -7) and np.all(val == 0.5)
    rc, _, _, nnz = _raw_sparsify(t, total, ip, None, val)        # a missing output pointer
    assert (rc, nnz) == (-3, total) and np.all(ip == -7) and np.all(val == 0.5)
    rc, keep, kept_offsets, nnz = _raw_sparsify(t, total, ip, col, val)
    assert (rc, nnz) == (0, total)
    assert level_cases.same_result((keep.astype(bool), kept_offsets, ip, col, val), want)


def test_a_stray_frozen_spin_is_refused_naming_the_first_segment():
    from annealing_sign_problem_amd import _lib

    t = level_cases.sparsify_table(level_cases.STRAY)
    with pytest.raises(level_cases.Stray) as law:
        t.law()
    assert (law.value.segment, law.value.count) == (1, 1)
    capacity = t.data.size
    ip, col, val = (np.full(int(t.offsets[-1]) + 1, -7, dtype=np.int64), np.full(capacity, -7, dtype=np.int32),
                    np.full(capacity, 0.5))
    rc, keep, kept_offsets, nnz = _raw_sparsify(t, capacity, ip, col, val)
    assert rc == -3 and "segment 1: 1 frozen spins are not connected to the anchor" in _lib.last_error()
    assert np.all(keep == 9) and np.all(ip == -7) and np.all(col == -7) and np.all(val == 0.5)
    # the Python surface raises
    with pytest.raises(_lib.AspError, match="segment 1: 1 frozen"):
        _sparsify(t)


# -- asp_operator_extend_segments ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", level_cases.EXTEND_NAMES)
def test_every_extend_case_is_the_law_and_the_loop(name):
    from annealing_sign_problem_amd import _lib

    t = level_cases.extend_table(name)
    device = t.operator.device()
    states, out_offsets = device.extend_segments(t.keys, t.offsets)
    assert states.dtype == np.uint64 and out_offsets.dtype == np.uint64
    assert level_cases.same_extension((states, out_offsets), t.law()), name
    for g in range(t.segments):
        assert np.array_equal(states[int(out_offsets[g]):int(out_offsets[g + 1])], device.extend(t.segment(g))), (name, g)
    # the sizing call, a capacity one too small, a missing output
    want, want_offsets = t.law()

    def call(capacity, out):
        offsets, count = np.full(t.segments + 1, 77, dtype=np.uint64), ctypes.c_uint64(991)
        rc = device._lib.asp_operator_extend_segments(device._handle, t.segments, _lib.ptr(t.offsets), _lib.ptr(t.keys),
                                                      capacity, _lib.ptr(out), _lib.ptr(offsets), ctypes.byref(count))
        return rc, int(count.value), offsets

    rc, count, offsets = call(0, None)
    assert (rc, count) == (0, want.size) and np.array_equal(offsets, want_offsets)
    out = np.full(want.size, 4242, dtype=np.uint64)
    rc, count, offsets = call(want.size - 1, out)
    assert (rc, count) == (-3, want.size) and "do not fit capacity" in _lib.last_error()
    assert np.array_equal(offsets, want_offsets) and np.all(out == 4242)
    rc, count, offsets = call(want.size, None)
    assert (rc, count) == (-3, want.size)
    rc, count, offsets = call(want.size, out)
    assert (rc, count) == (0, want.size) and np.array_equal(out, want) and np.array_equal(offsets, want_offsets)


def test_a_key_above_the_sites_is_refused_before_any_launch():
    from annealing_sign_problem_amd import _lib

    t = level_cases.extend_table("segments of 0 1 2 63 64 65 keys")
    device = t.operator.device()
    keys = t.keys.copy()
    at = int(t.offsets[2]) + 1                       # the second key of segment 2
    keys[at] |= np.uint64(1 << t.operator.basis.number_spins)
    out, offsets, count = (np.full(8, 4242, dtype=np.uint64), np.full(t.segments + 1, 77, dtype=np.uint64),
                           ctypes.c_uint64(991))
    rc = device._lib.asp_operator_extend_segments(device._handle, t.segments, _lib.ptr(t.offsets), _lib.ptr(keys), 8,
                                                  _lib.ptr(out), _lib.ptr(offsets), ctypes.byref(count))
    assert rc == -3 and "key 1 of segment 2 has a bit at or above site 16" in _lib.last_error()
    assert np.all(out == 4242) and np.all(offsets == 77) and count.value == 991
    with pytest.raises(_lib.AspError, match="key 1 of segment 2"):
        device.extend_segments(keys, t.offsets)


def test_a_source_outside_the_sector_is_refused():
    from annealing_sign_problem_amd import _lib
    import symmetry_cases

    e = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    assert e.outside is not None
    keys = np.concatenate([e.keys[:5], [np.uint64(e.outside)], e.keys[5:9]]).astype(np.uint64)
    with pytest.raises(_lib.AspError, match="outside the symmetry sector"):
        e.operator.device().extend_segments(keys, np.array([0, 3, 10], dtype=np.uint64))


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
    """(operator over its built basis, ground state, its log-amplitude closure, 8 grown clusters, cutoff)."""
    from annealing_sign_problem_amd import common
    import eloc_cases

    g = golden("make_ising_kagome16_cluster.npz")
    op, states = eloc_cases.kagome16_basis()
    assert np.array_equal(states, g["basis_states"])
    vector = np.ascontiguousarray(g["ground_state"], dtype=np.float64)
    clusters = [cases.grow(op, size, 200 + size) for size in (1, 2, 7, 12, 20, 33, 64, 90)]
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), clusters, 1e-4


@pytest.fixture(scope="module")
def kagome18_sector():
    """The same for a symmetry-adapted basis (inversion -1), with a random vector as the state."""
    from annealing_sign_problem_amd import common

    op = cases.model_operator("heisenberg_kagome_18", -1)
    op.basis.build()
    rng = np.random.default_rng(18)
    vector = rng.normal(size=op.basis.states.size) * np.exp(0.5 * rng.normal(size=op.basis.states.size))
    clusters = [cases.grow(op, size, 300 + size) for size in (1, 3, 5, 9, 17, 30, 41, 66)]
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), clusters, 1e-3


def _level_loop(models, clusters, log_fn, reltol, field, spare=2):
    """The per-cluster calls of one level; a cluster whose cutoff strands a frozen spin (the per-cluster call
    refuses it) leaves the round — decided by the existing calls alone."""
    from annealing_sign_problem_amd import _lib, common

    kept, extended, want = [], [], []
    for c, m in enumerate(models):
        bigger = common.make_hamiltonian_extension(m, log_fn, **field)
        try:
            cut = common.sparsify_using_global_cutoff(bigger, reltol, clusters[c])
        except _lib.AspError as error:
            assert "not connected to the anchor" in str(error)
            continue
        kept.append(c)
        extended.append(bigger)
        want.append(cut)
    assert len(kept) >= len(models) - spare
    return kept, extended, want


@pytest.mark.parametrize("which", ["kagome16", "kagome18_sector"])
@pytest.mark.parametrize("external_field", [False, True])
def test_the_model_functions_are_their_loops(which, external_field, request):
    from annealing_sign_problem_amd import common

    op, vector, log_fn, clusters, reltol = request.getfixturevalue(which)
    field = {"external_field": True} if external_field else {}
    models = common.make_ising_models(clusters, op, log_psi_fn=log_fn, **field)
    kept, extended, want = _level_loop(models, clusters, log_fn, reltol, field)
    some, frozen = [models[c] for c in kept], [clusters[c] for c in kept]
    _same_models(common.sparsify_models_using_global_cutoff(extended, reltol, frozen), want)
    _same_models(common.extend_and_sparsify_models(some, log_fn, reltol, frozen, **field), want)
    got = common.extension_spins_segments(op, [m.spins for m in some])
    assert all(np.array_equal(a, b.spins) and a.dtype == np.uint64 for a, b in zip(got, extended))
    # a second level grows from the first
    still, _, again = _level_loop(want, frozen, log_fn, reltol, field, spare=len(want))
    _same_models(common.extend_and_sparsify_models([want[c] for c in still], log_fn, reltol, [frozen[c] for c in still],
                                                   **field), again)


@pytest.mark.parametrize("which", ["kagome16", "kagome18_sector"])
def test_the_pipeline_stages_the_same_models_and_results(which, request):
    from annealing_sign_problem_amd import common, sampled_components

    op, vector, log_fn, clusters, reltol = request.getfixturevalue(which)
    models = common.make_ising_models(clusters, op, log_psi_fn=log_fn)
    kept, _, want = _level_loop(models, clusters, log_fn, reltol, {})
    kept = [c for c, ok in zip(kept, _second_level_runs(want, [clusters[c] for c in kept], log_fn, reltol)) if ok][:6]
    some = [clusters[c] for c in kept]
    assert len(some) >= 4
    for greedy_batch in ({}, {"greedy_batch": True}):
        loop = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 2, reltol, **greedy_batch,
                                                 build_batch=True)
        batch = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 2, reltol, **greedy_batch,
                                                  build_batch=True, level_batch=True)
        assert len(batch) == len(loop) == 3 * len(some)
        assert [entry[0] for entry in batch] == [entry[0] for entry in loop]
        _same_models([entry[1] for entry in batch], [entry[1] for entry in loop])
        for a, b in zip(batch, loop):
            assert np.array_equal(a[2], b[2]) and cases.same_bits(a[3], b[3])
            assert a[4].to_csv_str() == b[4].to_csv_str()


def _second_level_runs(models, clusters, log_fn, reltol):
    """Per model: whether the per-cluster calls of the NEXT level accept it too."""
    from annealing_sign_problem_amd import _lib, common

    out = []
    for m, cluster in zip(models, clusters):
        try:
            common.sparsify_using_global_cutoff(common.make_hamiltonian_extension(m, log_fn), reltol, cluster)
            out.append(True)
        except _lib.AspError:
            out.append(False)
    return out
