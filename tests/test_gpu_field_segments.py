"""The segmented boundary field on the device (asp_operator_field_segments: k_segment_insert, k_field_rows_seg,
k_field_list_seg; csrc/operator_field_segments.hip) against the law of tests/field_segment_cases.py and the loop of
DeviceOperator.field, bit for bit, and through make_ising_models, make_hamiltonian_extensions,
extend_and_sparsify_models, reweight_ising_models and stage_clusters with external_field=True."""
import numpy as np
import pytest

import field_segment_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _device(c, scale):
    return c.operator.device().field_segments(c.keys, c.psi, c.offsets, c.env_keys, c.env_psi, c.env_offsets,
                                              scale=scale)


def _loop(c, scale):
    """DeviceOperator.field, segment by segment."""
    device = c.operator.device()
    field = np.zeros(c.keys.size)
    unresolved = np.zeros(c.segments, dtype=np.uint64)
    for g in range(c.segments):
        keys, psi, env_keys, env_psi = c.segment(g)
        lo = int(c.offsets[g])
        field[lo:lo + keys.size], unresolved[g] = device.field(keys, psi, env_keys, env_psi, scale=scale)
    return field, unresolved


# -- the law -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_at_every_scale_is_the_law_and_the_loop(name):
    c = cases.case(name)
    assert c.operator.device().unique_targets == (name in cases.PLAIN)
    for scale in cases.SCALES:
        got = _device(c, scale)
        assert got[0].shape == c.keys.shape and got[1].shape == (c.segments,) and got[1].dtype == np.uint64
        assert cases.equal(got, c.law(scale)), scale
        if c.segments <= 10 or scale == 2.0:
            assert cases.equal(got, _loop(c, scale)), scale
    if c.keys.size:
        assert c.operator.device().last_ms > 0.0


@pytest.mark.parametrize("wrong", sorted(cases.WRONG))
def test_the_device_is_none_of_the_wrong_variants(wrong):
    c = cases.case(cases.WRITTEN_FOR[wrong])
    assert not cases.equal(_device(c, 2.0), c.law(2.0, wrong=wrong)), cases.WRONG[wrong]


@pytest.mark.parametrize("name", ["kagome16 sizes", "empty segments", "parts of ring22 inversion -1"])
def test_the_order_of_the_segments_does_not_matter(name):
    c = cases.case(name)
    want, lost = _device(c, 2.0)
    order = list(np.random.default_rng(5).permutation(c.segments))
    p = c.permuted(order)
    field, unresolved = _device(p, 2.0)
    for at, g in enumerate(order):
        lo, hi = int(c.offsets[g]), int(c.offsets[g + 1])
        plo = int(p.offsets[at])
        assert cases.same_bits(field[plo:plo + hi - lo], want[lo:hi]) and unresolved[at] == lost[g]


def test_no_environment_at_all_and_a_null_unresolved():
    from annealing_sign_problem_amd import _lib

    c = cases.case("kagome16 sizes")
    device = c.operator.device()
    field, unresolved = device.field_segments(c.keys, c.psi, c.offsets, None, None, None, scale=-1.0)
    assert cases.same_bits(field, -1.0 * np.zeros(c.keys.size))
    for g in range(c.segments):
        _, _, coeffs = c.connections(g)
        keys = c.segment(g)[0]
        leaving = ~cases.positions(keys, c.connections(g)[1])[1] & (coeffs != 0)
        assert unresolved[g] == np.count_nonzero(leaving) > 0
    out = np.full(c.keys.size, np.nan)
    _lib.check(device._lib.asp_operator_field_segments(
        device._handle, c.segments, _lib.ptr(c.offsets), _lib.ptr(c.keys), _lib.ptr(c.psi), _lib.ptr(c.env_offsets),
        _lib.ptr(c.env_keys), _lib.ptr(c.env_psi), 2.0, _lib.ptr(out), None))
    assert cases.same_bits(out, c.law(2.0)[0])


def test_a_key_outside_the_sector_is_refused_naming_the_segment():
    from annealing_sign_problem_amd import _lib
    import symmetry_cases

    expected = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    assert expected.outside is not None
    good = expected.keys[:40]
    bad = np.union1d(expected.keys[10:30], np.array([expected.outside], dtype=np.uint64))
    keys = np.concatenate([good, good[:3], bad, bad])
    offsets = np.array([0, 40, 43, 43 + bad.size, 43 + 2 * bad.size], dtype=np.uint64)
    device = expected.operator.device()
    field = np.full(keys.size, 12345.5)
    unresolved = np.full(4, 77, dtype=np.uint64)
    env_offsets = np.zeros(5, dtype=np.uint64)
    rc = device._lib.asp_operator_field_segments(
        device._handle, 4, _lib.ptr(offsets), _lib.ptr(keys), _lib.ptr(np.ones(keys.size)), _lib.ptr(env_offsets),
        None, None, 2.0, _lib.ptr(field), _lib.ptr(unresolved))
    assert rc == -3
    message = _lib.last_error()
    assert "2 states lie outside the symmetry sector" in message and "the first in segment 2" in message
    assert np.all(field == 12345.5) and np.all(unresolved == 77)
    with pytest.raises(_lib.AspError, match="outside the symmetry sector"):
        device.field_segments(keys, np.ones(keys.size), offsets, None, None, None)


# -- through the entry points ------------------------------------------------------------------------------------
def _same_models(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.spins.dtype == b.spins.dtype and np.array_equal(a.spins, b.spins)
        x, y = a.ising_hamiltonian.exchange, b.ising_hamiltonian.exchange
        assert x.shape == y.shape and np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
        assert cases.same_bits(x.data, y.data)
        assert cases.same_bits(a.ising_hamiltonian.field, b.ising_hamiltonian.field)
        assert np.array_equal(a.initial_signs, b.initial_signs)
        assert (a.basis_index is None) == (b.basis_index is None)
        assert a.basis_index is None or np.array_equal(a.basis_index, b.basis_index)
        assert a.quantum_hamiltonian is b.quantum_hamiltonian


SIZES = (5, 12, 33, 64, 150, 300)
RELTOL = 1e-4


@pytest.fixture(scope="module")
def kagome16():
    """(operator over its built basis, ground state, its log-amplitude closure, 6 grown clusters of 5-300 states)."""
    from annealing_sign_problem_amd import common
    import eloc_cases

    g = golden("make_ising_kagome16_cluster.npz")
    op, states = eloc_cases.kagome16_basis()
    assert np.array_equal(states, g["basis_states"])
    vector = np.ascontiguousarray(g["ground_state"], dtype=np.float64)
    clusters = [cases.grow(op, size, 400 + size) for size in SIZES]
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), clusters


@pytest.fixture(scope="module")
def loops(kagome16):
    """What the per-cluster calls give, computed once: the models, their extensions and the level with its cutoff
    (a cluster whose cutoff strands a frozen spin leaves the level — decided by the per-cluster calls alone)."""
    from annealing_sign_problem_amd import _lib, common

    op, _, log_fn, clusters = kagome16
    models = [common.make_ising_model(c, op, log_psi_fn=log_fn, external_field=True) for c in clusters]
    extended = [common.make_hamiltonian_extension(m, log_fn, external_field=True) for m in models]
    kept, cut = [], []
    for c, bigger in enumerate(extended):
        try:
            cut.append(common.sparsify_using_global_cutoff(bigger, RELTOL, clusters[c]))
            kept.append(c)
        except _lib.AspError as error:
            assert "not connected to the anchor" in str(error)
    assert len(kept) >= 4
    assert all(np.count_nonzero(m.ising_hamiltonian.field) > 0 for m in models + extended)
    return models, extended, kept, cut


def _no_per_cluster_field(monkeypatch):
    from annealing_sign_problem_amd import operators

    def field(self, *args, **keywords):
        raise AssertionError("the per-cluster field call is not used")

    monkeypatch.setattr(operators.DeviceOperator, "field", field)


@pytest.mark.parametrize("per_cluster_call", ["allowed", "raises"])
def test_the_model_functions_are_their_loops_field_by_field(kagome16, loops, per_cluster_call, monkeypatch):
    from annealing_sign_problem_amd import common

    op, _, log_fn, clusters = kagome16
    models, extended, kept, cut = loops
    if per_cluster_call == "raises":
        _no_per_cluster_field(monkeypatch)
    _same_models(common.make_ising_models(clusters, op, log_psi_fn=log_fn, external_field=True), models)
    _same_models(common.make_hamiltonian_extensions(models, log_fn, external_field=True), extended)
    _same_models(common.extend_and_sparsify_models([models[c] for c in kept], log_fn, RELTOL,
                                                   [clusters[c] for c in kept], external_field=True), cut)


def test_a_log_psi_fn_without_the_index_shortcut_is_asked_per_cluster_in_order(kagome16, loops, monkeypatch):
    from annealing_sign_problem_amd import common

    op, _, log_fn, clusters = kagome16
    asked = []

    def plain(spins):
        asked.append(np.array(spins, copy=True))
        return log_fn(spins)

    _no_per_cluster_field(monkeypatch)
    _same_models([m for m in common.make_ising_models(clusters[:3], op, log_psi_fn=plain, external_field=True)],
                 [common.IsingModel(m.spins, op, m.ising_hamiltonian, m.initial_signs, None) for m in loops[0][:3]])
    assert len(asked) == 6
    for got, want in zip(asked, clusters[:3] + [common.extension_spins(op, c) for c in clusters[:3]]):
        assert np.array_equal(got, want)


def test_the_error_is_that_of_the_first_unresolved_cluster(kagome16, monkeypatch):
    from annealing_sign_problem_amd import common

    op, _, log_fn, clusters = kagome16
    whole = [common.extension_spins(op, c) for c in clusters]
    short = list(whole)
    for g in (2, 4):  # without their first state outside the cluster
        outside = whole[g][~cases.positions(clusters[g], whole[g])[1]]
        short[g] = whole[g][whole[g] != outside[0]]
    monkeypatch.setattr(common, "extension_spins", lambda hamiltonian, spins: short[2])
    with pytest.raises(ValueError, match=r"^[1-9][0-9]* connections leave the cluster") as loop_error:
        common.make_ising_model(clusters[2], op, log_psi_fn=log_fn, external_field=True)
    monkeypatch.setattr(common, "extension_spins_segments", lambda hamiltonian, spins_list: list(short))
    with pytest.raises(ValueError, match=r"^[1-9][0-9]* connections leave the cluster") as error:
        common.make_ising_models(clusters, op, log_psi_fn=log_fn, external_field=True)
    assert str(error.value) == str(loop_error.value)


def test_reweight_ising_models_with_the_field_is_the_per_draw_call(kagome16, monkeypatch):
    from annealing_sign_problem_amd import common

    op, vector, log_fn, clusters = kagome16
    base = common.make_ising_model(clusters[3], op, log_psi_fn=log_fn, external_field=True)
    base.ising_hamiltonian.plan()
    made = []
    try:
        np.random.seed(13)
        noisy = [common.add_noise_to_amplitudes(vector, eps=0.5) for _ in range(4)]
        fns = [common.ground_state_to_log_coeff_fn(x, op.basis) for x in noisy]
        want = [common.reweight_ising_model(base, None, fn, True) for fn in fns]
        made += want
        fields = [m.ising_hamiltonian.field for m in want]
        assert all(np.count_nonzero(f) > 0 for f in fields) and not cases.same_bits(fields[0], fields[1])
        _no_per_cluster_field(monkeypatch)
        got = common.reweight_ising_models(base, log_psi_fns=fns, external_field=True)
        made += got
        _same_models(got, want)
        for g in got:
            assert np.shares_memory(g.ising_hamiltonian.exchange.indices, base.ising_hamiltonian.exchange.indices)
    finally:
        for m in made:
            m.ising_hamiltonian.release()
        base.ising_hamiltonian.release()


def test_the_pipeline_stages_the_results_of_the_unbatched_call(kagome16, loops):
    from annealing_sign_problem_amd import sampled_components

    op, vector, log_fn, clusters = kagome16
    some = [clusters[c] for c in loops[2]]
    loop = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 1, RELTOL, external_field=True)
    batch = sampled_components.stage_clusters(some, op, vector, vector, log_fn, 1, RELTOL, external_field=True,
                                              build_batch=True, level_batch=True)
    assert len(batch) == len(loop) == 2 * len(some)
    assert [entry[0] for entry in batch] == [entry[0] for entry in loop]
    _same_models([entry[1] for entry in batch], [entry[1] for entry in loop])
    for a, b in zip(batch, loop):
        assert np.array_equal(a[2], b[2]) and cases.same_bits(a[3], b[3])
        assert a[4].to_csv_str() == b[4].to_csv_str()
    assert all(np.count_nonzero(entry[1].ising_hamiltonian.field) > 0 for entry in batch)
