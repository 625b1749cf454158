"""The boundary field on the device (asp_operator_field: k_field_rows, k_field_list; csrc/operator_field.hip)
against the sequential law of tests/field_cases.py and the reference binary's fixture, bit for bit, and through
make_ising_model(..., external_field=True), the sparsifier, the solvers and process_cluster."""
import numpy as np
import pytest
import scipy.sparse

import field_cases as cases
import oracle
from conftest import golden

pytestmark = pytest.mark.gpu


def _device_equals_law(c, env_keys=None, env_psi=None, scale=1.0):
    env_keys = c.env_keys if env_keys is None else env_keys
    env_psi = c.env_psi if env_psi is None else env_psi
    field, unresolved = c.operator.device().field(c.keys, c.psi, env_keys, env_psi, scale=scale)
    want, lost = c.law(env_keys, env_psi, scale=scale)
    assert unresolved == lost
    assert cases.same_bits(field, want)
    return field, unresolved


# -- cluster sizes, chunking, bases ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_at_every_scale(name):
    """k_field_rows for the plain bases (24, 64, 65 and 120 bonds; K = 1 ... 301; keys with bit 63), k_field_list
    for the symmetry-adapted bases and single-site flips."""
    c = cases.case(name)
    assert c.operator.device().unique_targets == (name in cases.PLAIN)
    for scale in (1.0, 2.0, 0.3, -1.0):
        _, unresolved = _device_equals_law(c, scale=scale)
        assert unresolved == 0
    if c.env_keys.size:
        assert np.count_nonzero(c.law()[0]) > 0


def test_fixture_of_the_reference_binary():
    g = golden("field_kagome16_cluster.npz")
    device = cases.model_operator("heisenberg_kagome_16").device()
    field, unresolved = device.field(g["keys"], g["psi"], g["env_keys"], g["env_psi"], scale=1.0)
    assert unresolved == 0 and cases.same_bits(field, g["field"])
    assert device.last_ms > 0.0


def test_no_environment():
    """E = 0 with null pointers: the 4-site ring's full basis (nothing leaves: +0.0, nothing unresolved) and a
    cluster whose every off-cluster connection is then unresolved."""
    from annealing_sign_problem_amd import _lib

    ring = cases.case("ring4 full basis")
    field, unresolved = ring.operator.device().field(ring.keys, ring.psi, None, None)
    assert unresolved == 0 and cases.same_bits(field, np.zeros(6))
    c = cases.case("kagome16 K=7")
    device = c.operator.device()
    field, unresolved = device.field(c.keys, c.psi, None, None, scale=-1.0)
    assert unresolved == np.count_nonzero(c.leaving) > 0 and cases.same_bits(field, -1.0 * np.zeros(7))
    # unresolved may be NULL
    out = np.full(7, np.nan)
    _lib.check(device._lib.asp_operator_field(device._handle, 7, _lib.ptr(c.keys), _lib.ptr(c.psi), 0, None, None,
                                              2.0, _lib.ptr(out), None))
    assert cases.same_bits(out, np.zeros(7))


@pytest.mark.parametrize("size", [1, 63, 64, 65, 4095, 4096, 4097])
def test_environment_sizes(size):
    c = cases.case("kagome16 K=300")
    env_keys, env_psi = cases.environment_of_size(c, size, seed=size)
    _device_equals_law(c, env_keys, env_psi)


def test_environment_that_differs_only_above_bit_32():
    """The environment of one state of the 64-site ring, restricted to the targets that flip sites >= 32: its keys
    share their low 32 bits."""
    c = cases.case("ring64 bit 63")
    op = c.operator
    key = c.keys[-1:]
    one = cases.make_case("one state", op, key, seed=3)
    high = one.env_keys[(one.env_keys ^ key[0]) < np.uint64(1 << 32)]
    env = one.env_keys[(one.env_keys ^ key[0]) >= np.uint64(1 << 32)]
    env = env[((env ^ key[0]) & np.uint64(0xFFFFFFFF)) == 0]
    assert env.size >= 8 and high.size >= 8 and np.unique(env & np.uint64(0xFFFFFFFF)).size == 1
    field, unresolved = _device_equals_law(one, env, np.linspace(-1.0, 1.0, env.size))
    assert unresolved == one.env_keys.size - env.size and field[0] != 0.0


@pytest.mark.parametrize("name", ["kagome16 K=1", "kagome16 K=7", "ring20 all-to-all, inversion -1"])
def test_awkward_amplitudes(name):
    """-0.0, 0.0, subnormals and negatives in env_psi; terms that cancel to zero on the way."""
    c = cases.case(name)
    _device_equals_law(c, env_psi=cases.awkward_amplitudes(c.env_keys.size), scale=-1.0)
    _device_equals_law(c, env_psi=cases.awkward_amplitudes(c.env_keys.size), scale=0.3)
    # +x, -x, +x, ... in the order in which the connections first reach the environment states
    leaving = c.other[c.leaving]
    order = leaving[np.sort(np.unique(leaving, return_index=True)[1])]
    cancel = np.zeros(c.env_keys.size)
    cancel[cases.positions(c.env_keys, order)[0]] = np.where(np.arange(order.size) % 2 == 0, 0.3, -0.3)
    field, _ = _device_equals_law(c, env_psi=cancel)
    if name == "kagome16 K=1":  # equal coefficients, an even number of terms: every second partial sum is +0.0
        assert c.env_keys.size % 2 == 0 and np.unique(c.coeffs[c.leaving]).size == 1
        assert cases.same_bits(field, np.zeros(1))


@pytest.mark.parametrize("name", ["kagome16 K=300", "kagome18 inversion -1"])
def test_overlapping_environment_has_no_effect(name):
    c = cases.case(name)
    both = np.union1d(c.env_keys, c.keys)
    wrong = np.full(both.size, 1e3)
    wrong[cases.positions(both, c.env_keys)[0]] = c.env_psi
    field, unresolved = _device_equals_law(c, both, wrong)
    assert unresolved == 0 and cases.same_bits(field, c.law()[0])


@pytest.mark.parametrize("name", ["kagome16 K=300", "ring22 inversion -1"])
def test_a_missing_environment_key_is_counted(name):
    c = cases.case(name)
    _, unresolved = _device_equals_law(c, c.env_keys[1:], c.env_psi[1:])
    assert unresolved >= 1


def test_a_key_outside_the_sector_is_refused():
    from annealing_sign_problem_amd import _lib
    import symmetry_cases

    expected = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    assert expected.outside is not None
    keys = np.union1d(expected.keys, np.array([expected.outside], dtype=np.uint64))
    with pytest.raises(_lib.AspError, match="outside the symmetry sector") as error:
        expected.operator.device().field(keys, np.ones(keys.size), None, None)
    assert error.value.code == -3


# -- through the entry points ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kagome16():
    """(operator, ground state over its basis, amplitude closure, a cluster)."""
    from annealing_sign_problem_amd import common

    g = golden("make_ising_kagome16_cluster.npz")
    op = cases.model_operator("heisenberg_kagome_16")
    op.basis.build()
    assert np.array_equal(op.basis.states, g["basis_states"])
    vector = np.ascontiguousarray(g["ground_state"], dtype=np.float64)
    return op, vector, common.ground_state_to_log_coeff_fn(vector, op.basis), np.ascontiguousarray(g["spins"])


def test_make_ising_model_with_field(kagome16):
    from annealing_sign_problem_amd import common

    op, vector, log_fn, cluster = kagome16
    plain = common.make_ising_model(cluster, op, log_psi_fn=log_fn)
    model = common.make_ising_model(cluster, op, log_psi_fn=log_fn, external_field=True)
    assert not np.any(plain.ising_hamiltonian.field) and np.count_nonzero(model.ising_hamiltonian.field) > 0
    for a, b in ((plain.ising_hamiltonian.exchange, model.ising_hamiltonian.exchange),):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert a.data.tobytes() == b.data.tobytes()
    assert np.array_equal(plain.initial_signs, model.initial_signs) and np.array_equal(plain.spins, model.spins)
    worst, scale = cases.identity_defect(op, vector, model.spins, model.ising_hamiltonian.exchange,
                                         model.ising_hamiltonian.field)
    assert worst <= 1e-12 * scale
    blind, _ = cases.identity_defect(op, vector, plain.spins, plain.ising_hamiltonian.exchange,
                                     plain.ising_hamiltonian.field)
    assert blind > 1e-6 * scale
    # the extension passes the flag on, and the sparsifier keeps field[keep]
    extended = common.make_hamiltonian_extension(model, log_fn, external_field=True)
    assert np.array_equal(extended.spins, common.extension_spins(op, cluster))
    worst, scale = cases.identity_defect(op, vector, extended.spins, extended.ising_hamiltonian.exchange,
                                         extended.ising_hamiltonian.field)
    assert worst <= 1e-12 * scale
    assert not np.any(common.make_hamiltonian_extension(model, log_fn).ising_hamiltonian.field)
    cut = common.sparsify_using_global_cutoff(extended, 2e-3, cluster)
    assert cut.size < extended.size
    keep = cases.positions(extended.spins, cut.spins)[0]
    assert cases.same_bits(cut.ising_hamiltonian.field, extended.ising_hamiltonian.field[keep])


def test_make_ising_model_raises_on_unresolved_connections(kagome16, monkeypatch):
    from annealing_sign_problem_amd import common

    op, _, log_fn, cluster = kagome16
    whole = common.extension_spins(op, cluster)
    outside = whole[~cases.positions(cluster, whole)[1]]
    monkeypatch.setattr(common, "extension_spins", lambda hamiltonian, spins: whole[whole != outside[0]])
    with pytest.raises(ValueError, match=r"^[1-9][0-9]* connections leave the cluster"):
        common.make_ising_model(cluster, op, log_psi_fn=log_fn, external_field=True)


def test_solvers_take_the_field_bit_for_bit(kagome16):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import common

    op, _, log_fn, cluster = kagome16
    model = common.make_ising_model(cluster, op, log_psi_fn=log_fn, external_field=True)
    ham = model.ising_hamiltonian
    J, h = scipy.sparse.csr_matrix(ham.exchange), np.array(ham.field)
    info = ham.info()
    betas = sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 24)
    for shuffled, reference in ((False, oracle.sa_anneal), (True, oracle.sa_anneal_shuffled)):
        xs, es = sa.anneal_raw(ham, 4242, betas, 5, 0, None, shuffled=shuffled)
        oxs, oes, _, _ = reference(J, h, 4242, betas, 5, 0, None, info.energy_scale_exp, num_threads=4)
        assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    x, e = sa.greedy_solve(ham)
    ox, oe = oracle.greedy_solve(J, h)
    assert np.array_equal(x, ox) and e == oe


def test_process_cluster_with_and_without_the_flag(kagome16):
    from annealing_sign_problem_amd import common, sampled_components

    op, vector, log_fn, cluster = kagome16

    def run(**keywords):
        return sampled_components.process_cluster(cluster, op, vector, vector, log_fn, 1, 1e-4, False, **keywords)

    def today():  # the function's body before the flag existed
        out, h = [], None
        for i in range(2):
            if i == 0:
                h = common.make_ising_model(cluster, op, log_psi_fn=log_fn)
                exact_signs, weights = sampled_components.exact_signs_and_weights(cluster, h, vector, op.basis)
            else:
                h = common.sparsify_using_global_cutoff(common.make_hamiltonian_extension(h, log_fn), 1e-4, cluster)
            assert not np.any(h.ising_hamiltonian.field)
            r = sampled_components.solve_and_test_model(h, cluster, exact_signs, weights, False)
            r.amplitude_overlap = sampled_components.amplitude_overlap(h.spins, vector, vector, op.basis, h.basis_index)
            out.append(r)
        return out

    without, explicit, before = run(), run(external_field=False), today()
    assert [r.to_csv_str() for r in without] == [r.to_csv_str() for r in before] == [r.to_csv_str() for r in explicit]
    with_field = run(external_field=True)
    assert [r.size for r in with_field] == [r.size for r in without]
    for r in with_field:
        assert np.isfinite([r.greedy_accuracy, r.greedy_overlap, r.amplitude_overlap]).all()
        assert 0.5 <= r.greedy_accuracy <= 1.0 and 0.0 <= r.greedy_overlap <= 1.0 + 1e-12
    # the field changes no starting configuration
    a = common.make_ising_model(cluster, op, log_psi_fn=log_fn)
    b = common.make_ising_model(cluster, op, log_psi_fn=log_fn, external_field=True)
    assert np.array_equal(a.initial_signs, b.initial_signs)
    staged = sampled_components.stage_clusters([cluster], op, vector, vector, log_fn, 1, 1e-4, external_field=True)
    assert [entry[4].to_csv_str() for entry in staged] == [r.to_csv_str() for r in with_field]
    assert all(np.count_nonzero(entry[1].ising_hamiltonian.field) > 0 for entry in staged)
