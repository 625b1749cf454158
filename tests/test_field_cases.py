"""No device: the cases of tests/field_cases.py and its sequential restatement `field_law` of the boundary field
(specification ASP-FIELD-1) against the reference's build_matrix, the energy identity that makes
scale = 2 the right field, the unresolved count, and what every case is there to reach."""
import numpy as np
import pytest

import field_cases as cases
import oracle
from conftest import golden


def _build_matrix(*args):
    """The reference binary where it can be built or was shipped, this repository's restatement of it otherwise."""
    try:
        return oracle.ref_build_matrix(*args)
    except RuntimeError:
        return oracle.build_matrix(*args)


def _reference_field(c, env_keys, env_psi):
    ones = np.ones(c.keys.size, dtype=np.int64)
    return _build_matrix(c.keys, ones, c.psi, c.other, c.coeffs, c.counts,
                         cases.other_psi(c.other, env_keys, env_psi))[4]


@pytest.mark.parametrize("name", cases.NAMES)
def test_field_law_is_the_reference_binary_bit_for_bit(name):
    c = cases.case(name)
    field, unresolved = c.law(scale=1.0)
    assert unresolved == 0
    assert cases.same_bits(field, _reference_field(c, c.env_keys, c.env_psi))
    # scale = 2 is exact
    assert cases.same_bits(c.law(scale=2.0)[0], 2.0 * field)


def test_reference_cases_cover_the_issue_list():
    sizes = sorted(cases.case(name).keys.size for name in cases.REFERENCE)
    assert sizes[0] == 1 and sizes[-1] == 300 and set(cases.REFERENCE) <= set(cases.NAMES)


@pytest.mark.parametrize("name", ["kagome16 K=7", "kagome16 K=300", "ring20 all-to-all, inversion -1"])
def test_field_law_with_awkward_and_missing_environments(name):
    """Signed zeros, subnormals, an environment that overlaps the cluster, one that misses keys."""
    c = cases.case(name)
    env_psi = cases.awkward_amplitudes(c.env_keys.size)
    assert cases.same_bits(c.law(env_psi=env_psi)[0], _reference_field(c, c.env_keys, env_psi))
    both = np.union1d(c.env_keys, c.keys)
    wrong = np.full(both.size, 1e3)
    wrong[cases.positions(both, c.env_keys)[0]] = c.env_psi
    field, unresolved = c.law(both, wrong)
    assert unresolved == 0 and cases.same_bits(field, c.law()[0])
    short_keys, short_psi = c.env_keys[1:], c.env_psi[1:]
    field, unresolved = c.law(short_keys, short_psi)
    assert unresolved == np.count_nonzero(c.other[c.leaving] == c.env_keys[0]) >= 1
    assert cases.same_bits(field, _reference_field(c, short_keys, short_psi))
    # no environment at all: everything that leaves is unresolved, the field is +0.0
    field, unresolved = c.law(c.env_keys[:0], c.env_psi[:0], scale=2.0)
    assert unresolved == np.count_nonzero(c.leaving) and cases.same_bits(field, np.zeros(c.keys.size))


def test_golden_fixture_is_the_law():
    g = golden("field_kagome16_cluster.npz")
    op = cases.model_operator("heisenberg_kagome_16")
    other, coeffs, counts = op.batched_apply(g["keys"])
    field, unresolved = cases.field_law(other[:, 0], coeffs.real, counts, g["keys"], g["psi"], g["env_keys"],
                                        g["env_psi"], 1.0)
    assert unresolved == 0 and cases.same_bits(field, g["field"]) and np.count_nonzero(g["field"]) > 0


@pytest.mark.parametrize("name", ["kagome16 K=1", "kagome16 K=7", "kagome16 K=300", "j1j2 64 bonds", "sk16 120 bonds",
                                  "kagome18 inversion +1", "kagome18 inversion -1"])
def test_energy_identity(name):
    """For a symmetric H, amplitudes |v_i| / c on the cluster and the outside signs kept, c^2 (s'Js + h's) with
    h = the field at scale 2 differs from phi(s)' H phi(s) by a constant: differences agree to the project's
    energy tolerance, 1e-12 relative to c^2 (sum|J| + sum|h|)."""
    c = cases.case(name)
    op = c.operator
    if op.basis._states is None:
        op.basis.build()
    rng = np.random.default_rng(5)
    vector = rng.normal(size=op.basis.number_states) * np.exp(rng.normal(size=op.basis.number_states))
    vector /= np.linalg.norm(vector)
    where = np.searchsorted(op.basis.states, c.keys)
    norm = np.linalg.norm(vector[where])
    psi = vector[where] / norm
    env_psi = vector[np.searchsorted(op.basis.states, c.env_keys)] / norm
    field, unresolved = c.law(env_psi=env_psi, scale=2.0, psi=psi)
    assert unresolved == 0
    exchange = cases.couplings(op, c.keys, psi)
    worst, scale = cases.identity_defect(op, vector, c.keys, exchange, field)
    assert worst <= 1e-12 * scale
    if c.keys.size > 1:
        # ... and without the field they do not (the check can fail)
        blind, _ = cases.identity_defect(op, vector, c.keys, exchange, np.zeros_like(field))
        assert blind > 1e-6 * scale


def test_cases_reach_what_they_are_there_for():
    one = cases.case("kagome16 K=1")
    assert one.leaving.sum() == one.counts.sum() - 1          # every connection but the diagonal leaves
    assert cases.case("kagome16 K=301").keys.size % 4 == 1    # the last workgroup holds one row
    ring4 = cases.case("ring4 full basis")
    assert ring4.env_keys.size == 0 and not ring4.leaving.any()
    bonds = [cases.num_bonds(cases.case(n).operator) for n in ("kagome16 K=7", "j1j2 64 bonds", "sk16 first 65 bonds",
                                                               "sk16 120 bonds")]
    assert bonds == [24, 64, 65, 120]
    high = cases.case("ring64 bit 63")
    assert np.any(high.keys >> np.uint64(63)) and np.any(high.env_keys >> np.uint64(63))
    # a row that reaches ONE outside representative twice, and targets of norm 0 (coefficient exactly 0)
    for name in ("ring20 all-to-all, inversion -1", "single-site flips"):
        c = cases.case(name)
        offsets = np.concatenate([[0], np.cumsum(c.counts)])
        twice = False
        for r in range(c.keys.size):
            out = c.other[offsets[r]:offsets[r + 1]][c.leaving[offsets[r]:offsets[r + 1]]]
            twice = twice or np.unique(out).size < out.size
        assert twice, name
    assert cases.case("ring20 all-to-all, inversion -1").counts.max() > 64   # more than one chunk of the list
    for name in ("ring20 all-to-all, inversion -1", "ring22 inversion -1"):
        c = cases.case(name)
        zero = c.coeffs == 0
        assert zero.any() and not cases.positions(c.keys, c.other[zero])[1].any()
        assert not cases.positions(c.env_keys, c.other[zero])[1].any()
    for name in cases.LISTED:
        op = cases.case(name).operator
        assert op.basis.group is not None or name == "single-site flips"


def test_environment_builders():
    c = cases.case("kagome16 K=300")
    for size in (1, 63, 64, 65, 4095, 4096, 4097):
        env_keys, env_psi = cases.environment_of_size(c, size, seed=size)
        assert env_keys.size == size == env_psi.size and np.all(env_keys[1:] > env_keys[:-1])
        assert not cases.positions(c.keys, env_keys)[1].any()
        _, unresolved = c.law(env_keys, env_psi)
        assert (unresolved == 0) == (size >= c.env_keys.size)
    assert 65 < c.env_keys.size < 4095
