"""The cases and the law of the segmented boundary field (tests/field_segment_cases.py, ASP-FIELD-SEG-1, DESIGN.md
§3.5.1) without a device: the law with one segment is the per-cluster law that tests/test_field_cases.py pins to the
reference binary; every named wrong variant differs from the law on the case written for it; and what the cases
claim about themselves is recomputed from their inputs."""
import numpy as np
import pytest

import field_cases
import field_segment_cases as cases


@pytest.mark.parametrize("name", field_cases.REFERENCE)
def test_the_law_with_one_segment_is_the_per_cluster_law(name):
    c = field_cases.case(name)
    for env_keys, env_psi in ((c.env_keys, c.env_psi), (c.env_keys[1:], c.env_psi[1:]), (c.env_keys[:0], c.env_psi[:0])):
        for scale in cases.SCALES + (0.3,):
            want, lost = field_cases.field_law(c.other, c.coeffs, c.counts, c.keys, c.psi, env_keys, env_psi, scale)
            field, unresolved = cases.field_segments_law(
                c.other, c.coeffs, c.counts, c.keys, c.psi, [0, c.keys.size], env_keys, env_psi, [0, env_keys.size],
                scale)
            assert cases.same_bits(field, want) and unresolved.tolist() == [lost]
    if c.env_keys.size:
        assert lost > 0  # (the empty environment loses every connection that leaves)


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_law_is_the_loop_over_the_segments(name):
    """Segment by segment, from connections computed for that segment alone."""
    c = cases.case(name)
    field, unresolved = c.law(2.0)
    assert field.shape == c.keys.shape and unresolved.shape == (c.segments,)
    assert int(c.offsets[-1]) == c.keys.size and int(c.env_offsets[-1]) == c.env_keys.size == c.env_psi.size
    step = max(1, c.segments // 7)
    for g in range(0, c.segments, step):
        keys, psi, env_keys, env_psi = c.segment(g)
        assert np.all(keys[1:] > keys[:-1]) and np.all(env_keys[1:] > env_keys[:-1])
        if keys.size == 0:
            assert unresolved[g] == 0
            continue
        other, coeffs, counts = c.operator.batched_apply(keys)
        want, lost = field_cases.field_law(np.ascontiguousarray(other[:, 0]), coeffs.real, counts, keys, psi, env_keys,
                                           env_psi, 2.0)
        lo = int(c.offsets[g])
        assert cases.same_bits(field[lo:lo + keys.size], want) and unresolved[g] == lost


@pytest.mark.parametrize("wrong", sorted(cases.WRONG))
def test_every_wrong_variant_differs_on_the_case_written_for_it(wrong):
    c = cases.case(cases.WRITTEN_FOR[wrong])
    for scale in cases.SCALES:
        law, other = c.law(scale), c.law(scale, wrong=wrong)
        assert not cases.equal(other, law), cases.WRONG[wrong]
        if wrong == "W3":
            assert cases.same_bits(other[0], law[0]) and other[1].sum() == law[1].sum()
        else:
            assert not cases.same_bits(other[0], law[0])


def test_segment_sizes():
    c = cases.case("kagome16 sizes")
    assert np.diff(c.offsets.astype(np.int64)).tolist() == [1, 2, 3, 5, 63, 64, 65, 301, 1]
    assert c.keys.size % 4 != 0
    # boundaries inside a workgroup of four rows
    assert np.count_nonzero(c.offsets[1:-1].astype(np.int64) % 4) >= 5
    many = cases.case("4097 segments of 1-3 keys")
    sizes = np.diff(many.offsets.astype(np.int64))
    assert many.segments == 4097 and set(sizes.tolist()) == {1, 2, 3}
    sizes = np.diff(cases.case("environment sizes").env_offsets.astype(np.int64))
    assert sizes.tolist() == [0, 1, 63, 64, 65, 4097]
    empty = cases.case("empty segments")
    sizes = np.diff(empty.offsets.astype(np.int64)).tolist()
    env_sizes = np.diff(empty.env_offsets.astype(np.int64)).tolist()
    assert (0, 0) in zip(sizes, env_sizes)
    assert any(n == 0 and e > 0 for n, e in zip(sizes, env_sizes))
    assert any(n > 0 and e == 0 for n, e in zip(sizes, env_sizes))
    nothing = cases.case("all segments empty")
    assert nothing.keys.size == 0 and nothing.segments == 3 and nothing.env_keys.size > 0
    assert cases.case("S=1: kagome16 K=7").segments == 1


def test_the_300_fold_membership():
    c = cases.case("one state in 300 segments")
    x, y = cases.shared_states()
    assert c.segments == 300
    in_cluster = sum(int(x in c.segment(g)[0].tolist()) for g in range(c.segments))
    in_environment = sum(int(y in c.segment(g)[2].tolist()) for g in range(c.segments))
    assert in_cluster == 300 and in_environment == 300
    assert np.count_nonzero(c.keys == np.uint64(x)) == 300 and np.count_nonzero(c.env_keys == np.uint64(y)) == 300


def test_the_neighbouring_clusters_share_targets():
    """Targets of A's rows that are cluster keys of B and environment keys of A."""
    c = cases.case("neighbouring clusters")
    a_keys, _, a_env, _ = c.segment(0)
    b_keys = c.segment(1)[0]
    _, targets, coeffs = c.connections(0)
    shared = (coeffs != 0) & cases.positions(b_keys, targets)[1] & cases.positions(a_env, targets)[1]
    assert np.count_nonzero(shared) >= 10 and np.unique(targets[shared]).size >= 10
    assert not np.any(cases.positions(a_keys, b_keys)[1])


def test_the_draws_share_keys_and_differ_in_amplitudes():
    c = cases.case("one cluster, 5 draws")
    assert c.segments == 5
    first = c.segment(0)
    for g in range(1, 5):
        keys, psi, env_keys, env_psi = c.segment(g)
        assert np.array_equal(keys, first[0]) and np.array_equal(env_keys, first[2])
        assert not np.array_equal(psi, first[1]) and not np.array_equal(env_psi, first[3])


def test_the_missing_key_is_missed_in_segment_2_only():
    c = cases.case("a missing environment key")
    unresolved = c.law(1.0)[1]
    assert unresolved[2] >= 1 and np.count_nonzero(unresolved) == 1 and c.segments == 5


def test_high_bits_and_bond_counts():
    ring = cases.case("parts of ring64 bit 63")
    assert np.count_nonzero(ring.keys >> np.uint64(63)) >= 10
    for name, bonds in (("j1j2 64 bonds", 64), ("sk16 first 65 bonds", 65), ("sk16 120 bonds", 120)):
        assert field_cases.num_bonds(cases.case("parts of " + name).operator) == bonds
    # rows of the list variant that reach one outside representative twice
    for name in ("parts of ring22 inversion -1", "parts of single-site flips"):
        c = cases.case(name)
        twice = 0
        for g in range(c.segments):
            keys = c.segment(g)[0]
            sources, targets, coeffs = c.connections(g)
            leaving = ~cases.positions(keys, targets)[1] & (coeffs != 0)
            pairs = np.stack([sources[leaving], targets[leaving]], axis=1)
            twice += int(np.count_nonzero(np.unique(pairs, axis=0, return_counts=True)[1] > 1))
        assert twice >= 1, name


def test_signed_zeros_and_subnormals_reach_the_field():
    c = cases.case("signed zeros and subnormals")
    assert np.any(np.signbit(c.env_psi) & (c.env_psi == 0)) and np.any((c.env_psi != 0) & (np.abs(c.env_psi) < 1e-307))
    plus, minus = c.law(1.0)[0], c.law(-1.0)[0]
    assert np.any(np.signbit(plus) != np.signbit(minus))
    nothing = cases.case("empty segments")
    field = nothing.law(-1.0)[0]
    lo, hi = int(nothing.offsets[1]), int(nothing.offsets[2])  # the cluster without an environment
    assert hi > lo and np.all(field[lo:hi] == 0) and np.all(np.signbit(field[lo:hi]))  # -1 * +0.0


@pytest.mark.parametrize("name", cases.CONTRIBUTIONS)
def test_between_10_and_90_percent_of_the_connections_contribute(name):
    share = cases.contributing_share(cases.case(name))
    assert 0.10 <= share <= 0.90, share


def test_a_permutation_keeps_every_segment():
    c = cases.case("kagome16 sizes")
    order = [4, 0, 8, 2, 7, 1, 6, 3, 5]
    p = c.permuted(order)
    field, unresolved = p.law(2.0)
    want, lost = c.law(2.0)
    for at, g in enumerate(order):
        lo, hi = int(c.offsets[g]), int(c.offsets[g + 1])
        plo = int(p.offsets[at])
        assert cases.same_bits(field[plo:plo + hi - lo], want[lo:hi]) and unresolved[at] == lost[g]
