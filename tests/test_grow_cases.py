"""The laws of tests/grow_cases.py against each other, without a GPU: the pass form of ASP-GROW-1
against the reference's state-by-state loop, against a plain breadth-first search at p = 1, its invariants, the WRONG
variants against the case list, and the numpy Philox against the oracle's."""
import numpy as np
import pytest

import accept_cases
import grow_cases as gc

CALLS = gc.calls()
NAMES = [c.name for c in CALLS]


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_form_is_the_state_by_state_loop(name):
    call = gc.call(name)
    assert gc.same(call.law(), call.loop())


@pytest.mark.parametrize("name", [c.name for c in CALLS if c.p == 1.0])
def test_keep_probability_one_is_the_truncated_breadth_first_search(name):
    call = gc.call(name)
    for (members, _), s0, size in zip(call.law(), call.seeds, call.sizes):
        assert np.array_equal(members, gc.breadth_first(call.operator, s0, size))


def test_keep_probability_zero_keeps_the_seed_alone():
    call = gc.call("keep probability 0")
    assert gc.threshold_of(0.0) == 0 and gc.threshold_of(1.0) == gc.WORDS
    assert [m.tolist() for m, _ in call.law()] == [[call.seeds[0]]] and call.law()[0][1] == 1


@pytest.mark.parametrize("name", NAMES)
def test_a_cluster_never_exceeds_its_size_and_falls_short_only_when_the_frontier_died(name):
    call = gc.call(name)
    for (members, passes), s0, size, stream in zip(call.law(), call.seeds, call.sizes, call.ids):
        assert np.all(members[1:] > members[:-1]) and s0 in members.tolist() and passes >= 1
        assert members.size <= size
        if members.size < size:
            trace = gc.trace_of(call.op, s0, size, stream, call.p, call.seed)
            # no pass stopped; the growth ended because the last pass's sources kept nothing
            assert all(one.stop is None for one in trace) and len(trace) == passes


def test_the_cases_are_what_their_names_say():
    assert gc.call("size 1").law()[0][1] == 1 and gc.call("size 2").law()[0][0].size == 2
    component = gc.call("the frontier dies").law()[0][0]
    assert 1 < component.size < 1000
    assert np.array_equal(component, gc.breadth_first(gc.operator("kagome16 three bonds"), gc.NEEL16, 10 ** 6))
    wide = gc.call("frontiers and member tables across")
    frontiers = [one.frontier.size for one in gc.trace_of(wide.op, gc.NEEL16, 1500, 7, 1.0, wide.seed)]
    assert frontiers[1] == gc.WAVE and max(frontiers) > 2 * gc.GROW_TILE
    assert [m.size for m, _ in wide.law()] == list(wide.sizes)
    mixed = [passes for _, passes in gc.call("ends in passes").law()]
    assert {1, 2, 3} <= set(mixed) and max(mixed) > 3
    a, b, c, d = [m for m, _ in gc.call("one seed").law()]
    assert np.array_equal(a, b) and np.array_equal(a, d) and not np.array_equal(a, c)
    x, (low, high) = gc.boundary_calls()
    assert x not in low.law()[0][0].tolist() and x in high.law()[0][0].tolist()
    assert high.p - low.p == 1.0 / gc.WORDS
    for name in ("kagome18 inversion -1", "ring22 inversion -1"):
        call = gc.call(name)
        rep, _, norm = call.operator.basis.group.state_info(np.array(call.seeds, dtype=np.uint64))
        assert rep.tolist() == list(call.seeds) and np.all(norm > 0)
    with pytest.raises(ValueError):
        gc.grow_law(gc.operator("ring22 inversion -1"), gc.norm0_state(), 5, 0, 0.5, gc.SEED)
    assert any(s >> 63 for s in gc.call("64 sites").seeds)


@pytest.mark.parametrize("variant", sorted(gc.VARIANTS))
def test_every_wrong_variant_differs_from_the_law_on_some_case(variant):
    differing = [c.name for c in CALLS if not gc.same(c.law(**gc.VARIANTS[variant]), c.law())]
    assert differing, variant


def test_applying_the_source_at_stop_too_cannot_be_seen():
    """The variant the specification names but no result can show: the pass that reaches the size ends the segment, so
    the draws of its last source reach neither the members nor the number of passes."""
    for switches in gc.UNOBSERVABLE.values():
        assert all(gc.same(c.law(**switches), c.law()) for c in CALLS)


def test_numpy_philox_is_the_oracles_on_the_counters_of_a_growth():
    import oracle

    call = gc.call("ends in passes")
    seed = call.seed
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    counters = [(0, 1, 0, 0), (3, 24, 2, 7), (300, 64, 5, 47), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)]
    counters += [(i, k, 1, stream) for i in (0, 1, 255, 256) for k in (0, 1, 25) for stream in (0, 4095)]
    for c in counters:
        want = oracle.philox4x32_10(np.array(c, dtype=np.uint32), key)
        assert np.array_equal(accept_cases.philox(*c, seed), want), c
        assert int(gc.words(*c, seed)) == int(want[0])
