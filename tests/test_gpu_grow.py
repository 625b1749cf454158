"""The segmented cluster growth on the device (asp_operator_grow_segments; csrc/cluster_grow.hip) against the pass
form of ASP-GROW-1 in tests/grow_cases.py: members and passes of every segment, bit for bit.

The case with seeds at or above 2^63 on 64 sites is in the list: the host action handles them."""
import ctypes

import numpy as np
import pytest

import grow_cases as gc

pytestmark = pytest.mark.gpu

INVALID = -3


def _grow(call, order=None):
    """``[(members, passes)]`` of a call's segments, in the call's order; `order`: the places they take in the call."""
    order = list(range(len(call.seeds))) if order is None else list(order)
    pick = lambda values, dtype: np.array([values[j] for j in order], dtype=dtype)  # noqa: E731
    clusters, passes = call.operator.device().grow_segments(
        pick(call.seeds, np.uint64), pick(call.sizes, np.uint64), call.p, call.seed, ids=pick(call.ids, np.uint32))
    out = [None] * len(order)
    for place, j in enumerate(order):
        out[j] = (clusters[place], int(passes[place]))
    return out


@pytest.mark.parametrize("name", [c.name for c in gc.calls()])
def test_every_case_is_the_law(name):
    call = gc.call(name)
    got = _grow(call)
    assert all(members.dtype == np.uint64 for members, _ in got)
    assert gc.same(got, call.law()), name
    assert call.operator.device().last_ms > 0.0


@pytest.mark.parametrize("variant", sorted(gc.VARIANTS))
def test_the_device_is_not_a_wrong_variant(variant):
    """On the cases where the variant differs from the law (tests/test_grow_cases.py: there is one) the device sides
    with the law."""
    told_apart = 0
    for call in gc.calls():
        wrong = call.law(**gc.VARIANTS[variant])
        if not gc.same(wrong, call.law()):
            assert not gc.same(_grow(call), wrong), (variant, call.name)
            told_apart += 1
    assert told_apart


def test_finished_segments_are_unchanged_by_later_passes():
    """Ends in passes 0, 1, 2 and later side by side: each segment is what it is alone."""
    call = gc.call("ends in passes")
    together = _grow(call)
    for j in range(len(call.seeds)):
        alone = gc.Call("alone", call.op, call.seeds[j:j + 1], call.sizes[j:j + 1], call.ids[j:j + 1], call.p,
                        call.seed)
        assert gc.same(_grow(alone), together[j:j + 1]), j
    assert sorted({passes for _, passes in together})[:3] == [1, 2, 3]


def test_equal_ids_give_equal_clusters_and_different_ids_different_ones():
    a, b, c, d = [members for members, _ in _grow(gc.call("one seed"))]
    assert np.array_equal(a, b) and np.array_equal(a, d) and not np.array_equal(a, c)


def test_one_call_eight_calls_and_the_reversed_call_agree():
    call = gc.EIGHT
    together = _grow(call)
    assert gc.same(together, call.law())
    assert gc.same(_grow(call, order=range(7, -1, -1)), together)
    one_by_one = []
    for j in range(8):
        one_by_one += _grow(gc.Call("one", call.op, call.seeds[j:j + 1], call.sizes[j:j + 1], call.ids[j:j + 1],
                                    call.p, call.seed))
    assert gc.same(one_by_one, together)


def test_the_decision_boundary():
    x, (low, high) = gc.boundary_calls()
    dropped, kept = _grow(low)[0][0], _grow(high)[0][0]
    assert x not in dropped.tolist() and x in kept.tolist()


def _raw(op, seeds, sizes, p=0.5):
    from annealing_sign_problem_amd import _lib

    seeds, sizes = np.array(seeds, dtype=np.uint64), np.array(sizes, dtype=np.uint64)
    ids = np.arange(seeds.size, dtype=np.uint32)
    out = np.full(int(sizes.sum()), 4242, dtype=np.uint64)
    out_offsets = np.full(seeds.size + 1, 77, dtype=np.uint64)
    passes = np.full(seeds.size, 55, dtype=np.uint32)
    count = ctypes.c_uint64(991)
    rc = _lib.load().asp_operator_grow_segments(
        op.device()._handle, seeds.size, _lib.ptr(seeds), _lib.ptr(sizes), _lib.ptr(ids), p, gc.SEED, out.size,
        _lib.ptr(out), _lib.ptr(out_offsets), ctypes.byref(count), _lib.ptr(passes))
    untouched = bool(np.all(out == 4242) and np.all(out_offsets == 77) and np.all(passes == 55) and count.value == 991)
    return rc, untouched


def test_a_seed_outside_the_sector_is_refused():
    from annealing_sign_problem_amd import _lib

    call = gc.call("ring22 inversion -1")
    rc, untouched = _raw(call.operator, [call.seeds[0], gc.norm0_state(), call.seeds[1]], [20, 20, 1])
    assert rc == INVALID and "outside the symmetry sector" in _lib.last_error() and untouched
    # ... also where its size is 1 and nothing it reaches matters
    rc, untouched = _raw(call.operator, [gc.norm0_state()], [1])
    assert rc == INVALID and untouched


def test_a_seed_with_a_bit_above_the_sites_is_refused_before_any_output():
    from annealing_sign_problem_amd import _lib

    rc, untouched = _raw(gc.operator("kagome16"), [gc.NEEL16, gc.NEEL16 | (1 << 16)], [5, 5])
    assert rc == INVALID and "seed of segment 1 has a bit at or above site 16" in _lib.last_error() and untouched


def test_passes_may_be_left_out():
    from annealing_sign_problem_amd import _lib

    call = gc.call("size 2")
    seeds, sizes = np.array(call.seeds, dtype=np.uint64), np.array(call.sizes, dtype=np.uint64)
    ids = np.array(call.ids, dtype=np.uint32)
    out, out_offsets, count = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64), ctypes.c_uint64(0)
    _lib.check(_lib.load().asp_operator_grow_segments(
        call.operator.device()._handle, 1, _lib.ptr(seeds), _lib.ptr(sizes), _lib.ptr(ids), call.p, call.seed, 2,
        _lib.ptr(out), _lib.ptr(out_offsets), ctypes.byref(count), None))
    assert count.value == 2 and out_offsets.tolist() == [0, 2] and np.array_equal(out, call.law()[0][0])
