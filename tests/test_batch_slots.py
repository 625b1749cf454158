"""CPU: where the shared launches of the batched calls place the workgroups of one launch class
(asp_sa_batch_slots_host: the table the launcher uploads, without a device).  Placement changes speed
only, so no result can catch a mistake in it; the table is compared here against the rule restated in
numpy: members in descending work, stable; each whole to the XCD (of eight) with the fewest workgroups
so far, ties to the lowest index; every list padded to the longest with (0xFFFFFFFF, 0); x-major."""
import ctypes

import numpy as np
import pytest

from annealing_sign_problem_amd import _lib

XCDS = 8
PAD = (0xFFFFFFFF, 0)
ASP_ERR_INVALID = -3


def rule(work, groups):
    """The table [8][slots_per_xcd][2] by the rule above."""
    order = sorted(range(len(work)), key=lambda k: -work[k])  # (sorted is stable)
    lists = [[] for _ in range(XCDS)]
    for k in order:
        x = min(range(XCDS), key=lambda j: (len(lists[j]), j))
        lists[x] += [(k, g) for g in range(groups[k])]
    longest = max(len(l) for l in lists)
    return np.array([l + [PAD] * (longest - len(l)) for l in lists], dtype=np.uint32).reshape(XCDS, longest, 2)


def table(work, groups, capacity=None):
    work = np.ascontiguousarray(work, dtype=np.float64)
    groups = np.ascontiguousarray(groups, dtype=np.uint32)
    if capacity is None:
        capacity = XCDS * int(groups.sum())  # (no list is longer than all workgroups together)
    slots = np.full((capacity, 2), 0xDEADBEEF, dtype=np.uint32)
    per_xcd = ctypes.c_uint32(0xDEADBEEF)
    rc = _lib.load().asp_sa_batch_slots_host(len(work), _lib.ptr(work), _lib.ptr(groups), ctypes.byref(per_xcd),
                                             _lib.ptr(slots), capacity)
    return rc, per_xcd.value, slots


def check(work, groups):
    rc, per_xcd, slots = table(work, groups)
    assert rc == 0, _lib.last_error()
    want = rule(list(work), list(groups))
    assert per_xcd == want.shape[1]
    got = slots[: XCDS * per_xcd].reshape(XCDS, per_xcd, 2)
    np.testing.assert_array_equal(got, want)
    assert (slots[XCDS * per_xcd:] == 0xDEADBEEF).all()  # nothing written past the table
    return got


def test_no_members():
    rc, per_xcd, slots = table([], [], capacity=4)
    assert rc == 0 and per_xcd == 0
    assert (slots == 0xDEADBEEF).all()


def test_fewer_members_than_xcds():
    got = check([5.0, 9.0, 7.0], [2, 1, 3])
    # longest first: member 1 on XCD 0, member 2 on XCD 1, member 0 on XCD 2; XCDs 3..7 all padding
    assert got[:3, 0, 0].tolist() == [1, 2, 0]
    assert (got[3:].reshape(-1, 2) == PAD).all()


def test_hand_checked_mixed_groups():
    groups = [3, 1, 1, 1, 1, 1, 1, 1, 1, 2]
    got = check(np.arange(10, 0, -1.0), groups)
    assert got.shape[1] == 3
    members = [sorted(set(int(m) for m in got[x, :, 0] if m != PAD[0])) for x in range(XCDS)]
    assert members == [[0], [1, 8], [2, 9], [3], [4], [5], [6], [7]]
    assert got[0].tolist() == [[0, 0], [0, 1], [0, 2]]
    assert got[1].tolist() == [[1, 0], [8, 0], list(PAD)]
    assert got[2].tolist() == [[2, 0], [9, 0], [9, 1]]


def test_one_group_each_is_round_robin():
    got = check(np.arange(20, 0, -1.0), [1] * 20)
    assert got.shape[1] == 3
    for j in range(20):  # member j (the j-th longest) is slot j // 8 of XCD j % 8
        assert got[j % XCDS, j // XCDS].tolist() == [j, 0]


def test_equal_work_keeps_the_order():
    got = check([1.0] * 11, [1] * 11)
    for j in range(11):
        assert got[j % XCDS, j // XCDS].tolist() == [j, 0]
    got = check([2.0, 3.0, 2.0, 3.0, 2.0], [1, 2, 1, 2, 1])  # ties inside a descending order
    assert got[:5, 0, 0].tolist() == [1, 3, 0, 2, 4]


@pytest.mark.parametrize("capacity", [0, 23])
def test_capacity_too_small_writes_nothing(capacity):
    groups = [3, 1, 1, 1, 1, 1, 1, 1, 1, 2]  # the table is 8 x 3 = 24 pairs
    rc, per_xcd, slots = table(np.arange(10, 0, -1.0), groups, capacity=capacity)
    assert rc == ASP_ERR_INVALID
    assert per_xcd == 0xDEADBEEF
    assert (slots == 0xDEADBEEF).all()
    rc, per_xcd, _ = table(np.arange(10, 0, -1.0), groups, capacity=24)
    assert rc == 0 and per_xcd == 3
