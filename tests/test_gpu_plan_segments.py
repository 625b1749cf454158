"""asp_sa_plan_create_segments on the GPU (law ASP-PLAN-SEG-1): for every case of
tests/plan_cases.py each plan of the segmented call equals the plan asp_sa_plan_create makes of the rebased
segment — asp_sa_plan_info as bits and every device array byte for byte (asp_sa_plan_read_array) —, the
arrays equal the numpy restatement's fill, the build counter advances by the number of segments, and content
errors name their segment and leave nothing behind.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import plan_cases as pc

pytestmark = pytest.mark.gpu

INVALID = -3
ROUNDS = sorted(pc.rounds())


def create_segments(segments):
    """(return code, handles) of one segmented call."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    _lib.require_gpu()
    offsets, indptr, indices, data, field = pc.concatenate(segments)
    plans = (ctypes.c_void_p * max(len(segments), 1))(*([1] * len(segments)))
    rc = lib.asp_sa_plan_create_segments(ctypes.c_uint64(len(segments)), _lib.ptr(offsets), _lib.ptr(indptr),
                                         _lib.ptr(indices), _lib.ptr(data), _lib.ptr(field), plans)
    return rc, [ctypes.c_void_p(p) if p else None for p in list(plans)[:len(segments)]]


def create_one(seg):
    from annealing_sign_problem_amd import _lib

    ip, ix, dv, h = seg
    handle = _lib.load().asp_sa_plan_create(ctypes.c_uint64(ip.size - 1), _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv),
                                            _lib.ptr(h))
    assert handle, _lib.last_error()
    return ctypes.c_void_p(handle)


def info_bytes(plan):
    from annealing_sign_problem_amd import _lib

    info = _lib.SaInfo()
    _lib.check(_lib.load().asp_sa_plan_info(plan, ctypes.byref(info)))
    return bytes(info), info


def layout_host(seg):
    from annealing_sign_problem_amd import _lib

    ip, ix, dv, h = seg
    n = ip.size - 1
    colors, positions = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(ctypes.c_uint64(n), _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv), _lib.ptr(h),
                                              None, _lib.ptr(colors), _lib.ptr(positions)))
    return colors, positions


@pytest.mark.parametrize("name", ROUNDS)
def test_plans_equal_asp_sa_plan_create_and_the_restatement(name):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    segments = pc.rounds()[name]
    _lib.require_gpu()
    before = lib.asp_sa_layout_build_count()
    rc, plans = create_segments(segments)
    assert rc == 0, _lib.last_error()
    assert lib.asp_sa_layout_build_count() == before + len(segments)
    assert lib.asp_sa_plan_segments_last_ms() >= 0.0
    assert all(plans) and len({p.value for p in plans}) == len(plans)  # objects of their own
    try:
        for g, (seg, plan) in enumerate(zip(segments, plans)):
            single = create_one(seg)
            try:
                got_info, info = info_bytes(plan)
                assert got_info == info_bytes(single)[0], (name, g)
                colors, positions = layout_host(seg)
                front = pc.plan_front(*seg)
                blocks = pc.plan_blocks(front["a_ptr"], colors, positions)
                expected = dict(blocks, **pc.plan_fill(front, positions, blocks["block_width"], blocks["ell_off"], seg[3]))
                for array in pc.ARRAYS:
                    got, want = sa.read_plan_array(plan, array), sa.read_plan_array(single, array)
                    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, g, array)
                    if array == "ell_col4" and want.size == 0:
                        continue  # the wide layout does not fit: the plan does not hold it
                    assert got.tobytes() == np.ascontiguousarray(expected[array], dtype=got.dtype).tobytes(), (name, g, array)
                if name == "cubic_45000":
                    assert sa.read_plan_array(plan, "ell_col4").size == 0 and sa.read_plan_array(plan, "ell_col").size > 0
                elif info.num_spins:
                    assert sa.read_plan_array(plan, "ell_col4").size == sa.read_plan_array(plan, "ell_col").size
            finally:
                lib.asp_sa_plan_destroy(single)
    finally:
        for plan in plans:  # in any order, each on its own
            lib.asp_sa_plan_destroy(plan)


def test_read_array_refuses_what_it_must():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    rc, plans = create_segments(pc.rounds()["round_of_1"])
    assert rc == 0, _lib.last_error()
    try:
        size = ctypes.c_uint64(0)
        out = np.zeros(4, dtype=np.uint32)
        assert lib.asp_sa_plan_read_array(plans[0], 99, _lib.ptr(out), ctypes.c_uint64(16), ctypes.byref(size)) == INVALID
        assert size.value == 0
        assert lib.asp_sa_plan_read_array(plans[0], 7, _lib.ptr(out), ctypes.c_uint64(16), ctypes.byref(size)) == INVALID
        assert size.value == 150 * 4 and not out.any()  # pos_of_spin of 150 spins: too small, nothing copied
        assert lib.asp_sa_plan_read_array(plans[0], 7, _lib.ptr(out), ctypes.c_uint64(16), None) == INVALID
    finally:
        lib.asp_sa_plan_destroy(plans[0])


@pytest.mark.parametrize("name", sorted(pc.CONTENT_ERRORS))
def test_content_errors_name_the_segment_and_leave_nothing(name):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    segments = pc.content_error_round(name)
    ip, ix, dv, h = segments[1]
    assert lib.asp_sa_layout_host(ctypes.c_uint64(ip.size - 1), _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv), _lib.ptr(h),
                                  None, None, None) == INVALID
    expected = "segment 1: " + _lib.last_error()  # asp_sa_plan_create's message
    rc, plans = create_segments(segments)
    assert rc == INVALID
    assert _lib.last_error() == expected
    assert plans == [None, None, None]
    rc, plans = create_segments([segments[0], segments[2]])  # a following valid call succeeds
    assert rc == 0 and all(plans), _lib.last_error()
    for plan in plans:
        lib.asp_sa_plan_destroy(plan)
