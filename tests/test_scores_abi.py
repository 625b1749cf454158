"""Sign scores (include/asp.h: asp_sign_scores*, asp_sign_distances, asp_sa_chains_scores / _distances;
specification ASP-SCORE-1): what can be checked without a device — the symbols and the
layout of the batch item, every refusal (raised before any device work, so before the missing device is
noticed), and the calls that need no device at all."""
import ctypes

import numpy as np
import pytest

INVALID = -3
TOO_LARGE = -4
SYMBOLS = ("asp_sign_scores", "asp_sign_scores_batch", "asp_sign_distances", "asp_sa_chains_scores",
           "asp_sa_chains_distances", "asp_sign_scores_last_ms")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _scores(spins, count, x, stride, scored, select, exact, weights, outputs=True):
    """Return code of asp_sign_scores, the message, and the outputs (prefilled with a marker)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    matches = np.full(max(count, 1), 77, dtype=np.uint64)
    signed = np.full(max(count, 1), 77.0)
    total = np.full(1, 77.0)
    rc = lib.asp_sign_scores(ctypes.c_uint64(spins), ctypes.c_uint32(count), _ptr(x), ctypes.c_uint64(stride),
                             ctypes.c_uint64(scored), _ptr(select), _ptr(exact), _ptr(weights),
                             _ptr(matches) if outputs else None, _ptr(signed) if outputs else None,
                             _ptr(total) if outputs else None)
    untouched = bool(np.all(matches == 77) and np.all(signed == 77.0) and total[0] == 77.0)
    return rc, _lib.last_error(), untouched


def test_symbols_and_item_layout():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.asp_sign_scores_last_ms.restype is ctypes.c_float
    item = _lib.SignScoresItem
    assert [f for f, _ in item._fields_] == ["num_spins", "count", "x", "x_stride", "num_scored", "select", "exact",
                                             "weights", "out_matches", "out_signed", "out_total"]
    assert ctypes.sizeof(item) == 88 and item.x.offset == 16 and item.out_total.offset == 80


def _valid(spins=130, count=2):
    words = (spins + 63) // 64
    return (np.zeros((count, words), dtype=np.uint64), np.zeros(words, dtype=np.uint64), np.ones(spins))


def test_scores_refusals_come_before_any_device_work():
    x, exact, weights = _valid()
    select = np.arange(130, dtype=np.int32)
    # null required pointers with a non-zero size
    assert _scores(130, 2, None, 3, 130, None, exact, weights)[::2] == (INVALID, True)
    assert _scores(130, 2, x, 3, 130, None, None, weights)[::2] == (INVALID, True)
    assert _scores(130, 2, x, 3, 130, select, None, None)[::2] == (INVALID, True)
    # a stride between 1 and W - 1
    for stride in (1, 2):
        rc, message, untouched = _scores(130, 2, x, stride, 130, None, exact, weights)
        assert (rc, untouched) == (INVALID, True) and "x_stride" in message
    # select entries outside [0, K)
    for bad in (-1, 130, 2**31 - 1):
        wrong = select.copy()
        wrong[77] = bad
        rc, message, untouched = _scores(130, 2, x, 3, 130, wrong, exact, weights)
        assert (rc, untouched) == (INVALID, True) and "select[77]" in message
    # weights that are negative, NaN or infinite
    for bad in (-1.0, -5e-324, np.nan, np.inf, -np.inf):
        wrong = weights.copy()
        wrong[129] = bad
        rc, message, untouched = _scores(130, 2, x, 3, 130, None, exact, wrong)
        assert (rc, untouched) == (INVALID, True) and "weight 129" in message
        assert _scores(130, 2, x, 3, 130, select, exact, wrong)[::2] == (INVALID, True)
    # 2^31 scored positions or more: through select's length, and through K without select
    assert _scores(130, 2, x, 3, 2**31, select, exact, None)[::2] == (TOO_LARGE, True)
    assert _scores(2**31, 2, x, 2**25, 0, None, exact, None)[::2] == (TOO_LARGE, True)


def test_batch_refusals_name_the_item():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    x, exact, weights = _valid()
    wrong = weights.copy()
    wrong[5] = -2.0
    outputs = [(np.full(2, 77, dtype=np.uint64), np.full(2, 77.0), np.full(1, 77.0)) for _ in range(3)]
    items = (_lib.SignScoresItem * 3)()
    for k, item in enumerate(items):
        item.num_spins, item.count, item.x, item.x_stride, item.num_scored = 130, 2, x.ctypes.data, 3, 130
        item.exact, item.weights = exact.ctypes.data, (wrong if k == 2 else weights).ctypes.data
        item.out_matches, item.out_signed, item.out_total = (a.ctypes.data for a in outputs[k])
    assert lib.asp_sign_scores_batch(items, ctypes.c_uint32(3)) == INVALID
    assert "item 2" in _lib.last_error() and "weight 5" in _lib.last_error()
    items[2].weights = weights.ctypes.data
    items[1].x_stride = 2
    assert lib.asp_sign_scores_batch(items, ctypes.c_uint32(3)) == INVALID
    assert "item 1" in _lib.last_error()
    for arrays in outputs:  # (item 0 was valid: nothing ran for it either)
        assert all(np.all(a == 77) for a in arrays)
    assert lib.asp_sign_scores_batch(None, ctypes.c_uint32(3)) == INVALID


def test_distance_and_handle_refusals():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    x, _, _ = _valid()
    out = np.full((2, 2), 77, dtype=np.uint32)

    def distances(spins, count, xs, stride, o):
        return lib.asp_sign_distances(ctypes.c_uint64(spins), ctypes.c_uint32(count), _ptr(xs),
                                      ctypes.c_uint64(stride), _ptr(o))

    assert distances(130, 2, None, 3, out) == INVALID
    assert distances(130, 2, x, 3, None) == INVALID
    assert distances(130, 2, x, 2, out) == INVALID and "x_stride" in _lib.last_error()
    assert distances(130, 32769, x, 3, out) == TOO_LARGE
    assert distances(2**32, 2, x, 2**26, out) == TOO_LARGE
    assert np.all(out == 77)
    # the handle calls: a null handle (a `which` above 1 needs a handle, so a device: test_gpu_chain_scores.py)
    assert lib.asp_sa_chains_scores(None, ctypes.c_uint32(0), ctypes.c_uint64(0), None, None, None, None, None,
                                    None) == INVALID
    assert lib.asp_sa_chains_distances(None, ctypes.c_uint32(0), None) == INVALID


def test_nothing_to_do_needs_no_device():
    from annealing_sign_problem_amd import _lib, scores

    lib = _lib.load()
    touched = _lib.gpu_touched()
    x, exact, weights = _valid()
    rc, _, untouched = _scores(130, 0, None, 0, 130, None, exact, weights)
    assert (rc, untouched) == (0, True)
    assert lib.asp_sign_scores_batch(None, ctypes.c_uint32(0)) == 0
    items = (_lib.SignScoresItem * 2)()  # a batch whose items all have no configurations
    for item in items:
        item.num_spins, item.count, item.num_scored = 130, 0, 130
        item.exact, item.weights = exact.ctypes.data, weights.ctypes.data
    assert lib.asp_sign_scores_batch(items, ctypes.c_uint32(2)) == 0
    assert lib.asp_sign_distances(ctypes.c_uint64(130), ctypes.c_uint32(0), None, ctypes.c_uint64(0), None) == 0
    assert scores.sign_scores_batch([]) == []
    assert scores.sign_distances(np.zeros((0, 3), dtype=np.uint64), 130).shape == (0, 0)
    matches, signed, total = scores.sign_scores(np.zeros((0, 3), dtype=np.uint64), exact, weights)
    assert matches.shape == signed.shape == (0,)
    assert _lib.gpu_touched() == touched
    # a refusal of the Python layer: the arguments do not fit one another
    with pytest.raises(ValueError):
        scores.sign_scores(x, exact, weights[:100], number_spins=130)
    with pytest.raises(ValueError):
        scores.sign_scores(x, exact, None, select=np.arange(5))
    with pytest.raises(ValueError):
        scores.sign_scores(x[:, :2], exact, weights)


def test_fails_loudly_without_a_device():
    from annealing_sign_problem_amd import _lib, scores

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    x, exact, weights = _valid()
    with pytest.raises(_lib.AspError) as err:
        scores.sign_scores(x, exact, weights)
    assert err.value.code == -1
    with pytest.raises(_lib.AspError):
        scores.sign_distances(x, 130)
