"""The word layout's difference bits (tests/lazy_best_cases.py) against a plain "copy on improvement" model,
on the flip / improve sequences of the very cases the GPU test runs, and on random sequences.  No GPU."""
import numpy as np
import pytest

import lazy_best_cases as lb

_events = {}


def _case(case):
    if case not in _events:
        _events[case] = lb.events_of(*case)
    return _events[case]


def _agrees(start, events, **variant):
    words, kept, cur = lb.replay(start, events, **variant)
    return all(np.array_equal(lb.best(words, m), kept[m]) and np.array_equal(lb.current(words, m), cur[m])
               for m in range(lb.M))


def _a_improves_b_stale(start, events):
    """Some sweep in which a replica improves while another one does not, has flipped in this sweep and
    differs from its own best."""
    cur, kept = start.copy(), start.copy()
    for masks, improved in events:
        flipped = [bool(((masks >> m) & 1).any()) for m in range(lb.M)]
        for m in range(lb.M):
            cur[m] ^= ((masks >> m) & 1).astype(np.uint8)
        stale = [m for m in range(lb.M) if not (improved >> m) & 1 and flipped[m] and (cur[m] != kept[m]).any()]
        if improved and stale and any(flipped[m] for m in range(lb.M) if (improved >> m) & 1):
            return True
        for m in range(lb.M):
            if (improved >> m) & 1:
                kept[m] = cur[m]
    return False


@pytest.mark.parametrize("case", lb.cases(), ids=lambda c: "%d-%s-%d" % c)
def test_words_keep_the_best_configuration(case):
    start, events = _case(case)
    assert _agrees(start, events)
    words, _, _ = lb.replay(start, events)
    for m in range(lb.M):  # the k-loop's sign byte never sees d
        assert np.array_equal(lb.sign_byte(words, m), np.where(lb.current(words, m), 0xBF, 0x3F))


def test_random_sequences():
    rng = np.random.default_rng(7)
    for _ in range(50):
        positions = int(rng.integers(1, 200))
        start = rng.integers(0, 2, size=(lb.M, positions)).astype(np.uint8)
        events = [(rng.integers(0, 16, size=positions).astype(np.uint32) * (rng.random(positions) < 0.3),
                   int(rng.integers(0, 16))) for _ in range(int(rng.integers(0, 12)))]
        events = [(m.astype(np.uint32), i) for m, i in events]
        assert _agrees(start, events)


def test_the_case_list_holds_the_telling_sweep():
    assert any(_a_improves_b_stale(*_case(c)) for c in lb.cases())


@pytest.mark.parametrize("variant", [dict(clear_variant="all"), dict(flip_variant="sign_only")],
                         ids=["clear-all-replicas", "flip-sign-bit-only"])
def test_wrong_variants_are_caught(variant):
    caught = [c for c in lb.cases() if not _agrees(*_case(c), **variant)]
    print("caught by", caught)
    assert caught, "no case of the list tells this wrong variant from the right one"


def test_no_improvement_returns_the_start():
    start, events = _case((600, "hot", 24))
    never = [(masks, 0) for masks, _ in events]
    words, kept, _ = lb.replay(start, never)
    assert np.array_equal(kept, start)
    assert all(np.array_equal(lb.best(words, m), start[m]) for m in range(lb.M))
