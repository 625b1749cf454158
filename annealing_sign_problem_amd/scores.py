"""Sign scores on the GPU (csrc/sign_scores.hip, specification ASP-SCORE-1 in DESIGN.md §3.11): how many
of the recovered signs agree with the exact ones and how large the weighted overlap is — what
``common.compute_accuracy_and_overlap`` (common.py:211-229 of the reference) computes on the host for one
configuration —, for many configurations of a model, for many models in one call, and the Hamming
distances between configurations.  ``annealer.Chains.scores`` / ``.distances`` are the same for the
configurations resident in a chains handle.

Signs are packed as everywhere else (``annealer.signs_to_bits``: bit ``i`` of word ``i // 64`` set means
``s_i = +1``).  ``matches`` is an exact integer; ``signed`` and ``total`` are the pairwise tree of the
specification (``tree_sum`` in tests/score_cases.py restates it in numpy), bit for bit, whatever the launch.

Consensus signs (csrc/sign_vote.hip, law ASP-VOTE-1 in DESIGN.md §3.12; not in the reference): the
configurations of a model aligned up to the global flip and a weighted vote per site — :func:`consensus`,
:func:`consensus_batch` for many models in one call, ``annealer.Chains.consensus`` and
``annealer.consensus_chains`` for resident chains; tests/vote_cases.py restates the law in numpy.
No CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

__all__ = ["sign_scores", "sign_scores_batch", "accuracy_and_overlap", "accuracy_and_overlap_batch",
           "accuracy_and_overlap_each", "sign_distances", "accuracy_and_overlap_of", "last_ms", "Consensus",
           "consensus", "consensus_batch", "vote_weights", "vote_last_ms"]

# asp_sign_scores_item as a numpy record (checked against the ctypes mirror where it is used)
_ITEM_RECORD = np.dtype([("num_spins", "<u8"), ("count", "<u4"), ("_pad", "<u4"), ("x", "<u8"), ("x_stride", "<u8"),
                         ("num_scored", "<u8"), ("select", "<u8"), ("exact", "<u8"), ("weights", "<u8"),
                         ("out_matches", "<u8"), ("out_signed", "<u8"), ("out_total", "<u8")])


class _Item:
    """The checked arrays of one model of a scoring call (kept alive over the call)."""

    def __init__(self, xs, exact, weights=None, select=None, number_spins=None, resident: bool = False):
        if select is not None:
            select = np.ascontiguousarray(select, dtype=np.int32).reshape(-1)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if number_spins is None:
            if select is not None or weights is None:
                raise ValueError("'number_spins' is needed without 'weights' and with 'select'")
            number_spins = weights.shape[0]
        self.number_spins = int(number_spins)
        if self.number_spins < 0:
            raise ValueError("'number_spins' must not be negative")
        self.scored = self.number_spins if select is None else select.shape[0]
        if weights is not None and weights.shape[0] != self.scored:
            raise ValueError("'weights' must hold {} values, one per scored position".format(self.scored))
        exact = np.ascontiguousarray(exact, dtype=np.uint64).reshape(-1)
        if exact.shape[0] * 64 < self.scored:
            raise ValueError("'exact' holds fewer than {} signs".format(self.scored))
        self.words = (self.number_spins + 63) // 64
        self.exact = exact if exact.shape[0] else np.zeros(1, dtype=np.uint64)
        self.weights, self.select = weights, select
        if select is not None and select.shape[0] == 0:
            self.select = np.zeros(1, dtype=np.int32)  # (never read; NULL would mean the identity)
        if resident:
            return
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        if xs.ndim == 1:
            xs = xs.reshape(1, -1)
        if xs.ndim != 2:
            raise ValueError("'xs' must be packed configurations [count, words] or one of them [words]")
        if xs.shape[1] < self.words:
            raise ValueError("'xs' holds fewer than {} spins per configuration".format(self.number_spins))
        self.count = xs.shape[0]
        self.stride = xs.shape[1]
        self.xs = xs if xs.size else np.zeros(1, dtype=np.uint64)

    def _outputs(self, count: int) -> None:
        self.matches = np.zeros(count, dtype=np.uint64)
        self.signed = np.zeros(count, dtype=np.float64)
        self.total = np.zeros(1, dtype=np.float64)

    def result(self) -> Tuple[np.ndarray, np.ndarray, float]:
        return self.matches, self.signed, float(self.total[0])

    def fill(self, item: "_lib.SignScoresItem", matches: int, signed: int, total: int) -> None:
        """The C item, with the addresses of this item's share of the call's output arrays."""
        item.num_spins = self.number_spins
        item.count = self.count
        item.x = _address(self.xs)
        item.x_stride = self.stride
        item.num_scored = self.scored
        item.select = None if self.select is None else _address(self.select)
        item.exact = _address(self.exact)
        item.weights = None if self.weights is None else _address(self.weights)
        item.out_matches = matches
        item.out_signed = signed
        item.out_total = total


def _address(array: np.ndarray) -> int:
    # (array.ctypes.data builds a ctypes object per look: several microseconds an item in a round of
    # a thousand small models, as much as scoring one of them on the host)
    return array.__array_interface__["data"][0]


def accuracy_and_overlap_of(matches, signed, total, scored) -> Tuple[np.ndarray, np.ndarray]:
    """``(accuracy, overlap)`` from the scores: ``a = matches / K0``, ``accuracy = max(a, 1 - a)`` (bit for
    bit ``compute_accuracy_and_overlap``'s) and ``overlap = |signed| / total`` (NaN when the weights sum
    to zero, as on the host)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.asarray(matches, dtype=np.float64) / np.asarray(scored, dtype=np.float64)
        accuracy = np.maximum(a, 1 - a)
        overlap = np.abs(np.asarray(signed, dtype=np.float64)) / np.asarray(total, dtype=np.float64)
    return accuracy, overlap


def sign_scores(xs, exact, weights=None, select=None, number_spins=None):
    """``(matches uint64[C], signed float64[C], total)`` of the configurations ``xs`` (``[C, words]``, or
    one ``[words]``) of a ``number_spins``-spin model against ``exact`` and ``weights``: position ``i``
    compares bit ``select[i]`` of a configuration with bit ``i`` of ``exact`` (``select=None``: the
    identity); ``weights=None``: all 1.  ``number_spins`` defaults to ``len(weights)``."""
    item = _Item(xs, exact, weights, select, number_spins)
    item._outputs(item.count)
    lib = _lib.load()
    _lib.check(lib.asp_sign_scores(ctypes.c_uint64(item.number_spins), ctypes.c_uint32(item.count), _lib.ptr(item.xs),
                                   ctypes.c_uint64(item.stride), ctypes.c_uint64(item.scored), _lib.ptr(item.select),
                                   _lib.ptr(item.exact), _lib.ptr(item.weights), _lib.ptr(item.matches),
                                   _lib.ptr(item.signed), _lib.ptr(item.total)))
    return item.result()


def _as_item(entry) -> _Item:
    if isinstance(entry, dict):
        return _Item(**entry)
    return _Item(*entry)


def _run_batch(items: Sequence[_Item]):
    """One asp_sign_scores_batch call; every item's outputs are views of three arrays of the call, which
    are returned with the items' first positions in them: ``(first, matches, signed, total)``."""
    n = len(items)
    raw = (_lib.SignScoresItem * max(n, 1))()
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([item.count for item in items], out=first[1:])
    matches = np.zeros(max(int(first[-1]), 1), dtype=np.uint64)
    signed = np.zeros(max(int(first[-1]), 1), dtype=np.float64)
    total = np.zeros(max(n, 1), dtype=np.float64)
    at_matches, at_signed, at_total = _address(matches), _address(signed), _address(total)
    for k, (slot, item) in enumerate(zip(raw, items)):
        begin, end = int(first[k]), int(first[k + 1])
        item.matches, item.signed, item.total = matches[begin:end], signed[begin:end], total[k:k + 1]
        item.fill(slot, at_matches + 8 * begin, at_signed + 8 * begin, at_total + 8 * k)
    _lib.check(_lib.load().asp_sign_scores_batch(raw, ctypes.c_uint32(n)))
    return first, matches[:first[-1]], signed[:first[-1]], total[:n]


def sign_scores_batch(items) -> list:
    """``[sign_scores(*item) for item in items]`` in ONE device call (``asp_sign_scores_batch``: one upload,
    one launch, one download), the same bits.  An item is the tuple of :func:`sign_scores`' arguments, or
    a dict of them."""
    items = [_as_item(entry) for entry in items]
    _run_batch(items)
    return [item.result() for item in items]


def accuracy_and_overlap(xs, exact, weights=None, number_spins=None, select=None):
    """``(accuracy float64[C], overlap float64[C])`` of the configurations ``xs``: for one configuration
    the accuracy IS ``common.compute_accuracy_and_overlap``'s and the overlap is within
    ``(K0 + 64) * 2**-53`` of it."""
    item = _Item(xs, exact, weights, select, number_spins)
    _run_batch([item])
    return accuracy_and_overlap_of(item.matches, item.signed, item.total[0], item.scored)


def accuracy_and_overlap_batch(items) -> list:
    """:func:`accuracy_and_overlap` of every item (tuples ``(xs, exact, weights, number_spins, select)`` or
    dicts) in one device call."""
    made = []
    for entry in items:
        if isinstance(entry, dict):
            made.append(_Item(**entry))
        else:
            xs, exact, weights, number_spins, select = (tuple(entry) + (None,) * 3)[:5]
            made.append(_Item(xs, exact, weights, select, number_spins))
    first, matches, signed, total = _run_batch(made)
    # (the two divisions for the whole batch at once: element by element what they are item by item)
    counts = np.diff(first)
    accuracy, overlap = accuracy_and_overlap_of(matches, signed, np.repeat(total, counts),
                                                np.repeat(np.array([m.scored for m in made], dtype=np.float64), counts))
    return [(accuracy[first[k]:first[k + 1]], overlap[first[k]:first[k + 1]]) for k in range(len(made))]


def accuracy_and_overlap_each(predicted_list, exact_list, weights_list) -> Tuple[np.ndarray, np.ndarray]:
    """``(accuracy float64[n], overlap float64[n])`` of ONE configuration per model, model ``k`` of
    ``len(weights_list[k])`` spins, in one device call — the shape of a round of cluster solutions:
    thousands of small models.  The same call and the same bits as :func:`accuracy_and_overlap_batch`,
    but the items are laid out with array arithmetic over three concatenated inputs: filling a ctypes
    item field by field takes as long per model as scoring a few hundred spins on the host."""
    assert _ITEM_RECORD.itemsize == ctypes.sizeof(_lib.SignScoresItem)
    n = len(weights_list)
    if not (len(predicted_list) == len(exact_list) == n):
        raise ValueError("lists of different lengths")
    if n == 0:
        return np.zeros(0), np.zeros(0)
    weights = [np.asarray(w, dtype=np.float64).reshape(-1) for w in weights_list]
    sizes = np.array([w.shape[0] for w in weights], dtype=np.int64)
    words = (sizes + 63) // 64

    def leading_words(arrays, what: str) -> np.ndarray:
        parts = []
        for array, count in zip(arrays, words):
            array = np.asarray(array, dtype=np.uint64).reshape(-1)
            if array.shape[0] < count:
                raise ValueError("{} holds fewer than {} words".format(what, count))
            parts.append(array[:count])
        return np.concatenate(parts)

    xs, exact = leading_words(predicted_list, "'predicted'"), leading_words(exact_list, "'exact'")
    weights = np.concatenate(weights)
    first_word, first_weight = np.cumsum(words) - words, np.cumsum(sizes) - sizes
    matches, signed, total = np.zeros(n, dtype=np.uint64), np.zeros(n), np.zeros(n)
    items = np.zeros(n, dtype=_ITEM_RECORD)
    items["num_spins"] = items["num_scored"] = sizes
    items["count"] = 1
    items["x"] = _address(xs) + 8 * first_word
    items["x_stride"] = words
    items["exact"] = _address(exact) + 8 * first_word
    items["weights"] = _address(weights) + 8 * first_weight
    step = 8 * np.arange(n)
    items["out_matches"], items["out_signed"] = _address(matches) + step, _address(signed) + step
    items["out_total"] = _address(total) + step
    _lib.check(_lib.load().asp_sign_scores_batch(
        ctypes.cast(_address(items), ctypes.POINTER(_lib.SignScoresItem)), ctypes.c_uint32(n)))
    return accuracy_and_overlap_of(matches, signed, total, sizes)


def sign_distances(xs, number_spins: int) -> np.ndarray:
    """``uint32[C, C]``: the Hamming distances between the configurations ``xs[C, words]`` over their first
    ``number_spins`` bits.  The distance up to a global flip is ``np.minimum(D, number_spins - D)``."""
    xs = np.ascontiguousarray(xs, dtype=np.uint64)
    if xs.ndim != 2:
        raise ValueError("'xs' must be packed configurations [count, words]")
    number_spins = int(number_spins)
    if number_spins < 0 or xs.shape[1] * 64 < number_spins:
        raise ValueError("'xs' holds fewer than {} spins per configuration".format(number_spins))
    count = xs.shape[0]
    # (above the library's limit the call is made for its refusal: no 4 GiB matrix first)
    out = np.zeros((count, count), dtype=np.uint32) if count <= 32768 else np.zeros(1, dtype=np.uint32)
    _lib.check(_lib.load().asp_sign_distances(ctypes.c_uint64(number_spins), ctypes.c_uint32(min(count, 0xFFFFFFFF)),
                                              _lib.ptr(xs if xs.size else np.zeros(1, dtype=np.uint64)),
                                              ctypes.c_uint64(xs.shape[1]), _lib.ptr(out if count else None)))
    return out


def last_ms() -> float:
    """Device time (ms) of the kernels of this thread's last scoring or distance call, copies excluded."""
    return float(_lib.load().asp_sign_scores_last_ms())


# ---- consensus signs (csrc/sign_vote.hip, law ASP-VOTE-1) ----

@dataclasses.dataclass
class Consensus:
    """What a vote returns (law ASP-VOTE-1): the consensus configuration ``x`` (``uint64[W]``, tail bits 0),
    per site ``ones`` (``uint32[K]``: the aligned configurations with the bit set), ``plus`` / ``minus``
    (``float64[K]``: their weights and the others', summed in ascending order of the configurations) and
    ``margin = (plus - minus) / (plus + minus)`` (computed on the host; 0 where nothing has weight), per
    configuration ``flipped`` (``bool[R]``) and ``distance`` (``uint32[R]``, to the last round's reference,
    before the flip), and ``changed``: the sites on which ``x`` differs from the last round's reference
    (0: a fixed point).  ``energy``: the Ising energy of ``x``, where a Hamiltonian was at hand."""
    x: np.ndarray
    ones: np.ndarray
    plus: np.ndarray
    minus: np.ndarray
    margin: np.ndarray
    flipped: np.ndarray
    distance: np.ndarray
    changed: int
    energy: Optional[float] = None


class _Vote:
    """The checked inputs and the outputs of one item of a vote (kept alive over the call)."""

    def __init__(self, number_spins, count, weights=None, ref=None, anchor=0, align=True, rounds=1, xs=None):
        self.number_spins, self.count = int(number_spins), int(count)
        if self.number_spins < 0:
            raise ValueError("'number_spins' must not be negative")
        self.words = (self.number_spins + 63) // 64
        self.stride = 0
        self.xs = None
        if xs is not None:
            xs = np.ascontiguousarray(xs, dtype=np.uint64)
            if xs.ndim != 2:
                raise ValueError("'xs' must be packed configurations [count, words]")
            if xs.shape[1] < self.words:
                raise ValueError("'xs' holds fewer than {} spins per configuration".format(self.number_spins))
            self.count, self.stride = xs.shape[0], xs.shape[1]
            self.xs = xs if xs.size else np.zeros(1, dtype=np.uint64)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if weights.shape[0] != self.count:
                raise ValueError("'weights' must hold {} values, one per configuration".format(self.count))
            if weights.shape[0] == 0:
                weights = None
        if ref is not None:
            ref = np.ascontiguousarray(ref, dtype=np.uint64).reshape(-1)
            if ref.shape[0] < self.words:
                raise ValueError("'ref' holds fewer than {} spins".format(self.number_spins))
            if ref.shape[0] == 0:
                ref = np.zeros(1, dtype=np.uint64)  # (never read; NULL would mean x[anchor])
        anchor, rounds = int(anchor), int(rounds)
        if not (0 <= anchor < 2**32 and 0 <= rounds < 2**32):
            raise ValueError("'anchor' and 'rounds' must fit 32 bits")
        self.weights, self.ref, self.anchor, self.align, self.rounds = weights, ref, anchor, bool(align), rounds
        self.distance = np.zeros(self.count, dtype=np.uint32)
        self.flipped = np.zeros(self.count, dtype=np.uint8)
        self.ones = np.zeros(self.number_spins, dtype=np.uint32)
        self.plus = np.zeros(self.number_spins, dtype=np.float64)
        self.minus = np.zeros(self.number_spins, dtype=np.float64)
        self.x = np.zeros(self.words, dtype=np.uint64)
        self.changed = np.zeros(1, dtype=np.uint32)

    def fill(self, item) -> None:
        """The fields that asp_sign_vote_item and asp_sa_chains_vote_item share, and x where there is one."""
        if self.xs is not None:
            item.num_spins = self.number_spins
            item.count = self.count
            item.x = _address(self.xs)
            item.x_stride = self.stride
        item.weights = None if self.weights is None else _address(self.weights)
        item.ref = None if self.ref is None else _address(self.ref)
        item.anchor, item.align, item.rounds = self.anchor, int(self.align), self.rounds
        item.out_distance = _address(self.distance) if self.count else None
        item.out_flipped = _address(self.flipped) if self.count else None
        item.out_ones = _address(self.ones) if self.number_spins else None
        item.out_plus = _address(self.plus) if self.number_spins else None
        item.out_minus = _address(self.minus) if self.number_spins else None
        item.out_consensus = _address(self.x) if self.words else None
        item.out_changed = _address(self.changed)

    def result(self) -> Consensus:
        total = self.plus + self.minus
        margin = np.zeros_like(total)
        np.divide(self.plus - self.minus, total, out=margin, where=total != 0)
        return Consensus(self.x, self.ones, self.plus, self.minus, margin, self.flipped.astype(bool), self.distance,
                         int(self.changed[0]))


def _as_vote(entry) -> _Vote:
    if isinstance(entry, dict):
        entry = dict(entry)
        return _Vote(entry.pop("number_spins"), 0, xs=entry.pop("xs"), **entry)
    xs, number_spins, *rest = entry
    return _Vote(number_spins, 0, *rest, xs=xs)


def consensus_batch(items) -> list:
    """``[consensus(*item) for item in items]`` in ONE device call (``asp_sign_vote_batch``: one upload, two
    launches a round whatever the number of items, one download), the same bits.  An item is the tuple of
    :func:`consensus`' arguments, or a dict of them."""
    votes = [_as_vote(entry) for entry in items]
    raw = (_lib.SignVoteItem * max(len(votes), 1))()
    for slot, vote in zip(raw, votes):
        vote.fill(slot)
    _lib.check(_lib.load().asp_sign_vote_batch(raw, ctypes.c_uint32(len(votes))))
    return [vote.result() for vote in votes]


def consensus(xs, number_spins, weights=None, ref=None, anchor=0, align=True, rounds=1) -> Consensus:
    """The vote of law ASP-VOTE-1 over the configurations ``xs[R, words]`` of a
    ``number_spins``-spin model, on the device: every configuration is aligned with the reference (``ref``,
    packed, or ``xs[anchor]``) up to the global flip — flipped when it differs from it on more than half
    of the sites; ``align=False``: never, for models with a field — and every site takes the sign that the
    larger weight votes for (``weights``: one per configuration, ``None``: all 1; a tie takes the
    reference's).  ``rounds > 1`` repeats the vote with the consensus as the reference."""
    return consensus_batch([(xs, number_spins, weights, ref, anchor, align, rounds)])[0]


def vote_weights(energies, beta=None) -> np.ndarray:
    """Weights of a vote from the configurations' energies: ones (``beta=None``), or the Boltzmann factors
    ``exp(-beta * (E - E.min()))``."""
    energies = np.asarray(energies, dtype=np.float64).reshape(-1)
    if beta is None or energies.shape[0] == 0:
        return np.ones(energies.shape[0], dtype=np.float64)
    return np.exp(-float(beta) * (energies - energies.min()))


def vote_last_ms() -> float:
    """Device time (ms) of the kernels of this thread's last vote, copies excluded."""
    return float(_lib.load().asp_sign_vote_last_ms())
