"""The cases of tests/test_grow_cases.py and tests/test_gpu_grow.py: the growth of many sampled clusters in one call,
specification ASP-GROW-1 (csrc/cluster_grow.hip), and TWO restatements of its law over the host
action ``operators.Operator.batched_apply`` with the draws of ``accept_cases.philox``:

(a) :func:`grow_law`, the pass form of the specification, vectorised;
(b) :func:`grow_loop`, the reference's state-by-state loop (children_of, spins.add, break, one union per child) with
    two changes only: ``for child in sorted(children)``, and the draw keyed (i, k, t, id), i the position of the child
    in ``sorted(set(children))``.

A helper module like tests/level_cases.py: no fixtures, no files, nothing compiled, no GPU.  The keyword arguments of
the laws switch on the WRONG variants.  A segment's law is computed once and shared.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np

import accept_cases
import eloc_cases
import symmetry_cases
from field_cases import first_bonds, model_operator

U64 = np.uint64
WAVE = 64
GROW_TILE = 256          # kThreads of cluster_grow.hip: k_grow_stop scans a frontier in tiles of so many states
WORDS = 1 << 32


def threshold_of(p):
    """floor(p * 2^32): the product is exact, p = 1 keeps every word and p = 0 none."""
    return int(p * 4294967296.0)


# ==================================================================================================
# operators
# ==================================================================================================
def _ring22_minus():
    return symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"]).operator


OPERATORS = {
    "kagome16": lambda: model_operator("heisenberg_kagome_16"),
    "sk16": lambda: model_operator("sk_16_1"),
    "kagome16 three bonds": lambda: first_bonds("heisenberg_kagome_16", 3),
    "kagome18 inversion -1": lambda: model_operator("heisenberg_kagome_18", -1),
    "ring22 inversion -1": _ring22_minus,
    "ring64": lambda: eloc_cases.table("ring64 bit 63").operator,
}


@functools.lru_cache(maxsize=None)
def operator(name):
    return OPERATORS[name]()


def connections(op, states):
    """``(targets u64[N], counts i64[n], valid bool[N])`` of the host action: per state its own state first, then its
    connections in term order; in a symmetry-adapted basis the representatives, ``valid`` false for a target of norm 0.
    A source of norm 0 raises ValueError (batched_apply)."""
    other, _, counts = op.batched_apply(np.asarray(states, dtype=U64))
    targets = np.ascontiguousarray(other[:, 0], dtype=U64)
    group = getattr(op.basis, "group", None)
    if group is None:
        return targets, np.asarray(counts, dtype=np.int64), np.ones(targets.shape[0], dtype=bool)
    _, _, norm = group.state_info(targets)
    return targets, np.asarray(counts, dtype=np.int64), norm > 0


def in_sorted(values, haystack):
    if haystack.shape[0] == 0:
        return np.zeros(values.shape[0], dtype=bool)
    at = np.minimum(np.searchsorted(haystack, values), haystack.shape[0] - 1)
    return haystack[at] == values


def words(i, k, t, stream, seed):
    """uint64[...]: word 0 of Philox4x32-10(counter (i, k, t, stream), key (seed lo, seed hi))."""
    return accept_cases.philox(i, k, t, stream, seed)[..., 0].astype(U64)


# ==================================================================================================
# (a) the pass form
# ==================================================================================================
@dataclass
class Pass:
    frontier: np.ndarray      # F_t
    before: np.ndarray        # M before the pass
    grows: np.ndarray         # bool[|F_t|]
    stop: object              # int or None
    applied: int


def grow_law(op, s0, size, stream, p, seed, *, index=0, trace=None, no_earlier=False, stop_on_positions=False,
             stop_applied=False, draw_le=False, keyed_by_index=False):
    """``(members u64 ascending, passes)`` of ASP-GROW-1 for one segment; ``index`` is the segment's place in its call
    (only the WRONG variant looks at it); ``trace``: a list that receives one :class:`Pass` per pass."""
    threshold = threshold_of(p)
    key = index if keyed_by_index else stream          # WRONG: the draw keyed by the call's segment index
    members = np.array([s0], dtype=U64)
    frontier = np.array([s0], dtype=U64)
    t = 0
    while frontier.size:
        grows = ~in_sorted(frontier, members)
        if stop_on_positions:                          # WRONG: every frontier state counts
            reach = members.size + np.arange(1, frontier.size + 1)
            if t == 0:
                reach = reach - 1
        else:
            reach = members.size + np.cumsum(grows)
        full = np.flatnonzero(reach >= size)
        ends = full.size > 0
        stop = int(full[0]) if ends else None
        added = frontier[:stop + 1][grows[:stop + 1]] if ends else frontier[grows]
        applied = (stop + (1 if stop_applied else 0)) if ends else frontier.size   # WRONG: the source at stop too
        if trace is not None:
            trace.append(Pass(frontier, members, grows, stop, applied))
        upcoming = np.zeros(0, dtype=U64)
        if applied and not ends:                       # (what an ending pass draws reaches no output)
            targets, counts, valid = connections(op, frontier[:applied])
            i = np.repeat(np.arange(applied), counts)
            k = np.arange(targets.size) - np.repeat(np.cumsum(counts) - counts, counts)
            at = np.searchsorted(frontier, targets)
            here = frontier[np.minimum(at, frontier.size - 1)] == targets
            member = in_sorted(targets, members)
            if not no_earlier:                         # WRONG without: the states added earlier in this pass
                member |= here & (at <= i)
            candidate = np.flatnonzero(valid & ~member)
            w = words(i[candidate], k[candidate], t, key, seed)
            kept = candidate[(w <= U64(threshold)) if draw_le else (w < U64(threshold))]   # WRONG: <=
            upcoming = np.unique(targets[kept])
        members = np.union1d(members, added)
        frontier = upcoming
        t += 1
    return members, t


# ==================================================================================================
# (b) the reference's loop
# ==================================================================================================
def grow_loop(op, s0, size, stream, p, seed):
    """The reference's create_small_cluster_around_point, state by state, with ``sorted(children)`` and the draw
    keyed (i, k, t, id)."""
    threshold = threshold_of(p)
    spins = {int(s0)}

    def children_of(state, i, t):
        targets, _, valid = connections(op, [state])
        ks = [k for k, x in enumerate(targets.tolist()) if valid[k] and x not in spins]
        w = words(i, np.array(ks, dtype=np.int64), t, stream, seed)   # (one draw per candidate, all at once)
        return {int(targets[k]) for k, word in zip(ks, w.tolist()) if word < threshold}

    children = children_of(int(s0), 0, 0) if size > 1 else set()
    t = 1
    while len(spins) < size and len(children) > 0:
        new_children = set()
        for i, child in enumerate(sorted(children)):
            spins.add(child)
            if len(spins) >= size:
                break
            new_children |= children_of(child, i, t)
        children = new_children
        t += 1
    return np.array(sorted(spins), dtype=U64), t


def breadth_first(op, s0, size):
    """Independent of both: the truncated breadth-first search in ascending order (what p = 1 gives)."""
    seen, level = [int(s0)], [int(s0)]
    while level and len(seen) < size:
        found = set()
        for state in level:
            targets, _, valid = connections(op, [state])
            found |= {x for x, ok in zip(targets.tolist(), valid) if ok}
        level = sorted(found - set(seen))
        seen += level[:size - len(seen)]
    return np.array(sorted(seen), dtype=U64)


# ==================================================================================================
# cases: calls of several segments
# ==================================================================================================
@dataclass(frozen=True)
class Call:
    name: str
    op: str
    seeds: Tuple[int, ...]
    sizes: Tuple[int, ...]
    ids: Tuple[int, ...]
    p: float
    seed: int

    @property
    def operator(self):
        return operator(self.op)

    def law(self, **switches):
        """``[(members, passes)]``, one per segment."""
        return [_segment_law(self.op, s, r, i, self.p, self.seed, g, tuple(sorted(switches.items())))
                for g, (s, r, i) in enumerate(zip(self.seeds, self.sizes, self.ids))]

    def loop(self):
        return [grow_loop(self.operator, s, r, i, self.p, self.seed)
                for s, r, i in zip(self.seeds, self.sizes, self.ids)]


@functools.lru_cache(maxsize=None)
def _segment_law(op, s0, size, stream, p, seed, index, switches):
    switches = dict(switches)
    if not switches.get("keyed_by_index"):
        index = 0            # the law does not look at it: one computation for every place in a call
    return grow_law(operator(op), s0, size, stream, p, seed, index=index, **switches)


def trace_of(op, s0, size, stream, p, seed):
    trace = []
    grow_law(operator(op), s0, size, stream, p, seed, trace=trace)
    return trace


NEEL16 = 0x5555            # 16 sites, 8 up
STRIPES16 = 0x0F0F
SEED = 0x1234_5678_9ABC_DEF1


def _one(name, op, s0, size, stream=0, p=0.5, seed=SEED):
    return Call(name, op, (s0,), (size,), (stream,), p, seed)


def _last_of_a_frontier():
    """The size is reached exactly on the LAST state of a frontier (which grows)."""
    trace = trace_of("kagome16", NEEL16, 10 ** 6, 3, 0.5, SEED)
    for t, one in enumerate(trace[1:], start=1):
        if one.grows[-1] and one.frontier.size > 2:
            size = one.before.size + int(one.grows.sum())
            call = _one("size reached on the last state of frontier %d" % t, "kagome16", NEEL16, size, 3)
            last = trace_of("kagome16", NEEL16, size, 3, 0.5, SEED)[t]
            assert last.stop == last.frontier.size - 1
            return call
    raise AssertionError("no such pass")


def _members_do_not_count():
    """High keep probability: a frontier holds states that were added later in the pass before, and the size is
    reached only because they do not count — counting frontier positions would stop earlier."""
    p = 0.9375
    trace = trace_of("kagome16", NEEL16, 10 ** 6, 7, p, SEED)
    for t, one in enumerate(trace[1:], start=1):
        stale = np.flatnonzero(~one.grows)
        later = np.flatnonzero(one.grows)
        if stale.size and later.size and later[-1] > stale[0]:
            j = int(later[later > stale[0]][0])                      # a growing state behind a member
            size = one.before.size + int(one.grows[:j + 1].sum())
            assert stale[0] < j and one.before.size + j + 1 > size   # positions would reach the size before j
            return Call("frontier states that are members do not count (pass %d)" % t, "kagome16", (NEEL16,), (size,),
                        (7,), p, SEED)
    raise AssertionError("no frontier with a member in it")


def first_candidate(op, s0, stream, seed):
    """``(target, word)`` of the first candidate of pass 0: the seed's first connection of non-zero norm."""
    targets, _, valid = connections(operator(op), [s0])
    k = int(np.flatnonzero(valid & (targets != U64(s0)))[0])
    return int(targets[k]), int(words(0, k, 0, stream, seed))


def boundary_calls():
    """The decision boundary: p = w0 / 2^32 drops the first candidate of pass 0, p = (w0 + 1) / 2^32 keeps it (both
    exact doubles).  The size is that of {seed} + F_1, so that the members are exactly those."""
    x, w0 = first_candidate("kagome16", NEEL16, 11, SEED)
    calls = []
    for w in (w0, w0 + 1):
        p = w / WORDS
        assert threshold_of(p) == w
        first = trace_of("kagome16", NEEL16, 10 ** 6, 11, p, SEED)
        size = 1 + max(first[1].frontier.size if len(first) > 1 else 0, 1)
        calls.append(Call("boundary: threshold = w0 + %d" % (w - w0), "kagome16", (NEEL16,), (size,), (11,), p, SEED))
    return x, calls


def _mixed_passes():
    """Segments that end in passes 0, 1, 2 and later side by side (and a frontier that dies early)."""
    sizes = (1, 2, 1, 9, 40, 2, 300, 25)
    return Call("ends in passes 0, 1, 2 and later", "kagome16", (NEEL16, STRIPES16) * 4, sizes, tuple(range(8)), 0.5,
                SEED)


EIGHT = Call("eight segments", "kagome16", (NEEL16, STRIPES16, 0x00FF, 0x3333, NEEL16, 0xF00F, 0x0FF0, 0xAAAA),
             (30, 77, 5, 130, 64, 1, 257, 18), (40, 41, 42, 43, 44, 45, 46, 47), 0.5, SEED)


def _ring22_norm0():
    """Inversion -1 with lattice symmetries: rows that reach orbits of norm 0, which are skipped."""
    e = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    bounds = np.concatenate([[0], np.cumsum(e.counts)])
    rows = [r for r in range(e.keys.size) if np.any(e.target_norm[bounds[r]:bounds[r + 1]] == 0)]
    assert rows
    seeds = tuple(int(e.keys[r]) for r in rows[:3])
    call = Call("ring22 inversion -1: norm-0 targets", "ring22 inversion -1", seeds, (60, 9, 130), (0, 1, 2), 0.75, SEED)
    for s in seeds:     # pass 0 itself meets a target of norm 0
        assert not connections(call.operator, [s])[2].all()
    return call


def norm0_state():
    """A state outside the -1 sector of the 22-site ring (norm 0)."""
    e = symmetry_cases.expected(symmetry_cases.BY_NAME["ring22 inversion -1"])
    raw = e.raw_targets[e.target_norm == 0]
    rep, _, norm = e.operator.basis.group.state_info(raw[:1])
    assert norm[0] == 0
    return int(rep[0])


def _ring64():
    t = eloc_cases.table("ring64 bit 63")
    high = [int(k) for k in t.keys if int(k) >> 63][:2]
    low = [int(k) for k in t.keys if not int(k) >> 63][:1]
    assert high and low
    seeds = tuple(high + low)
    return Call("64 sites, seeds with bit 63", "ring64", seeds, (70, 5, 33)[:len(seeds)], tuple(range(len(seeds))),
                0.5, SEED)


@functools.lru_cache(maxsize=None)
def calls():
    sk = "sk16"
    out = [
        _one("size 1", "kagome16", NEEL16, 1),
        _one("size 2: stop is the first frontier state", "kagome16", NEEL16, 2),
        _last_of_a_frontier(),
        _members_do_not_count(),
        _one("the frontier dies before the size: the component at p = 1", "kagome16 three bonds", NEEL16, 1000, p=1.0),
        _one("keep probability 0", "kagome16", NEEL16, 50, p=0.0),
        _one("keep probability 1", "kagome16", NEEL16, 50, p=1.0),
        # rows of 65 connections at p = 1: frontiers of 64 and of thousands of states, member tables across 64, 256
        Call("frontiers and member tables across %d, %d and the tile" % (WAVE, GROW_TILE), sk, (NEEL16,) * 8,
             (WAVE, WAVE + 1, WAVE + 2, GROW_TILE, GROW_TILE + 1, GROW_TILE + 2, 2 * GROW_TILE + 1, 1500),
             tuple(range(8)), 1.0, SEED),
        Call("frontiers across the tile with draws", sk, (NEEL16, STRIPES16, NEEL16), (GROW_TILE + 3, 700, 63),
             (9, 8, 7), 0.5, SEED),
        _mixed_passes(),
        Call("one seed: equal ids, different ids", "kagome16", (NEEL16,) * 4, (60,) * 4, (5, 5, 6, 5), 0.5, SEED),
        EIGHT,
        Call("kagome18 inversion -1", "kagome18 inversion -1", (0b010101010101010101, 0b000000000111111111),
             (90, 300), (1, 0), 0.5, SEED),
        _ring22_norm0(),
        _ring64(),
    ]
    out += boundary_calls()[1]
    return tuple(out)


def call(name):
    for c in calls():
        if c.name.startswith(name):
            return c
    raise KeyError(name)


VARIANTS = {
    "membership without the states added earlier in the pass": dict(no_earlier=True),
    "stop counted on frontier positions": dict(stop_on_positions=True),
    "the draw compared with <=": dict(draw_le=True),
    "the draw keyed by the call's segment index": dict(keyed_by_index=True),
}
# The source at stop applied too: the pass ENDS the segment, so what it draws reaches neither the members nor the
# number of passes.  No result can tell this variant from the law; tests/test_grow_cases.py asserts exactly that.
UNOBSERVABLE = {"the source at stop applied too": dict(stop_applied=True)}


def same(got, want):
    """Members and passes of every segment, bit for bit."""
    return len(got) == len(want) and all(
        np.array_equal(np.asarray(a, dtype=U64), b) and int(x) == int(y) for (a, x), (b, y) in zip(got, want))
