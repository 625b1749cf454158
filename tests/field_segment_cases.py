"""The cases of tests/test_field_segment_cases.py and tests/test_gpu_field_segments.py: the boundary fields of many
clusters in one call, specification ASP-FIELD-SEG-1 (csrc/operator_field_segments.hip), its law
and five named wrong variants of it.

A helper module like tests/field_cases.py, whose operators, clusters, environments and law it uses: no fixtures, no
files, nothing compiled, no GPU.  The law is the loop of `field_cases.field_law` over the segments — the cluster and
the environment of segment g alone — returning the concatenated field and the per-segment unresolved counts.  The
connections of a case come from the host `Operator.batched_apply` of the concatenated keys (it works key by key),
are computed once per case and shared, as is the law at every scale.
"""
import functools
from dataclasses import dataclass

import numpy as np

import field_cases
from field_cases import awkward_amplitudes, environment_of_size, field_law, grow, model_operator, positions, same_bits

__all__ = ["awkward_amplitudes", "model_operator", "same_bits"]

SCALES = (1.0, 2.0, -1.0)


# -- the law -------------------------------------------------------------------------------------------------
def _cut(offsets):
    offsets = np.asarray(offsets).astype(np.int64)
    return [(int(offsets[g]), int(offsets[g + 1])) for g in range(offsets.size - 1)]


def field_segments_law(other, coeffs, counts, keys, psi, offsets, env_keys, env_psi, env_offsets, scale, wrong=None):
    """ASP-FIELD-SEG-1: `(field f64[T], unresolved u64[S])`, segment by segment what `field_law` gives for the
    segment's keys, amplitudes and environment alone.  `other`, `coeffs`: the connections of the concatenated keys,
    `counts[r]` of them per key.  `wrong`: None, or one of "W1" ... "W5" (see WRONG)."""
    counts = np.asarray(counts).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    env_psi = np.asarray(env_psi, dtype=np.float64)
    rows, envs = _cut(offsets), _cut(env_offsets)
    if wrong == "W1":
        everyones = np.unique(keys)
    if wrong == "W2":  # every environment, a key with the amplitude of the first segment that holds it
        all_env, first = np.unique(env_keys, return_index=True)
        all_env_psi = env_psi[first]
    field = np.zeros(len(keys), dtype=np.float64)
    unresolved = np.zeros(len(rows), dtype=np.uint64)
    for g, ((lo, hi), (elo, ehi)) in enumerate(zip(rows, envs)):
        first, last = int(starts[lo]), int(starts[hi])
        seg_other, seg_psi = other[first:last], psi[lo:hi]
        seg_env, seg_env_psi = env_keys[elo:ehi], env_psi[elo:ehi]
        if wrong == "W1" and hi > lo:  # a target among ANY segment's keys counts as a hit of the cluster
            seg_other = np.where(positions(everyones, seg_other)[1], keys[lo], seg_other)
        if wrong == "W2":
            seg_env, seg_env_psi = all_env, all_env_psi
        if wrong == "W4":
            seg_psi = psi[0:hi - lo]
        if wrong == "W5":
            seg_env_psi = env_psi[0:ehi - elo]
        part, lost = field_law(seg_other, coeffs[first:last], counts[lo:hi], keys[lo:hi], seg_psi, seg_env,
                               seg_env_psi, scale)
        field[lo:hi] = part
        unresolved[g] = lost
    if wrong == "W3" and len(rows):
        unresolved[:] = [unresolved.sum()] + [0] * (len(rows) - 1)
    return field, unresolved


WRONG = {
    "W1": "the cluster probe sees every segment's keys",
    "W2": "the environment probe sees every segment's environment, with the amplitude of the first segment that "
          "holds the key",
    "W3": "unresolved is summed over the call and reported in segment 0",
    "W4": "|psi_r| is read at the segment-local row index",
    "W5": "env_psi is read at the segment-local position",
}
# the case on which each wrong variant must differ from the law
WRITTEN_FOR = {"W1": "neighbouring clusters", "W2": "one cluster, 5 draws", "W3": "a missing environment key",
               "W4": "kagome16 sizes", "W5": "kagome16 sizes"}


def equal(got, want):
    """Field as bits, unresolved per segment."""
    return bool(same_bits(got[0], want[0]) and np.array_equal(np.asarray(got[1], dtype=np.uint64),
                                                              np.asarray(want[1], dtype=np.uint64)))


# -- cases ---------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    operator: object
    keys: np.ndarray         # u64[T]: the clusters one after the other, each ascending and unique
    psi: np.ndarray          # f64[T]: signed, unit norm over every non-empty segment
    offsets: np.ndarray      # u64[S + 1]
    env_keys: np.ndarray     # u64[E]: the environments one after the other, each ascending and unique
    env_psi: np.ndarray      # f64[E]
    env_offsets: np.ndarray  # u64[S + 1]
    other: np.ndarray        # host batched_apply(keys): targets u64[N]
    coeffs: np.ndarray       # f64[N]
    counts: np.ndarray       # i64[T]

    def law(self, scale=1.0, wrong=None, psi=None, env_psi=None):
        if wrong is None and psi is None and env_psi is None and self.name in BUILDERS and case(self.name) is self:
            return _shared_law(self.name, float(scale))
        return field_segments_law(self.other, self.coeffs, self.counts, self.keys, self.psi if psi is None else psi,
                                  self.offsets, self.env_keys, self.env_psi if env_psi is None else env_psi,
                                  self.env_offsets, scale, wrong)

    @property
    def segments(self):
        return self.offsets.size - 1

    def segment(self, g):
        """`(keys, psi, env_keys, env_psi)` of segment g."""
        (lo, hi), (elo, ehi) = _cut(self.offsets)[g], _cut(self.env_offsets)[g]
        return self.keys[lo:hi], self.psi[lo:hi], self.env_keys[elo:ehi], self.env_psi[elo:ehi]

    def connections(self, g):
        """`(sources, targets, coeffs)` of segment g's rows, one entry per connection."""
        lo, hi = _cut(self.offsets)[g]
        starts = np.concatenate([[0], np.cumsum(self.counts)])
        first, last = int(starts[lo]), int(starts[hi])
        return np.repeat(self.keys[lo:hi], self.counts[lo:hi]), self.other[first:last], self.coeffs[first:last]

    def permuted(self, order):
        """The same segments in another order (the connections with them)."""
        parts = [self.segment(g) for g in order]
        links = [self.connections(g) for g in order]
        sizes = [self.counts[lo:hi] for lo, hi in (_cut(self.offsets)[g] for g in order)]
        return Case(self.name + " permuted", self.operator, _concat([p[0] for p in parts], np.uint64),
                    _concat([p[1] for p in parts], np.float64), _offsets([p[0] for p in parts]),
                    _concat([p[2] for p in parts], np.uint64), _concat([p[3] for p in parts], np.float64),
                    _offsets([p[2] for p in parts]), _concat([x[1] for x in links], np.uint64),
                    _concat([x[2] for x in links], np.float64), _concat(sizes, np.int64))


def _concat(parts, dtype):
    parts = [np.asarray(p, dtype=dtype) for p in parts]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=dtype)


def _offsets(parts):
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return offsets


def _empty():
    return np.zeros(0, dtype=np.uint64)


NATURAL = "natural"  # an environment: the one-hop extension of the cluster without the cluster


def from_segments(name, op, clusters, environments, seed, psis=None, env_psis=None):
    """A case from its clusters and environments (`NATURAL`, or sorted keys).  Amplitudes: given, or random with
    unit norm over the cluster and 0.1 x random over the environment (field_cases.make_case's)."""
    rng = np.random.default_rng(seed)
    clusters = [np.asarray(c, dtype=np.uint64) for c in clusters]
    keys, offsets = _concat(clusters, np.uint64), _offsets(clusters)
    if keys.size:
        other, coeffs, counts = op.batched_apply(keys)
        assert not np.any(coeffs.imag)
        other, coeffs = np.ascontiguousarray(other[:, 0]), np.ascontiguousarray(coeffs.real)
    else:
        other, coeffs, counts = _empty(), np.zeros(0), np.zeros(0, dtype=np.int64)
    counts = np.asarray(counts).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    envs, amplitudes, env_amplitudes = [], [], []
    for g, (cluster, env) in enumerate(zip(clusters, environments)):
        if isinstance(env, str) and env == NATURAL:
            first, last = int(starts[int(offsets[g])]), int(starts[int(offsets[g + 1])])
            seg_other, seg_coeffs = other[first:last], coeffs[first:last]
            env = np.unique(seg_other[~positions(cluster, seg_other)[1] & (seg_coeffs != 0)])
        env = np.asarray(env, dtype=np.uint64)
        envs.append(env)
        if psis is not None and psis[g] is not None:
            psi = np.asarray(psis[g], dtype=np.float64)
        else:
            psi = rng.normal(size=cluster.size) * np.exp(rng.normal(size=cluster.size))
            if cluster.size:
                psi /= np.linalg.norm(psi)
        amplitudes.append(psi)
        if env_psis is not None and env_psis[g] is not None:
            env_psi = np.asarray(env_psis[g], dtype=np.float64)
        else:
            env_psi = rng.normal(size=env.size) * np.exp(rng.normal(size=env.size)) * 0.1
        assert psi.shape == cluster.shape and env_psi.shape == env.shape
        assert np.all(cluster[1:] > cluster[:-1]) and np.all(env[1:] > env[:-1])
        env_amplitudes.append(env_psi)
    return Case(name, op, keys, _concat(amplitudes, np.float64), offsets, _concat(envs, np.uint64),
                _concat(env_amplitudes, np.float64), _offsets(envs), other, coeffs, counts)


def _kagome16():
    return model_operator("heisenberg_kagome_16")


SIZES = (1, 2, 3, 5, 63, 64, 65, 301, 1)  # T = 505: segment boundaries inside a workgroup, T no multiple of 4


def _sizes():
    op = _kagome16()
    return from_segments("kagome16 sizes", op, [grow(op, n, 200 + i) for i, n in enumerate(SIZES)],
                         [NATURAL] * len(SIZES), 201)


MANY = 4097


def _many_segments():
    """4097 segments of 1, 2, 3, 1, ... consecutive basis states (the bisection)."""
    op = _kagome16()
    op.basis.build()
    states = op.basis.states
    sizes = 1 + np.arange(MANY) % 3
    ends = np.cumsum(sizes)
    assert ends[-1] <= states.size
    return from_segments("4097 segments of 1-3 keys", op, [states[e - n:e] for e, n in zip(ends, sizes)],
                         [NATURAL] * MANY, 203)


FOLD = 300


def shared_states():
    """`(x, y)`: x sits in 300 clusters, its neighbour y in their 300 environments."""
    op = _kagome16()
    x = grow(op, 1, 205)
    other, coeffs, _ = op.batched_apply(x)
    leaving = other[:, 0][(other[:, 0] != x[0]) & (coeffs.real != 0)]
    return int(x[0]), int(leaving[0])


def _one_state_everywhere():
    op = _kagome16()
    op.basis.build()
    x, y = shared_states()
    rest = op.basis.states[(op.basis.states != x) & (op.basis.states != y)]
    rest = np.random.default_rng(207).permutation(rest)[:FOLD]
    return from_segments("one state in 300 segments", op, [np.unique([x, int(z)]) for z in rest], [NATURAL] * FOLD, 209)


def _neighbours():
    """Segment A: a cluster; segment B: a cluster made of states of A's environment."""
    op = _kagome16()
    a = grow(op, 60, 211)
    env = field_cases.make_case("A", op, a, 0).env_keys
    return from_segments("neighbouring clusters", op, [a, env[::2]], [NATURAL, NATURAL], 213)


DRAWS = 5


def _draws():
    """The reweight shape: the same keys and environment keys in 5 segments, 5 different psi / env_psi."""
    op = _kagome16()
    cluster = grow(op, 60, 215)
    env = field_cases.make_case("cluster", op, cluster, 0).env_keys
    return from_segments("one cluster, 5 draws", op, [cluster] * DRAWS, [env] * DRAWS, 217)


def _missing_key():
    """Five clusters; segment 2's environment lacks its first key."""
    op = _kagome16()
    clusters = [grow(op, 30 + 7 * g, 220 + g) for g in range(5)]
    envs = [field_cases.make_case("c", op, c, 0).env_keys for c in clusters]
    envs[2] = envs[2][1:]
    return from_segments("a missing environment key", op, clusters, envs, 227)


def _empty_segments():
    """An empty cluster with an environment, a cluster without environment, a full segment, nothing at all."""
    op = _kagome16()
    a, b = grow(op, 9, 229), grow(op, 6, 231)
    env = field_cases.make_case("a", op, a, 0).env_keys
    return from_segments("empty segments", op, [_empty(), b, a, _empty(), a[:1]], [env, _empty(), NATURAL, _empty(),
                                                                                    NATURAL], 233)


def _all_empty():
    op = _kagome16()
    env = field_cases.make_case("a", op, grow(op, 4, 235), 0).env_keys
    return from_segments("all segments empty", op, [_empty()] * 3, [env, _empty(), env[:2]], 237)


def _single(name):
    """S = 1: a case of field_cases.py with its own environment and amplitudes."""
    c = field_cases.case(name)
    return from_segments("S=1: " + name, c.operator, [c.keys], [c.env_keys], 0, [c.psi], [c.env_psi])


ENV_SIZES = (0, 1, 63, 64, 65, 4097)


def _environment_sizes():
    c = field_cases.case("kagome16 K=300")
    envs = [environment_of_size(c, size, seed=size) if size else (_empty(), np.zeros(0)) for size in ENV_SIZES]
    return from_segments("environment sizes", c.operator, [c.keys] * len(envs), [e[0] for e in envs], 239,
                         [c.psi] * len(envs), [e[1] for e in envs])


def _split(name):
    """Three overlapping parts of a field_cases.py cluster: a head, the whole, a middle."""
    c = field_cases.case(name)
    k = c.keys
    return from_segments("parts of " + name, c.operator, [k[:k.size // 3], k, k[k.size // 5:3 * k.size // 4]],
                         [NATURAL] * 3, 241 + field_cases.NAMES.index(name))


def _awkward():
    """-0.0, 0.0, subnormals and negatives in env_psi (and in psi, of which only |psi| counts)."""
    op = _kagome16()
    clusters = [grow(op, n, 250 + n) for n in (1, 7, 2, 33)]
    natural = from_segments("tmp", op, clusters, [NATURAL] * 4, 0)
    envs = [natural.segment(g)[2] for g in range(4)]
    env_psis = [awkward_amplitudes(e.size) for e in envs]
    env_psis[2] = np.roll(env_psis[2], 3)
    psis = [None, awkward_amplitudes(7)[::-1].copy(), None, None]
    return from_segments("signed zeros and subnormals", op, clusters, envs, 251, psis, env_psis)


SPLIT_PLAIN = ("j1j2 64 bonds", "sk16 first 65 bonds", "sk16 120 bonds", "ring64 bit 63")
SPLIT_LISTED = ("kagome18 inversion +1", "kagome18 inversion -1", "ring22 inversion -1", "single-site flips")
BUILDERS = {
    "kagome16 sizes": _sizes,
    "4097 segments of 1-3 keys": _many_segments,
    "one state in 300 segments": _one_state_everywhere,
    "neighbouring clusters": _neighbours,
    "one cluster, 5 draws": _draws,
    "a missing environment key": _missing_key,
    "empty segments": _empty_segments,
    "all segments empty": _all_empty,
    "S=1: kagome16 K=7": functools.partial(_single, "kagome16 K=7"),
    "environment sizes": _environment_sizes,
    "signed zeros and subnormals": _awkward,
}
BUILDERS.update({"parts of " + name: functools.partial(_split, name) for name in SPLIT_PLAIN + SPLIT_LISTED})
BUILDERS["S=1: ring22 inversion -1"] = functools.partial(_single, "ring22 inversion -1")
LISTED = tuple("parts of " + name for name in SPLIT_LISTED) + ("S=1: ring22 inversion -1",)
PLAIN = tuple(name for name in BUILDERS if name not in LISTED)
NAMES = PLAIN + LISTED
# the cases about contributions: between 10 % and 90 % of their off-diagonal connections add a term
CONTRIBUTIONS = ("kagome16 sizes", "neighbouring clusters", "one cluster, 5 draws", "a missing environment key",
                 "environment sizes")


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.name = name
    return c


@functools.lru_cache(maxsize=None)
def _shared_law(name, scale):
    c = case(name)
    field, unresolved = field_segments_law(c.other, c.coeffs, c.counts, c.keys, c.psi, c.offsets, c.env_keys,
                                           c.env_psi, c.env_offsets, scale)
    field.setflags(write=False)
    unresolved.setflags(write=False)
    return field, unresolved


def contributing_share(c):
    """The share of the off-diagonal connections (non-zero coefficient, target other than the row's own state) that
    add a term under the per-cluster law: they leave the cluster of their segment and end in its environment."""
    adds = total = 0
    for g in range(c.segments):
        keys, _, env_keys, _ = c.segment(g)
        sources, targets, coeffs = c.connections(g)
        off_diagonal = (targets != sources) & (coeffs != 0)
        total += int(np.count_nonzero(off_diagonal))
        adds += int(np.count_nonzero(off_diagonal & ~positions(keys, targets)[1] & positions(env_keys, targets)[1]))
    return adds / total
