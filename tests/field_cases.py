"""The cases of tests/test_field_cases.py and tests/test_gpu_field.py: the boundary field of a cluster,
specification ASP-FIELD-1 (csrc/operator_field.hip), and its sequential numpy restatement
`field_law`.

A helper module like tests/helpers.py and tests/symmetry_cases.py: no fixtures, no files, nothing compiled, no
GPU.  The connections of a case come from the host `Operator.batched_apply` (the device action equals it bit for
bit: tests/test_gpu_operator.py, tests/test_gpu_symmetry_edges.py), are computed once per case and shared.
"""
import functools
from dataclasses import dataclass

import numpy as np


# -- the law -------------------------------------------------------------------------------------------------
def positions(haystack, needles):
    """(index of every needle in the sorted haystack, found?)."""
    haystack = np.asarray(haystack, dtype=np.uint64)
    needles = np.asarray(needles, dtype=np.uint64)
    if haystack.size == 0:
        return np.zeros(needles.shape[0], dtype=np.int64), np.zeros(needles.shape[0], dtype=bool)
    at = np.minimum(np.searchsorted(haystack, needles), haystack.size - 1)
    return at.astype(np.int64), haystack[at] == needles


def field_law(other, coeffs, counts, keys, psi, env_keys, env_psi, scale):
    """ASP-FIELD-1 with Python floats (IEEE doubles, every operation rounded on its own, no contraction):
    `(field f64[K], unresolved)`.  Per row, over its connections in order, from +0.0: a target among `keys`
    adds nothing; a target `env_keys[p]` adds `(coeff * |psi_r|) * env_psi[p]`; any other target adds nothing
    and is counted when its coefficient is non-zero; `field[r] = scale * sum`."""
    _, inside = positions(keys, other)
    where, known = positions(env_keys, other)
    env_psi = np.asarray(env_psi, dtype=np.float64)
    field = np.zeros(len(keys), dtype=np.float64)
    unresolved = 0
    e = 0
    for r, count in enumerate(np.asarray(counts).tolist()):
        acc = 0.0
        a = abs(float(psi[r]))
        for _ in range(count):
            if not inside[e]:
                if known[e]:
                    acc = acc + ((float(coeffs[e]) * a) * float(env_psi[where[e]]))
                elif coeffs[e] != 0:
                    unresolved += 1
            e += 1
        field[r] = float(scale) * acc
    return field, unresolved


def other_psi(other, env_keys, env_psi):
    """`other_psi` of the reference's build_matrix for an environment: its amplitude where the target is an
    environment state, 0 elsewhere (a hit ignores it)."""
    where, known = positions(env_keys, other)
    if not known.any():
        return np.zeros(len(other), dtype=np.float64)
    return np.where(known, np.asarray(env_psi, dtype=np.float64)[where], 0.0)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# -- operators -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    from annealing_sign_problem_amd import synthetic

    return synthetic.load_models()


def model_operator(name, inversion=None):
    """A bundled model; `inversion`: the same model in the sector with that spin-inversion character."""
    import copy

    from annealing_sign_problem_amd import operators

    config = copy.deepcopy(_models()[name])
    if inversion is not None:
        config["basis"]["spin_inversion"] = inversion
    return operators.Operator.from_config(config)


def first_bonds(name, count):
    """The first `count` bonds of a bundled model (distinct site pairs: rows reach distinct states)."""
    from annealing_sign_problem_amd import operators

    op = model_operator(name)
    flat = [(t.matrix, s) for t in op.terms for s in t.sites][:count]
    assert len(flat) == count
    basis = operators.SpinBasis(op.basis.number_spins, op.basis.hamming_weight)
    return operators.Operator(basis, [operators.Term(m, [s]) for m, s in flat])


def plain_ring(n, weight):
    """Heisenberg ring without symmetries."""
    from annealing_sign_problem_amd import operators

    bonds = [(i, (i + 1) % n) for i in range(n)] if n > 2 else [(0, 1)]
    return operators.Operator(operators.SpinBasis(n, weight), [operators.Term(operators.SIGMA_DOT_SIGMA, bonds)])


def num_bonds(op):
    return sum(len(t.sites) for t in op.terms)


# -- clusters and environments ---------------------------------------------------------------------------------
def _keep(op, states):
    """The states that are basis states (a symmetric basis: representatives of non-zero norm)."""
    group = op.basis.group
    if group is None:
        return states
    rep, _, norm = group.state_info(states)
    return np.unique(rep[norm > 0])


def grow(op, count, seed, start=None):
    """`count` sorted unique basis states grown from one state through the operator's connections."""
    rng = np.random.default_rng(seed)
    n, w = op.basis.number_spins, op.basis.hamming_weight
    if start is None:
        bits = rng.choice(n, size=n // 2 if w is None else w, replace=False)
        start = sum(1 << int(b) for b in bits)
    keys = {int(x) for x in _keep(op, np.array([start], dtype=np.uint64))[:1]}
    assert keys, "the start state has norm 0"
    frontier = sorted(keys)
    while len(keys) < count:
        other, _, _ = op.batched_apply(np.array(frontier, dtype=np.uint64))
        cand = rng.permutation(_keep(op, np.unique(other[:, 0])))
        fresh = [int(x) for x in cand if int(x) not in keys][: max(2, count // 6)][: count - len(keys)]
        if not fresh:
            assert len(frontier) < len(keys), "the sector holds fewer than {} connected states".format(count)
            frontier = sorted(keys)
            continue
        keys.update(fresh)
        frontier = fresh
    return np.array(sorted(keys), dtype=np.uint64)


@dataclass
class Case:
    name: str
    operator: object
    keys: np.ndarray       # u64[K] ascending, unique
    psi: np.ndarray        # f64[K] signed, unit norm
    other: np.ndarray      # host batched_apply(keys): targets u64[N]
    coeffs: np.ndarray     # f64[N]
    counts: np.ndarray     # i64[K]
    env_keys: np.ndarray   # the one-hop extension without the cluster
    env_psi: np.ndarray    # signed amplitudes of the environment

    def law(self, env_keys=None, env_psi=None, scale=1.0, psi=None):
        env_keys = self.env_keys if env_keys is None else env_keys
        env_psi = self.env_psi if env_psi is None else env_psi
        return field_law(self.other, self.coeffs, self.counts, self.keys, self.psi if psi is None else psi,
                         env_keys, env_psi, scale)

    @property
    def leaving(self):
        """Per connection: it leaves the cluster with a non-zero coefficient."""
        return ~positions(self.keys, self.other)[1] & (self.coeffs != 0)


def make_case(name, op, keys, seed):
    rng = np.random.default_rng(seed)
    other, coeffs, counts = op.batched_apply(keys)
    assert not np.any(coeffs.imag)
    other, coeffs = np.ascontiguousarray(other[:, 0]), np.ascontiguousarray(coeffs.real)
    psi = rng.normal(size=keys.size) * np.exp(rng.normal(size=keys.size))
    psi /= np.linalg.norm(psi)
    outside = ~positions(keys, other)[1] & (coeffs != 0)
    env_keys = np.unique(other[outside])
    env_psi = rng.normal(size=env_keys.size) * np.exp(rng.normal(size=env_keys.size)) * 0.1
    return Case(name, op, keys, psi, other, coeffs, counts, env_keys, env_psi)


def _kagome16(count, seed):
    op = model_operator("heisenberg_kagome_16")
    return op, grow(op, count, seed)


def _symmetry_case(name):
    import symmetry_cases

    expected = symmetry_cases.expected(symmetry_cases.BY_NAME[name])
    return expected.operator, expected.keys


def _ring64_high():
    """64 sites, and keys with bit 63 set."""
    op = plain_ring(64, 32)
    start = sum(1 << i for i in range(1, 64, 2))  # 1010...10: site 63 up
    keys = grow(op, 50, 7, start)
    assert np.count_nonzero(keys >> np.uint64(63)) >= 10 and np.count_nonzero(keys >> np.uint64(63) == 0) >= 1
    return op, keys


def _single_site_flips():
    """No symmetry, single-site flips: bonds that share a site reach the same state twice (list form)."""
    from helpers import random_operator

    op, keys, _ = random_operator(5, "double_reach", number_spins=14, num_bonds=20, num_keys=90)
    return op, keys


BUILDERS = {
    "kagome16 K=1": lambda: _kagome16(1, 11),
    "kagome16 K=7": lambda: _kagome16(7, 12),
    "kagome16 K=300": lambda: _kagome16(300, 13),
    "kagome16 K=301": lambda: _kagome16(301, 14),          # 301 = 75 workgroups of 4 rows + 1
    "ring4 full basis": lambda: (plain_ring(4, 2), np.array([3, 5, 6, 9, 10, 12], dtype=np.uint64)),
    "j1j2 64 bonds": lambda: (model_operator("j1j2_square_4x4"), grow(model_operator("j1j2_square_4x4"), 40, 15)),
    "sk16 first 65 bonds": lambda: (first_bonds("sk_16_1", 65), grow(first_bonds("sk_16_1", 65), 40, 16)),
    "sk16 120 bonds": lambda: (model_operator("sk_16_1"), grow(model_operator("sk_16_1"), 40, 17)),
    "ring64 bit 63": _ring64_high,
    "kagome18 inversion +1": lambda: (model_operator("heisenberg_kagome_18", 1),
                                      grow(model_operator("heisenberg_kagome_18", 1), 40, 18)),
    "kagome18 inversion -1": lambda: (model_operator("heisenberg_kagome_18", -1),
                                      grow(model_operator("heisenberg_kagome_18", -1), 40, 19)),
    "ring20 all-to-all, inversion -1": lambda: _symmetry_case("ring20 all-to-all, inversion -1"),
    "ring22 inversion -1": lambda: _symmetry_case("ring22 inversion -1"),
    "single-site flips": _single_site_flips,
}
PLAIN = ("kagome16 K=1", "kagome16 K=7", "kagome16 K=300", "kagome16 K=301", "ring4 full basis", "j1j2 64 bonds",
         "sk16 first 65 bonds", "sk16 120 bonds", "ring64 bit 63")
LISTED = ("kagome18 inversion +1", "kagome18 inversion -1", "ring20 all-to-all, inversion -1", "ring22 inversion -1",
          "single-site flips")
NAMES = PLAIN + LISTED
# the cases the reference binary's field is pinned on (the issue's list: kagome_16, sk_16_1, j1j2_4x4,
# kagome_18 with inversion +-1; K = 1 ... 300)
REFERENCE = ("kagome16 K=1", "kagome16 K=7", "kagome16 K=300", "j1j2 64 bonds", "sk16 120 bonds",
             "kagome18 inversion +1", "kagome18 inversion -1")


@functools.lru_cache(maxsize=None)
def case(name):
    op, keys = BUILDERS[name]()
    return make_case(name, op, keys, seed=100 + NAMES.index(name))


# -- environments --------------------------------------------------------------------------------------------
def environment_of_size(c, size, seed=0):
    """`size` sorted environment keys for a kagome16 case: the needed ones first (in a random order), then
    other states of the basis; fewer than needed leaves connections unresolved.  With amplitudes."""
    rng = np.random.default_rng(seed)
    basis = c.operator.basis
    if basis._states is None:
        basis.build()
    rest = np.setdiff1d(np.setdiff1d(basis.states, c.env_keys), c.keys)
    pool = np.concatenate([rng.permutation(c.env_keys), rng.permutation(rest)])
    assert pool.size >= size
    env_keys = np.sort(pool[:size])
    return env_keys, rng.normal(size=size)


def awkward_amplitudes(count):
    """-0.0, 0.0, subnormals of both signs, negatives and positives in turn."""
    values = np.array([-0.0, 0.0, 5e-324, -1e-310, -0.75, 0.5, 2.5e-308, -3.0])
    return values[np.arange(count) % values.size].copy()


# -- the energy identity -------------------------------------------------------------------------------------
def couplings(op, keys, psi):
    """J of make_ising_model from numpy and scipy (tests/helpers.py: reference_route_ising), CSR."""
    from helpers import reference_route_ising

    return reference_route_ising(op, keys, psi).tocsr()


def identity_defect(op, vector, keys, exchange, field, trials=6, seed=0):
    """The largest `|(c^2 (s'Js + h's) - phi(s)'H phi(s)) - (the same at s0)|` over random sign vectors s, and
    the scale `c^2 (sum|J| + sum|h|)`.  `vector`: signed amplitudes over the built basis; phi(s): `vector` with
    its entries on `keys` replaced by `s |vector|`; c: the norm of `vector` over `keys`."""
    h = op.to_sparse().real.tocsr()
    where = np.searchsorted(op.basis.states, keys)
    assert np.array_equal(op.basis.states[where], keys)
    c2 = float(np.dot(vector[where], vector[where]))
    rng = np.random.default_rng(seed)

    def gap(s):
        phi = vector.copy()
        phi[where] = s * np.abs(vector[where])
        return c2 * (s @ (exchange @ s) + field @ s) - phi @ (h @ phi)

    base = gap(np.sign(vector[where]) + (vector[where] == 0))
    worst = max(abs(gap(rng.choice([-1.0, 1.0], size=keys.size)) - base) for _ in range(trials))
    return worst, c2 * (abs(exchange).sum() + np.abs(field).sum())
