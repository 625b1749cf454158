"""The coupling stencil on the GPU (csrc/ising_stencil.hip, ASP-STENCIL-1): couplings
from stored matrix elements and new amplitudes alone equal asp_operator_ising_csr's bit for bit on both of
its paths; a pattern change in either direction is reported and touches nothing; a batch of plans takes
the values exactly as asp_sa_plan_reweight would; the noise study's rows do not depend on the route.
Everything is exact: values are compared as uint64 views."""
import ctypes
import functools

import numpy as np
import pytest

import stencil_cases as law

pytestmark = pytest.mark.gpu

INVALID = -3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _build_count():
    from annealing_sign_problem_amd import _lib

    return _lib.load().asp_sa_layout_build_count()


# ---- operators ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_ring(n):
    """tests/test_gpu_noise.py's ring: no symmetries, half filling."""
    from annealing_sign_problem_amd import operators

    matrix = [[1, 0, 0, 0], [0, -1, 2, 0], [0, 2, -1, 0], [0, 0, 0, 1]]
    config = {"basis": {"number_spins": n, "hamming_weight": n // 2, "symmetries": []},
              "hamiltonian": {"terms": [{"matrix": matrix, "sites": [[i, (i + 1) % n] for i in range(n)]}]}}
    operator = operators.Operator.from_config(config)
    operator.basis.build()
    return operator


@functools.lru_cache(maxsize=None)
def _symmetric_ring(n):
    """tests/test_gpu_sector.py's ring: translations, reflection and spin inversion +1 — rows reach a
    representative more than once, their own among them."""
    from annealing_sign_problem_amd import operators, symmetry

    generators = [[(i + 1) % n for i in range(n)], [(n - i) % n for i in range(n)]]
    basis = operators.SpinBasis(n, n // 2, symmetry.SymmetryGroup(n, generators, 1))
    operator = operators.Operator(basis, [operators.Term(operators.SIGMA_DOT_SIGMA, [(i, (i + 1) % n) for i in range(n)])])
    operator.basis.build()
    return operator


@functools.lru_cache(maxsize=None)
def _j1j2():
    from annealing_sign_problem_amd import operators, synthetic

    operator = operators.Operator.from_config(synthetic.load_models()["j1j2_square_4x4"])
    operator.basis.build()
    return operator


@functools.lru_cache(maxsize=None)
def _random(kind):
    """tests/helpers.py: "one_way" (distinct targets, elements in one direction only), "double_reach"
    (single-site flips, every element mirrored: duplicates) and "single_flip" (duplicates AND
    one-directional elements: the fused build refuses, and so does the stencil)."""
    from helpers import random_operator

    seed = {"one_way": 3, "double_reach": 5, "single_flip": 4}[kind]
    operator, keys, _ = random_operator(seed, kind, number_spins=14, num_bonds=20, num_keys=200)
    return operator, keys


def _grown(operator, size, seed):
    from annealing_sign_problem_amd import synthetic

    states = operator.basis.states
    keys = synthetic.grow_cluster(operator, int(states[len(states) // 3]), size, seed=seed)
    assert keys.shape[0] == size
    return keys


def _with_isolated_row(operator):
    """A grown cluster and one more state that no member reaches and that reaches none: its row has no
    in-cluster connection but its diagonal."""
    keys = _grown(operator, 40, 9)
    other, _, _ = operator.batched_apply(keys)
    reached = np.unique(other[:, 0])
    lonely = np.setdiff1d(operator.basis.states, reached)
    assert lonely.shape[0] > 0
    return np.union1d(keys, lonely[:1])


def _case(name):
    if name.startswith("ring10 K="):
        operator = _plain_ring(10)
        return operator, _grown(operator, int(name.split("=")[1]), 11)
    if name == "single-site flips, mirrored":
        return _random("double_reach")
    if name == "one-directional elements":
        return _random("one_way")
    operator, keys = {
        "ring10 whole basis": lambda: (_plain_ring(10), None),
        "ring10 isolated row": lambda: (_plain_ring(10), _with_isolated_row(_plain_ring(10))),
        "ring12 whole basis, zero diagonals": lambda: (_plain_ring(12), None),
        "symmetric ring12 whole basis": lambda: (_symmetric_ring(12), None),
        "symmetric ring12 first 20": lambda: (_symmetric_ring(12), _symmetric_ring(12).basis.states[:20]),
        "j1j2 whole basis": lambda: (_j1j2(), None),
        "j1j2 K=130": lambda: (_j1j2(), _grown(_j1j2(), 130, 13)),
    }[name]()
    return operator, operator.basis.states if keys is None else keys


CASES = ["ring10 whole basis", "ring10 K=1", "ring10 K=2", "ring10 K=63", "ring10 K=64", "ring10 K=65", "ring10 K=130",
         "ring10 isolated row", "ring12 whole basis, zero diagonals", "symmetric ring12 whole basis",
         "symmetric ring12 first 20", "j1j2 whole basis", "j1j2 K=130", "single-site flips, mirrored",
         "one-directional elements"]


def _amplitudes(rng, shape):
    """exp(N(0, 1.5^2)) with random signs."""
    return np.exp(rng.normal(scale=1.5, size=shape)) * rng.choice([-1.0, 1.0], size=shape)


def _connections(operator, keys):
    other, coeffs, counts = operator.device().apply(keys)
    offsets = np.zeros(keys.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, law.resolve(keys, other), coeffs


def _check(device, stencil, keys, pattern, psi):
    """values(psi) against ising_csr(keys, psi): status 0 and the same bits where the pattern is the
    stencil's, status 1 where it is not.  Returns whether it was."""
    indptr, col, val = device.ising_csr(keys, psi)
    data, status = stencil.values(psi)
    same = np.array_equal(indptr, pattern[0]) and np.array_equal(col, pattern[1])
    assert status.tolist() == [0 if same else 1]
    if same:
        assert np.array_equal(_bits(data[0]), _bits(val))
    return same


@pytest.mark.parametrize("name", CASES)
def test_values_equal_ising_csr(name):
    operator, keys = _case(name)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    K = keys.shape[0]
    device = operator.device()
    rng = np.random.default_rng(len(name) + K)
    psi0 = _amplitudes(rng, K)
    indptr, col, val0 = device.ising_csr(keys, psi0)
    pattern = (indptr.copy(), col.copy())
    with device.ising_stencil(keys, *pattern) as stencil:
        info = stencil.info
        assert (info.num_spins, info.stored) == (K, col.shape[0])
        assert info.groups <= info.connections and info.longest_group >= 1
        if "symmetric" in name or "single-site" in name:
            assert not device.unique_targets  # the duplicate-keeping build
        if name == "symmetric ring12 whole basis":
            assert info.groups < info.connections and info.longest_group > 1  # and duplicates are there
        if name == "ring12 whole basis, zero diagonals":
            assert info.silent_pairs > 0 and np.count_nonzero(np.diff(indptr) == 0) == 0
        if name == "ring10 isolated row":
            assert 1 in np.diff(indptr).tolist()
        if K <= 252:  # the restatement, from the connection list of asp_operator_apply
            offsets, targets, coeffs = _connections(operator, keys)
            assert info.connections == np.count_nonzero(targets >= 0)
            assert info.silent_pairs == len(law.silent_pairs(offsets, targets, *pattern))
            want, changed = law.values(offsets, targets, coeffs, psi0, *pattern)
            assert not changed and np.array_equal(_bits(want), _bits(val0))
        # single draws: as drawn, and scaled up and down by 2^400
        assert _check(device, stencil, keys, pattern, psi0)
        psi = _amplitudes(rng, K)
        for scale in (1.0, 2.0 ** 400, 2.0 ** -400):
            assert _check(device, stencil, keys, pattern, psi * scale), scale
        if K <= 252:
            want, changed = law.values(offsets, targets, coeffs, psi, *pattern)
            assert not changed and np.array_equal(_bits(want), _bits(stencil.values(psi)[0][0]))
        # a batch of 16 equals the 16 single calls
        psis = _amplitudes(rng, (16, K))
        data, status = stencil.values(psis)
        assert status.tolist() == [0] * 16
        for d in (0, 7, 15) if K > 1000 else range(16):
            single, one = stencil.values(psis[d])
            assert one.tolist() == [0] and np.array_equal(_bits(single[0]), _bits(data[d]))
            assert np.array_equal(_bits(device.ising_csr(keys, psis[d])[2]), _bits(data[d]))


@pytest.mark.parametrize("name", ["ring10 whole basis", "symmetric ring12 whole basis", "j1j2 K=130"])
def test_subnormal_amplitudes(name):
    """Some amplitudes subnormal: products underflow, partly to subnormals and partly to 0.  The stencil is
    made from the pattern such a draw has; other draws of that kind keep it or are reported."""
    operator, keys = _case(name)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    K = keys.shape[0]
    device = operator.device()
    rng = np.random.default_rng(K)
    tiny = rng.random(K) < 0.3
    psi0 = _amplitudes(rng, K) * np.where(tiny, 2.0 ** -1030, 1.0)
    assert np.any((np.abs(psi0) < 2.3e-308) & (psi0 != 0))
    indptr, col, val = device.ising_csr(keys, psi0)
    assert np.any((np.abs(val) < 2.3e-308) & (val != 0))
    pattern = (indptr.copy(), col.copy())
    with device.ising_stencil(keys, *pattern) as stencil:
        assert stencil.info.silent_pairs > 0  # pairs of two subnormal amplitudes vanished
        assert _check(device, stencil, keys, pattern, psi0)
        kept = 0
        for _ in range(4):
            psi = _amplitudes(rng, K) * np.where(tiny, 2.0 ** -1030, 1.0)
            kept += _check(device, stencil, keys, pattern, psi)
        assert kept > 0
        # all amplitudes subnormal: every product is 0, every stored pair is gone
        assert not _check(device, stencil, keys, pattern, psi0 * np.where(tiny, 1.0, 2.0 ** -1030))


# ---- plans -------------------------------------------------------------------------------------------------
def observe(ham, full=True):
    """What the issue lists, as a dict of exactly comparable arrays; ``full=False``: info and energies."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    info = ham.info()
    K = ham.size
    out = {"info": np.array([repr(getattr(info, name)) for name, _ in _lib.SaInfo._fields_])}
    rng = np.random.default_rng(7)
    xs = np.stack([sa.signs_to_bits(rng.choice([-1.0, 1.0], size=K)) for _ in range(8)])
    out["energies"] = _bits(ham.energies(xs))
    if not full:
        return out
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, 64)
    for name, shuffled in (("colour", False), ("shuffled", True)):
        x, e = sa.anneal_raw(ham, 3, betas, 4, shuffled=shuffled)
        out[name + "_x"], out[name + "_e"] = x.copy(), _bits(e)
    for tree in ("host", "device"):
        x, e = sa.greedy_solve(ham, tree=tree)
        out["greedy_" + tree + "_x"], out["greedy_" + tree + "_e"] = np.array(x), _bits([e])
    x, e = sa.parallel_tempering_cluster(ham, seed=5, number_rounds=1, sweeps_per_round=2, repetitions=4,
                                         only_best=False)
    out["pt_x"], out["pt_e"] = np.array(x), _bits(e)
    return out


def assert_same(got, expected):
    assert sorted(got) == sorted(expected)
    for name in expected:
        assert np.array_equal(got[name], expected[name]), name


def _raw_batch(stencil, hams, psis, fields=None, want_data=True):
    """asp_sa_plan_reweight_stencil_batch itself: (rc, message, statuses, data)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    count = len(hams)
    psis = np.ascontiguousarray(psis, dtype=np.float64)
    data = np.full((count, stencil.nnz), np.nan)
    items = (_lib.SaStencilItem * max(count, 1))()
    for d, ham in enumerate(hams):
        items[d].plan = ham.plan()
        items[d].psi = psis[d].ctypes.data
        items[d].field = None if fields is None else fields[d].ctypes.data
        items[d].data_out = data[d].ctypes.data if want_data else None
        items[d].status = -1
    rc = lib.asp_sa_plan_reweight_stencil_batch(stencil.handle(), items, ctypes.c_uint32(count))
    return rc, _lib.last_error(), [items[d].status for d in range(count)], data


class _Family:
    """A base Hamiltonian on the whole basis of `operator` (couplings of psi0, a non-zero field) and its
    stencil."""

    def __init__(self, operator, seed):
        from annealing_sign_problem_amd import annealer as sa

        self.operator, self.keys = operator, operator.basis.states
        self.device = operator.device()
        self.rng = np.random.default_rng(seed)
        self.K = self.keys.shape[0]
        psi0 = _amplitudes(self.rng, self.K)
        psi0 /= np.linalg.norm(psi0)
        self.indptr, self.col, val = self.device.ising_csr(self.keys, psi0)
        self.field0 = self.rng.normal(size=self.K) * np.abs(val).mean()
        self.base = sa.Hamiltonian.from_canonical_csr(self.indptr, self.col, val.copy(), self.field0)
        self.base.plan()
        self.stencil = self.device.ising_stencil(self.keys, self.indptr, self.col)

    def draws(self, count):
        psis = _amplitudes(self.rng, (count, self.K))
        return psis / np.linalg.norm(psis, axis=1, keepdims=True)

    def fresh(self, psi, field):
        from annealing_sign_problem_amd import annealer as sa

        indptr, col, val = self.device.ising_csr(self.keys, psi)
        assert np.array_equal(indptr, self.indptr) and np.array_equal(col, self.col)
        return sa.Hamiltonian.from_canonical_csr(indptr.copy(), col.copy(), val.copy(), field), val

    def close(self):
        self.stencil.close()
        self.base.release()


@pytest.mark.parametrize("count, with_field, with_data, warm", [(1, True, True, False), (3, False, False, True),
                                                                (16, True, False, False), (3, True, True, True)])
@pytest.mark.parametrize("which", ["ring10", "symmetric ring12"])
def test_batch_equals_fresh_plans(which, count, with_field, with_data, warm):
    """`warm`: the shuffled, cluster and device-tree paths were used BEFORE the call, so their lazily
    uploaded arrays exist and are scattered into; otherwise they are first used after it and come from the
    updated host layout."""
    family = _Family(_plain_ring(10) if which == "ring10" else _symmetric_ring(12), seed=count + 10 * warm)
    try:
        clones = [family.base.clone() for _ in range(count)]
        if warm:
            expected = observe(family.base)
            for clone in clones:
                assert_same(observe(clone), expected)
        psis = family.draws(count)
        fields = family.rng.normal(size=(count, family.K)) * 0.01 if with_field else None
        builds = _build_count()
        rc, message, statuses, data = _raw_batch(family.stencil, clones, psis, fields, with_data)
        assert rc == 0, message
        assert statuses == [0] * count and _build_count() == builds
        from annealing_sign_problem_amd import annealer as sa

        assert sa.reweight_hamiltonians_last_ms() > 0.0
        for d, clone in enumerate(clones):
            fresh, val = family.fresh(psis[d], fields[d] if with_field else family.field0)
            if with_data:
                assert np.array_equal(_bits(data[d]), _bits(val))
            else:
                assert np.isnan(data[d]).all()
            assert_same(observe(clone), observe(fresh))
            fresh.release()
        for clone in clones:
            clone.release()
    finally:
        family.close()


def test_stored_entries_of_value_zero_that_the_plan_does_not_hold():
    """One-directional elements onto a state whose amplitude is the smallest subnormal: the pair's sum is
    one or two units in the last place, so the entry exists, and its half rounds to 0.0 — a stored pair
    with J_ij + J_ji = 0, which the plan's A drops.  Such pairs must keep cancelling; they do here, and
    the batch equals the fresh plans."""
    from annealing_sign_problem_amd import annealer as sa

    operator, keys = _random("one_way")
    device = operator.device()
    K = keys.shape[0]
    rng = np.random.default_rng(4)

    def draw():
        psi = rng.uniform(0.75, 1.25, size=K) * rng.choice([-1.0, 1.0], size=K)
        psi[tiny] = 5e-324
        return psi

    for tiny in range(K):  # the first state that a one-directional element of size about 1 lands on
        indptr, col, val = device.ising_csr(keys, draw())
        if np.any(val == 0.0):
            break
    assert np.any(val == 0.0)
    base = sa.Hamiltonian.from_canonical_csr(indptr.copy(), col.copy(), val.copy(), np.zeros(K))
    assert base.info().nnz_offdiag < np.count_nonzero(np.repeat(np.arange(K), np.diff(indptr)) != col)
    with device.ising_stencil(keys, indptr, col) as stencil:
        clones = [base.clone() for _ in range(3)]
        psis = np.stack([draw() for _ in range(3)])
        rc, message, statuses, data = _raw_batch(stencil, clones, psis)
        assert rc == 0, message
        for d, clone in enumerate(clones):
            indptr_d, col_d, val_d = device.ising_csr(keys, psis[d])
            same = np.array_equal(indptr_d, indptr) and np.array_equal(col_d, col)
            assert statuses[d] == (0 if same else 1)
            if same:
                assert np.array_equal(_bits(data[d]), _bits(val_d))
                assert_same(observe(clone), observe(sa.Hamiltonian.from_canonical_csr(indptr_d, col_d, val_d, np.zeros(K))))
            else:
                assert_same(observe(clone, False), observe(base, False))
            clone.release()
        assert 0 in statuses
    base.release()


def test_reweight_hamiltonians_updates_the_python_objects():
    from annealing_sign_problem_amd import annealer as sa

    family = _Family(_plain_ring(10), seed=5)
    try:
        clones = [family.base.clone() for _ in range(3)]
        assert all(c.family() is family.base.family() for c in clones)
        psis = family.draws(3)
        fields = family.rng.normal(size=(3, family.K)) * 0.01
        assert sa.reweight_hamiltonians(clones[:2], family.stencil, psis[:2], fields[:2]) == [True, True]
        assert sa.reweight_hamiltonians(clones[2:], family.stencil, psis[2:]) == [True]
        for d, clone in enumerate(clones):
            field = fields[d] if d < 2 else family.field0
            fresh, val = family.fresh(psis[d], field)
            assert np.array_equal(_bits(clone.exchange.data), _bits(val)) and np.array_equal(clone.field, field)
            assert not clone.exchange.data.flags.writeable and not clone.field.flags.writeable
            assert np.shares_memory(clone.exchange.indices, family.base.exchange.indices)
            assert_same(observe(clone), observe(fresh))
            x, e = sa.greedy_solve(clone)  # (and the plan is still the object's: no rebuild behind the scenes)
            assert clone._plan_key == clone._key()
        assert sa.reweight_hamiltonians([], family.stencil, np.zeros((0, family.K))) == []
    finally:
        family.close()


def test_refusals_touch_nothing_and_name_the_item():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    family = _Family(_plain_ring(10), seed=6)
    other = _Family(_plain_ring(12), seed=6)
    try:
        clones = [family.base.clone() for _ in range(3)]
        before = [observe(c, False) for c in clones]
        psis = family.draws(3)

        def refused(hams, amplitudes, match, fields=None):
            rc, message, statuses, _ = _raw_batch(family.stencil, hams, amplitudes, fields)
            assert rc == INVALID and match in message, message
            for clone, expected in zip(clones, before):
                assert_same(observe(clone, False), expected)

        # a plan of another pattern: another model, and the same states with one coupling less
        refused([clones[0], other.base], [psis[0], psis[1]], "item 1: pattern mismatch")
        thinner = family.draws(1)[0]
        thinner[17] = 0.0
        indptr, col, val = family.device.ising_csr(family.keys, thinner)
        assert col.shape[0] < family.col.shape[0]
        foreign = sa.Hamiltonian.from_canonical_csr(indptr, col, val, np.zeros(family.K))
        refused([clones[0], clones[1], foreign], psis, "item 2: pattern mismatch")
        # one plan twice
        refused([clones[0], clones[1], clones[0]], psis, "item 2: the plan of item 0 again")
        # a live Chains handle
        chains = sa.Chains(clones[1], seed=1, repetitions=2)
        refused(clones, psis, "item 1: the plan has 1 live chains")
        chains.close()
        # NaN and inf amplitudes, an inf in a field
        for bad in (np.nan, np.inf, -np.inf):
            broken = psis.copy()
            broken[2, 100] = bad
            refused(clones, broken, "item 2: non-finite amplitude at 100")
        fields = np.zeros((3, family.K))
        fields[1, 7] = np.inf
        refused(clones, psis, "item 1: non-finite field at 7", fields)
        # couplings that overflow: found on the device, still before any plan is touched
        refused(clones, np.stack([psis[0], psis[1] * 1e160, psis[2]]), "item 1: couplings overflow double range")
        with pytest.raises(_lib.AspError, match="non-finite amplitude"):
            family.stencil.values(np.full(family.K, np.nan))
        # after all that the call goes through
        rc, message, statuses, _ = _raw_batch(family.stencil, clones, psis)
        assert rc == 0 and statuses == [0, 0, 0], message
        # a stencil used after close()
        family.stencil.close()
        with pytest.raises(ValueError, match="closed"):
            family.stencil.values(psis[0])
        with pytest.raises(ValueError, match="closed"):
            sa.reweight_hamiltonians(clones, family.stencil, psis)
        with pytest.raises(ValueError, match="closed"):
            family.stencil.info
        family.stencil.close()  # (twice is fine)
    finally:
        family.close()
        other.close()


def test_creation_refusals():
    from annealing_sign_problem_amd import _lib

    operator = _plain_ring(10)
    keys = operator.basis.states
    device = operator.device()
    psi = _amplitudes(np.random.default_rng(1), keys.shape[0])
    indptr, col, _ = device.ising_csr(keys, psi)
    with pytest.raises(_lib.AspError, match="not sorted"):
        device.ising_stencil(keys[::-1].copy(), indptr, col)
    with pytest.raises(_lib.AspError, match="not sorted"):
        device.ising_stencil(np.concatenate([keys[:1], keys[:-1]]), indptr, col)
    # an entry that no connection produces: (0, j) and (j, 0) for a state j that row 0 does not reach
    dense = np.zeros(keys.shape[0], dtype=bool)
    dense[col[indptr[0]:indptr[1]]] = True
    j = int(np.flatnonzero(~dense)[-1])
    import scipy.sparse

    extra = scipy.sparse.csr_matrix((np.ones(col.shape[0]), col, indptr), shape=(keys.shape[0],) * 2).tolil()
    extra[0, j] = extra[j, 0] = 1.0
    extra = extra.tocsr()
    extra.sort_indices()
    with pytest.raises(_lib.AspError, match=r"pattern entry \(0, %d\) is produced by no connection" % j):
        device.ising_stencil(keys, extra.indptr, extra.indices)
    # a pattern with (i, j) and without (j, i)
    lopsided = extra.tolil()
    lopsided[0, j] = 0.0
    lopsided = lopsided.tocsr()
    lopsided.eliminate_zeros()
    with pytest.raises(_lib.AspError):
        device.ising_stencil(keys, lopsided.indptr, lopsided.indices)
    first = int(next(c for c in col[indptr[0]:indptr[1]] if c != 0))
    halved = scipy.sparse.csr_matrix((np.ones(col.shape[0]), col, indptr), shape=(keys.shape[0],) * 2).tolil()
    halved[0, first] = 0.0
    halved = halved.tocsr()
    halved.eliminate_zeros()
    with pytest.raises(_lib.AspError, match=r"pattern holds \(%d, 0\) without its mirror entry" % first):
        device.ising_stencil(keys, halved.indptr, halved.indices)
    # a key outside the sector (spin inversion -1 drops the orbits of norm 0), as ising_csr refuses it
    from annealing_sign_problem_amd import operators, symmetry

    n = 8
    group = symmetry.SymmetryGroup(n, [[(i + 1) % n for i in range(n)]], -1)
    odd = operators.Operator(operators.SpinBasis(n, n // 2, group),
                             [operators.Term(operators.SIGMA_DOT_SIGMA, [(i, (i + 1) % n) for i in range(n)])])
    outside = np.array([0b01010101], dtype=np.uint64)  # its shift is its inverse: character -1 in the stabiliser
    with pytest.raises(_lib.AspError, match="outside the symmetry sector"):
        odd.device().ising_csr(outside, np.ones(1))
    with pytest.raises(_lib.AspError, match="outside the symmetry sector"):
        odd.device().ising_stencil(outside, np.array([0, 1]), np.array([0]))
    # single-site flips with one-directional elements: ising_csr sends the caller to the host route with
    # ASP_ERR_INVALID, and so does the stencil, whatever symmetric pattern it is given
    flips, cluster = _random("single_flip")
    psi = _amplitudes(np.random.default_rng(2), cluster.shape[0])
    with pytest.raises(_lib.AspError) as refused:
        flips.device().ising_csr(cluster, psi)
    assert refused.value.code == INVALID and "host route" in str(refused.value)
    K = cluster.shape[0]
    with pytest.raises(_lib.AspError) as refused:
        flips.device().ising_stencil(cluster, np.arange(K + 1), np.arange(K))
    assert refused.value.code == INVALID and "host route" in str(refused.value)


# ---- models ------------------------------------------------------------------------------------------------
def _assert_same_model(got, want):
    from annealing_sign_problem_amd import annealer as sa

    a, b = got.ising_hamiltonian.exchange, want.ising_hamiltonian.exchange
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(_bits(a.data), _bits(b.data))
    assert np.array_equal(_bits(got.ising_hamiltonian.field), _bits(want.ising_hamiltonian.field))
    assert np.array_equal(got.initial_signs, want.initial_signs) and np.array_equal(got.spins, want.spins)
    for tree in ("host", "device"):
        x_got, e_got = sa.greedy_solve(got.ising_hamiltonian, tree=tree)
        x_want, e_want = sa.greedy_solve(want.ising_hamiltonian, tree=tree)
        assert np.array_equal(x_got, x_want) and e_got == e_want


def test_reweight_ising_models_equals_the_per_model_route():
    from annealing_sign_problem_amd import common

    operator = _plain_ring(10)
    basis = operator.basis
    _, ground_state = operator.ground_state()
    base = common.make_ising_model(basis.states, operator,
                                   log_psi_fn=common.ground_state_to_log_coeff_fn(ground_state, basis))
    base.ising_hamiltonian.plan()
    np.random.seed(11)
    try:
        pool = None
        for round_ in range(2):
            noisy = [common.add_noise_to_amplitudes(ground_state, eps=1.0) for _ in range(4)]
            fns = [common.ground_state_to_log_coeff_fn(x, basis) for x in noisy]
            builds = _build_count()
            # two draws by closure, two by log_psi (one of them with both)
            log_psis = [None, None, fns[2](basis.states), fns[3](basis.states)]
            got = common.reweight_ising_models(base, log_psis=log_psis, log_psi_fns=[fns[0], fns[1], None, fns[3]],
                                               outs=pool)
            assert _build_count() == builds and len(got) == 4
            if pool is not None:
                assert all(g is p for g, p in zip(got, pool))
            for g, fn in zip(got, fns):
                assert np.shares_memory(g.ising_hamiltonian.exchange.indices, base.ising_hamiltonian.exchange.indices)
                assert g.ising_hamiltonian.family() is base.ising_hamiltonian.family()
                want = common.reweight_ising_model(base, log_psi_fn=fn)
                _assert_same_model(g, want)
                _assert_same_model(g, common.make_ising_model(basis.states, operator, log_psi_fn=fn))
                want.ising_hamiltonian.release()
            pool = got
        stencil = base.ising_hamiltonian.family()["stencil"]
        assert stencil.info.num_spins == 252
        for model in pool:
            model.ising_hamiltonian.release()
        assert stencil._handle  # (a clone's release leaves the family's stencil alone)
    finally:
        base.ising_hamiltonian.release()
    assert not stencil._handle and "stencil" not in base.ising_hamiltonian.family()  # released with the base model


@pytest.mark.parametrize("direction", ["a stored pair vanishes", "a silent pair fires"])
def test_pattern_changes_are_reported_and_touch_nothing(direction):
    from annealing_sign_problem_amd import common

    operator = _plain_ring(10)
    basis = operator.basis
    keys = basis.states
    device = operator.device()
    rng = np.random.default_rng(3)
    K = keys.shape[0]
    positive = np.exp(rng.normal(scale=1.5, size=(4, K)))
    positive /= np.linalg.norm(positive, axis=1, keepdims=True)
    psi0 = positive[0].copy()
    if direction == "a silent pair fires":
        psi0[17] = 0.0
    with np.errstate(divide="ignore"):
        base = common.make_ising_model(keys, operator, log_psi=np.log(psi0.astype(np.complex128)))
    base.ising_hamiltonian.plan()
    exchange = base.ising_hamiltonian.exchange
    try:
        with device.ising_stencil(keys, exchange.indptr, exchange.indices) as stencil:
            if direction == "a silent pair fires":
                assert stencil.info.silent_pairs > 0
                moved = [positive[1]]
                kept = positive[2].copy()
                kept[17] = 0.0
            else:
                moved = []
                for zero in (0.0, -0.0):
                    moved.append(positive[1].copy())
                    moved[-1][40] = zero
                kept = positive[2]
            data, status = stencil.values(np.stack(moved + [kept]))
            assert status.tolist() == [1] * len(moved) + [0]
            assert np.array_equal(_bits(data[-1]), _bits(device.ising_csr(keys, kept)[2]))
            # the plans: the draw that moved leaves its plan as it was, the other one is applied
            clones = [base.ising_hamiltonian.clone() for _ in range(len(moved) + 1)]
            before = observe(clones[0], False)
            old_data = [c.exchange.data for c in clones]
            rc, message, statuses, _ = _raw_batch(stencil, clones, np.stack(moved + [kept]))
            assert rc == 0 and statuses == [1] * len(moved) + [0], message
            for clone, data_before in zip(clones[:-1], old_data):
                assert_same(observe(clone, False), before)
                assert clone.exchange.data is data_before
            indptr, col, val = device.ising_csr(keys, kept)
            from annealing_sign_problem_amd import annealer as sa

            fresh = sa.Hamiltonian.from_canonical_csr(indptr, col, val, np.zeros(K))
            assert_same(observe(clones[-1]), observe(fresh))
            for clone in clones:
                clone.release()
        # the models: the draw that moved is make_ising_model's, the others still come from the stencil
        with np.errstate(divide="ignore"):
            log_psis = [np.log(x.astype(np.complex128)) for x in [kept, moved[0], positive[3] if direction.startswith("a stored") else kept]]
            builds = _build_count()
            got = common.reweight_ising_models(base, log_psis=log_psis)
            sa.greedy_solve_batch([g.ising_hamiltonian for g in got])
            assert _build_count() - builds == 1  # the one model that make_ising_model built
            shared = [np.shares_memory(g.ising_hamiltonian.exchange.indices, exchange.indices) for g in got]
            assert shared == [True, False, True]
            for g, log_psi in zip(got, log_psis):
                _assert_same_model(g, common.make_ising_model(keys, operator, log_psi=log_psi))
    finally:
        base.ising_hamiltonian.release()


def test_an_operator_the_stencil_refuses_takes_the_per_model_route():
    from annealing_sign_problem_amd import common

    operator, keys = _random("single_flip")
    rng = np.random.default_rng(8)
    log_psis = [np.log(_amplitudes(rng, keys.shape[0]).astype(np.complex128)) for _ in range(3)]
    base = common.make_ising_model(keys, operator, log_psi=log_psis[0])
    try:
        got = common.reweight_ising_models(base, log_psis=log_psis[1:])
        assert base.ising_hamiltonian.family()["stencil"] is False
        for g, log_psi in zip(got, log_psis[1:]):
            _assert_same_model(g, common.make_ising_model(keys, operator, log_psi=log_psi))
    finally:
        base.ising_hamiltonian.release()


# ---- the noise study ---------------------------------------------------------------------------------------
def _rows(operator, ground_state, levels, repetitions, **how):
    from annealing_sign_problem_amd.influence_of_noise import influence_of_noise

    return ["{},{},{}\n".format(*row).encode()
            for row in influence_of_noise(operator, ground_state, levels, repetitions, seed=435834, **how)]


def test_noise_rows_do_not_depend_on_the_route():
    """A condition, not a measurement: no draw may fall back (one build per run)."""
    operator = _plain_ring(10)
    _, ground_state = operator.ground_state()
    levels = np.exp(np.linspace(np.log(1e-2), np.log(1e2), 3))
    fresh = _rows(operator, ground_state, levels, 3, reuse=False)
    assert len(fresh) == 9 and len(set(fresh)) == 9
    builds = _build_count()
    assert _rows(operator, ground_state, levels, 3, from_amplitudes=True, batch=4) == fresh
    assert _build_count() - builds == 1
    assert _rows(operator, ground_state, levels, 3, from_amplitudes=True, batch=1) == fresh
    assert _build_count() - builds == 2


def test_noise_rows_on_kagome_16(models):
    """Identical rows and exactly one build also at eps = 100: DESIGN.md §4.14 records the smallest |J|
    there as 7e-184, far from underflow."""
    from annealing_sign_problem_amd import operators

    operator = operators.Operator.from_config(models["heisenberg_kagome_16"])
    operator.basis.build()
    _, ground_state = operator.ground_state()
    assert operator.basis.number_states == 12870
    fresh = _rows(operator, ground_state, [0.01, 100.0], 2, reuse=False)
    builds = _build_count()
    assert _rows(operator, ground_state, [0.01, 100.0], 2, from_amplitudes=True, batch=4) == fresh
    assert _build_count() - builds == 1
