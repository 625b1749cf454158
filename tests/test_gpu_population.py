"""Population annealing on resumable chains (asp_sa_chains_gather / _resample / _resample_batch,
annealer.Chains.gather / .resample, resample_chains, population_anneal(_batch)).

Every comparison is exact: np.array_equal on words and integers, energies compared as bytes.  The
checker is law ASP-PA-1 restated in Python integers (tests/population_law.py) on energies that are
themselves checked against the CPU oracle (oracle.sa_energy), and numpy fancy indexing of exported
state for the gather — never the code against itself.  Problems come from synthetic.planted_cluster
with a small random field, as in tests/test_gpu_chains.py.
"""
import ctypes

import numpy as np
import pytest

import oracle
import population_law as law

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -3, -4
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def _problem(n, seed):
    from annealing_sign_problem_amd import synthetic

    if n == 0:
        import scipy.sparse

        return scipy.sparse.csr_matrix((0, 0)), np.zeros(0)
    J, _, _ = synthetic.planted_cluster(n, seed=seed)
    h = np.random.default_rng(seed).normal(size=n) * 0.01
    return J, h


def _ham(n, seed):
    from annealing_sign_problem_amd import annealer as sa

    J, h = _problem(n, seed)
    return J, h, sa.Hamiltonian(J, h)


def _betas(J, count):
    """A ladder around the couplings' scale (hot enough that chains move, cold enough that they differ)."""
    scale = (float(np.abs(J.data).max()) if J.nnz else 0.0) or 1.0
    return np.geomspace(0.05 / scale, 2.0 / scale, count)


def _same(a, b):
    for name in STATE:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert a[name].tobytes() == b[name].tobytes(), name
    assert int(a["sweeps_done"]) == int(b["sweeps_done"])


def _resample_c(chains, dbeta, draw=0):
    """The single call of the C ABI with every output: (rc, source, energy, q, survivors)."""
    from annealing_sign_problem_amd import _lib

    R = chains.repetitions
    source = np.full(R, 0xDEAD, dtype=np.uint32)
    energy = np.full(R, -77.0)
    q = np.full(R, 0xDEAD, dtype=np.uint64)
    survivors = ctypes.c_uint32(0xDEAD)
    rc = _lib.load().asp_sa_chains_resample(chains._live(), ctypes.c_double(dbeta), ctypes.c_uint32(draw),
                                            _lib.ptr(source), _lib.ptr(energy), _lib.ptr(q), ctypes.byref(survivors))
    return rc, source, energy, q, survivors.value


def _untouched(source, energy, q, survivors):
    return np.all(source == 0xDEAD) and np.all(energy == -77.0) and np.all(q == 0xDEAD) and survivors == 0xDEAD


def _check_step(chains, J, h, dbeta, draw):
    """One resample through the C ABI against the oracle's energies and the restated law."""
    before = chains.state()
    rc, source, energy, q, survivors = _resample_c(chains, dbeta, draw)
    assert rc == 0
    assert energy.tobytes() == oracle.sa_energy(J, h, before["x_current"]).tobytes()
    lq, lsource, lsurvivors = law.resample(energy, dbeta, chains.seed, int(before["sweeps_done"]), draw)
    assert np.array_equal(q, lq) and np.array_equal(source, lsource) and survivors == lsurvivors
    _same(chains.state(), law.gathered(before, source))
    return source, energy, q, survivors


# ---- gather ------------------------------------------------------------------------------------------

def _maps(R, rng):
    return {"identity": np.arange(R), "all to one": np.full(R, R // 2), "reversal": np.arange(R)[::-1],
            "random": rng.integers(R, size=R)}


@pytest.mark.parametrize("R", [1, 3, 64, 257])
@pytest.mark.parametrize("K", [1, 64, 65, 200])
def test_gather_is_fancy_indexing(K, R):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham = _ham(K, 10 + K)
    betas = _betas(J, 4 + 4 * 16)
    rng = np.random.default_rng(K * 1000 + R)
    with sa.Chains(ham, seed=21, repetitions=R, replica_offset=3) as a, \
            sa.Chains(ham, seed=21, repetitions=R, replica_offset=3) as b:
        a.advance(betas[:4], sweep_order="colour")  # (best and current differ, integers are non-zero)
        done = 4
        for name, source in _maps(R, rng).items():
            before = a.state()
            a.gather(source)
            expected = law.gathered(before, source)
            _same(a.state(), expected)
            # ... and the handle goes on exactly as one loaded with the numpy result; entry 0 of a trace is
            # the host's mirror of the current tracked energies, which moves with the chains
            b.load_state(expected)
            current = expected["tracked_current"]
            for order in ("colour", "shuffled"):
                ta = a.advance(betas[done:done + 8], sweep_order=order, trace=True)
                tb = b.advance(betas[done:done + 8], sweep_order=order, trace=True)
                done += 8
                assert np.array_equal(ta, tb) and np.array_equal(ta[:, 0], current), (name, order)
                current = ta[:, -1]
            _same(a.state(), b.state())
            ra, rb = a.result(), b.result()
            assert np.array_equal(ra[0], rb[0]) and ra[1].tobytes() == rb[1].tobytes()


def test_gather_rejects_an_entry_beyond_the_chains():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham = _ham(65, 3)
    with sa.Chains(ham, seed=2, repetitions=5) as chains:
        chains.advance(_betas(J, 3), sweep_order="shuffled")
        before = chains.state()
        for bad in ([0, 1, 5, 3, 4], [0, 1, 2, 3, 2 ** 32 - 1]):
            source = np.array(bad, dtype=np.uint32)
            assert _lib.load().asp_sa_chains_gather(chains._live(), _lib.ptr(source)) == INVALID
            assert "source[" in _lib.last_error()
            _same(chains.state(), before)
        assert _lib.load().asp_sa_chains_gather(chains._live(), None) == INVALID
        with pytest.raises(ValueError):
            chains.gather([0, 1, 2])
        with pytest.raises(ValueError):
            chains.gather([0, 1, 2, 3, -1])
        _same(chains.state(), before)
        chains.gather([4, 4, 0, 0, 2])
        _same(chains.state(), law.gathered(before, [4, 4, 0, 0, 2]))


# ---- resample against the law ------------------------------------------------------------------------

@pytest.mark.parametrize("sweeps", [0, 16])
@pytest.mark.parametrize("K", [40, 300])
def test_resample_is_the_law(K, sweeps):
    from annealing_sign_problem_amd import annealer as sa

    R = 24
    J, h, ham = _ham(K, 40 + K)
    betas = _betas(J, 16)
    rng = np.random.default_rng(K)
    # starts in pairs: chains 2k and 2k + 1 tie before the first sweep (the minimum among them)
    half = np.stack([sa.signs_to_bits(np.where(rng.random(K) < 0.5, 1.0, -1.0)) for _ in range(R // 2)])
    x0 = np.repeat(half, 2, axis=0)

    def fresh():
        chains = sa.Chains(ham, seed=77, repetitions=R, x0=x0, replica_offset=1)
        chains.advance(betas[:sweeps], sweep_order="shuffled")
        assert chains.sweeps_done == sweeps
        return chains

    with fresh() as probe:
        energies = oracle.sa_energy(J, h, probe.state()["x_current"])
    gaps = np.sort(energies - energies.min())
    spread, smallest = float(gaps[-1]), float(gaps[gaps > 0][0])
    assert spread > 0
    ties = int(np.sum(gaps == 0))
    assert ties >= (2 if sweeps == 0 else 1)
    # dbeta = 0: the identity, whatever the draw
    with fresh() as chains:
        before = chains.state()
        source, _, q, survivors = _check_step(chains, J, h, 0.0, 3)
        assert np.array_equal(source, np.arange(R)) and np.all(q == 2 ** 31) and survivors == R
        _same(chains.state(), before)
    # every chain but the minimum is dead: all slots take the minimum, ties split them
    with fresh() as chains:
        big = 24.0 / smallest
        assert big * smallest >= 23.0
        source, energy, q, survivors = _check_step(chains, J, h, big, 0)
        lowest = np.flatnonzero(energy == energy.min())
        assert survivors == len(lowest) == ties and set(source) == set(lowest)
        assert np.all(q[lowest] == 2 ** 31) and int(q.sum()) == ties * 2 ** 31
        shares = np.bincount(source, minlength=R)[lowest]
        assert shares.min() >= R // ties and shares.max() <= -(-R // ties)
    # two moderate steps; the draw index and sweeps_done enter the random offset
    told = {}
    for dbeta, draw in ((3.0 / spread, 0), (3.0 / spread, 7), (10.0 / spread, 0), (10.0 / spread, 7)):
        with fresh() as chains:
            source, _, q, survivors = _check_step(chains, J, h, dbeta, draw)
            assert len(set(q.tolist())) > 2  # (a condition on the inputs: unequal weights)
            told[(dbeta, draw)] = source
            if draw == 0 and dbeta == 3.0 / spread:
                # the Python face runs the same call, and a second step on the resampled population
                with fresh() as twin:
                    psource, penergy, psurvivors = twin.resample(dbeta)
                    assert np.array_equal(psource, source) and psurvivors == survivors
                    _same(twin.state(), chains.state())
                _check_step(chains, J, h, dbeta, 1)
                chains.advance(betas[:5], sweep_order="colour")
                _check_step(chains, J, h, dbeta, 0)
    # (with unequal weights another offset moves some slot to another source — for these inputs, as the law
    # says too: both maps were compared with it above)
    assert law.draw_word(77, sweeps, 0) != law.draw_word(77, sweeps, 7)
    assert any(not np.array_equal(told[(c / spread, 0)], told[(c / spread, 7)]) for c in (3.0, 10.0))


def test_resample_at_the_64_bit_bound_and_beyond():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham = _ham(8, 8)
    with sa.Chains(ham, seed=5, repetitions=65536) as chains:
        energies = oracle.sa_energy(J, h, chains.state()["x_current"])
        spread = float(energies.max() - energies.min())
        assert spread > 0
        # every weight is above exp(-1/2) > 1/2, so R T > 2^16 2^16 2^30: the products of the law are at the bound
        source, _, q, survivors = _check_step(chains, J, h, 0.5 / spread, 0)
        assert 2 ** 62 < 65536 * int(q.astype(object).sum()) <= 2 ** 63
        assert 1 < survivors < 65536
    with sa.Chains(ham, seed=5, repetitions=65537) as chains:
        before = chains.state()
        rc, *outputs = _resample_c(chains, 1.0, 0)
        assert rc == TOO_LARGE and "65537" in _lib.last_error() and _untouched(*outputs)
        _same(chains.state(), before)
        with pytest.raises(_lib.AspError):
            chains.resample(1.0)


def test_resample_rejects_steps_that_are_not_finite_and_non_negative():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham = _ham(40, 4)
    with sa.Chains(ham, seed=5, repetitions=6) as chains:
        chains.advance(_betas(J, 4), sweep_order="colour")
        before = chains.state()
        for dbeta in (-1e-300, -1.0, float("nan"), float("inf")):
            rc, *outputs = _resample_c(chains, dbeta, 0)
            assert rc == INVALID and "dbeta" in _lib.last_error() and _untouched(*outputs)
            _same(chains.state(), before)
        # every output may be NULL
        twin_before = chains.state()
        assert _lib.load().asp_sa_chains_resample(chains._live(), ctypes.c_double(0.5), ctypes.c_uint32(0), None, None,
                                                  None, None) == 0
        energies = oracle.sa_energy(J, h, twin_before["x_current"])
        _, lsource, _ = law.resample(energies, 0.5, 5, 4, 0)
        _same(chains.state(), law.gathered(twin_before, lsource))


# ---- batch -------------------------------------------------------------------------------------------

SHAPES = ((40, 64), (65, 3), (300, 257), (1, 1), (0, 4))  # (spins, chains); the last plan has no spins


def _batch_set():
    from annealing_sign_problem_amd import annealer as sa

    problems, chains = [], []
    for k, (K, R) in enumerate(SHAPES):
        J, h, ham = _ham(K, 60 + k)
        c = sa.Chains(ham, seed=300 + k, repetitions=R, replica_offset=k)
        c.advance(_betas(J, 3 + k)[:3 + k], sweep_order="colour" if k % 2 else "shuffled")  # (different sweeps_done)
        problems.append((J, h, ham))
        chains.append(c)
    return problems, chains


def _steps(problems, chains):
    out = []
    for (J, h, _), c in zip(problems, chains):
        if J.shape[0] == 0:
            out.append(0.7)
            continue
        e = oracle.sa_energy(J, h, c.state()["x_current"])
        spread = float(e.max() - e.min())
        out.append(4.0 / spread if spread > 0 else 0.7)
    return out


def _resample_batch_c(chains, dbetas, draws, order, flags=None):
    from annealing_sign_problem_amd import _lib

    items = (_lib.SaChainsResampleItem * len(order))()
    outputs = {}
    for slot, k in enumerate(order):
        R = chains[k].repetitions
        source = np.full(R, 0xDEAD, dtype=np.uint32)
        energy = np.full(R, -77.0)
        q = np.full(R, 0xDEAD, dtype=np.uint64)
        survivors = ctypes.c_uint32(0xDEAD)
        outputs[slot] = (source, energy, q, survivors)
        items[slot].chains = chains[k]._live()
        items[slot].dbeta = dbetas[k]
        items[slot].draw = draws[k]
        items[slot].flags = 0 if flags is None else flags[slot]
        items[slot].out_source = source.ctypes.data
        items[slot].out_energy = energy.ctypes.data
        items[slot].out_q = q.ctypes.data
        items[slot].out_survivors = ctypes.addressof(survivors)
    rc = _lib.load().asp_sa_chains_resample_batch(items, ctypes.c_uint32(len(order)))
    return rc, [(s, e, q, v.value) for s, e, q, v in (outputs[slot] for slot in range(len(order)))]


def test_batch_is_the_single_calls_in_any_order():
    from annealing_sign_problem_amd import _lib

    draws = (0, 1, 2, 3, 4)
    sets = [_batch_set() for _ in range(3)]
    dbetas = _steps(*sets[0])
    told = []
    for (problems, chains), order in zip(sets[:2], ((0, 1, 2, 3, 4), (3, 4, 2, 0, 1))):
        rc, outputs = _resample_batch_c(chains, dbetas, draws, order)
        assert rc == 0 and _lib.load().asp_sa_chains_resample_last_ms() > 0.0
        told.append({k: outputs[slot] for slot, k in enumerate(order)})
    problems, chains = sets[2]
    befores = [c.state() for c in chains]
    single = {}
    for k, c in enumerate(chains):
        rc, *outputs = _resample_c(c, dbetas[k], draws[k])
        assert rc == 0
        single[k] = tuple(outputs)
    for k, (K, R) in enumerate(SHAPES):
        for other in told:
            for x, y in zip(other[k][:3], single[k][:3]):
                assert x.tobytes() == y.tobytes(), k
            assert other[k][3] == single[k][3]
        _same(sets[0][1][k].state(), chains[k].state())
        _same(sets[1][1][k].state(), chains[k].state())
        source, energy, q, survivors = single[k]
        if K == 0:  # nothing runs: energies 0, every weight 1, the identity
            assert np.all(energy == 0.0) and np.all(q == 2 ** 31) and survivors == R
            assert np.array_equal(source, np.arange(R))
            _same(chains[k].state(), befores[k])
            continue
        J, h, _ = problems[k]
        assert energy.tobytes() == oracle.sa_energy(J, h, befores[k]["x_current"]).tobytes()
        lq, lsource, lsurvivors = law.resample(energy, dbetas[k], 300 + k, int(befores[k]["sweeps_done"]), draws[k])
        assert np.array_equal(q, lq) and np.array_equal(source, lsource) and survivors == lsurvivors
        _same(chains[k].state(), law.gathered(befores[k], source))
    assert 1 < single[0][3] < 64 and 1 < single[2][3] < 257  # (a condition on the inputs: something was cloned)
    for _, handles in sets:
        for c in handles:
            c.close()


def test_batch_errors_change_nothing():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    problems, chains = _batch_set()
    twin = sa.Chains(problems[0][2], seed=9, repetitions=2)  # a second handle of plan 0
    everyone = chains + [twin]
    before = [c.state() for c in everyone]
    dbetas = [0.5] * len(everyone)
    draws = [0] * len(everyone)

    def call(order, flags=None, steps=None):
        rc, outputs = _resample_batch_c(everyone, dbetas if steps is None else steps, draws, order, flags)
        message = _lib.last_error()
        for out in outputs:
            assert _untouched(*out)
        for c, state in zip(everyone, before):
            _same(c.state(), state)
        return rc, message

    rc, message = call((0, 1, 0))
    assert rc == INVALID and "same handle" in message and "0" in message and "2" in message
    rc, message = call((0, 1, 5))
    assert rc == INVALID and "one plan" in message and "0" in message and "2" in message
    rc, message = call((0, 1, 2), flags=(0, 0, 1))
    assert rc == INVALID and "item 2" in message and "flags" in message
    rc, message = call((0, 1, 2), steps=[0.5, float("nan"), 0.5, 0.5, 0.5, 0.5])
    assert rc == INVALID and "item 1" in message and "dbeta" in message
    with pytest.raises(_lib.AspError):
        sa.resample_chains([chains[0], twin], 0.5)
    for c in everyone:
        c.close()


def test_batched_and_single_steps_alternate():
    """Batched and single resamples between batched and single segments on the same handles: whichever
    call runs a step, the handles hold the same bits."""
    from annealing_sign_problem_amd import annealer as sa

    (problems, set_a), (_, set_b) = _batch_set(), _batch_set()
    handles = range(len(SHAPES))
    ladders = [_betas(J, 12) for J, _, _ in problems]
    orders = ["shuffled", "colour", "shuffled", "colour", "shuffled"]
    done = 0
    # (batched segment?, batched resample?) of set a; set b does every step the other way
    for round_, (segment_a, resample_a) in enumerate(((True, False), (False, True), (True, True))):
        parts = [ladder[done:done + 4] for ladder in ladders]
        done += 4
        dbetas = _steps(problems, set_a)
        told = []
        for chains, batched_segment, batched_resample in ((set_a, segment_a, resample_a),
                                                          (set_b, not segment_a, not resample_a)):
            if batched_segment:
                sa.advance_chains(chains, parts, sweep_order=orders)
            else:
                for k in handles:
                    chains[k].advance(parts[k], sweep_order=orders[k])
            if batched_resample:
                told.append(sa.resample_chains(chains, dbetas, round_))
            else:
                told.append([chains[k].resample(dbetas[k], round_) for k in handles])
        for k in handles:
            _same(set_a[k].state(), set_b[k].state())
            (source_a, energy_a, survivors_a), (source_b, energy_b, survivors_b) = told[0][k], told[1][k]
            assert np.array_equal(source_a, source_b) and energy_a.tobytes() == energy_b.tobytes()
            assert survivors_a == survivors_b
    for c in set_a + set_b:
        c.close()


# ---- drivers -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_population_anneal(order):
    from annealing_sign_problem_amd import annealer as sa

    steps, per, R, seed = 6, 4, 16, 5
    J, h = _problem(300, 70)
    make = lambda: sa.Hamiltonian(J, h)
    info = make().info()
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, steps)
    kw = dict(seed=seed, number_steps=steps, sweeps_per_step=per, repetitions=R, sweep_order=order)
    # without resampling: the closed call on the repeated ladder (the continuation law)
    xs, es = sa.population_anneal(make(), only_best=False, resample=False, **kw)
    cxs, ces = sa.anneal_raw(make(), seed, np.repeat(ladder, per), R, shuffled=order == "shuffled")
    assert np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes()
    # with it: the route through the host — advance, state(), the law in numpy, load_state()
    xs, es = sa.population_anneal(make(), only_best=False, **kw)
    ham = make()
    cloned = 0
    with sa.Chains(ham, seed=seed, repetitions=R) as chains:
        for k in range(steps):
            if k >= 1:
                state = chains.state()
                energies = oracle.sa_energy(J, h, state["x_current"])
                _, source, survivors = law.resample(energies, ladder[k] - ladder[k - 1], seed, k * per, 0)
                cloned += R - survivors
                chains.load_state(law.gathered(state, source))
            chains.advance(np.full(per, ladder[k]), sweep_order=order)
        hxs, hes = chains.result()
    assert cloned > 0  # (a condition on the inputs: the resampling did something)
    assert np.array_equal(xs, hxs) and es.tobytes() == hes.tobytes()
    assert es.tobytes() == ham.energies(xs).tobytes()
    assert not (np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes())
    x, e = sa.population_anneal(make(), **kw)
    best = int(np.argmin(es))
    assert np.array_equal(x, xs[best]) and np.float64(e).tobytes() == es[best].tobytes()


def test_population_anneal_batch_is_the_single_calls():
    from annealing_sign_problem_amd import annealer as sa

    problems = [_problem(n, 80 + k) for k, n in enumerate((40, 130, 300))]
    kw = dict(number_steps=5, sweeps_per_step=3, repetitions=8, only_best=False, sweep_order="shuffled")
    batch = sa.population_anneal_batch([sa.Hamiltonian(J, h) for J, h in problems], seed=[3, 4, 5], **kw)
    for k, (J, h) in enumerate(problems):
        xs, es = sa.population_anneal(sa.Hamiltonian(J, h), seed=3 + k, **kw)
        assert np.array_equal(batch[k][0], xs) and batch[k][1].tobytes() == es.tobytes()
