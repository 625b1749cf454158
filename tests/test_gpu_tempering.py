"""Parallel tempering on resumable chains (asp_sa_chains_advance_ladder / _exchange, annealer.Chains
.advance_ladder / .exchange, parallel_tempering; DESIGN.md §4.10 "Ladder law" and §4.12).

Every comparison is exact: np.array_equal on words, integers and traces, energies compared as bytes.
The references are a one-chain handle run on the constant ladder, the CPU oracle (oracle.sa_anneal /
sa_anneal_shuffled), Hamiltonian.energies, the law restated in tests/tempering_law.py and numpy
indexing of an exported state (tests/population_law.gathered) — never the code against itself.
Problems come from synthetic.planted_cluster, like those of tests/test_gpu_chains.py.

What comes out when sweeps, exchange and cluster moves are composed is tested in
tests/test_gpu_ensemble_law.py against the exact joint law of tests/ensemble_exact_law.py, which is
independent of the restated law used here.
"""
import ctypes

import numpy as np
import pytest

import oracle
import population_law
import tempering_law as law

pytestmark = pytest.mark.gpu

INVALID = -3
ORDERS = {0: "colour", 1: "shuffled"}
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def _case(n, seed=5):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, _, planted = synthetic.planted_cluster(n, seed=seed)
    h = np.random.default_rng(seed).normal(size=n) * 0.01
    ham = sa.Hamiltonian(J, h)
    return J, h, ham, ham.info(), planted


def _random_x0(n, seed, rows):
    from annealing_sign_problem_amd import annealer as sa

    rng = np.random.default_rng(seed)
    return np.stack([sa.signs_to_bits(np.where(rng.random(n) < 0.5, 1.0, -1.0)) for _ in range(rows)])


def _chain_betas(info, R):
    """R distinct, unsorted inverse temperatures around the plan's automatic range, among them (from
    three chains on) a 0 and one that freezes every proposal with dE > 0."""
    lo, hi = max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6)
    pool = list(np.geomspace(lo, hi, 13))
    pool = [pool[k] for k in (6, 12, 0, 9, 3, 11, 1, 7, 4, 10, 2, 8, 5)]
    pool[1], pool[2] = 0.0, 1e9
    return np.array(pool[:R], dtype=np.float64)


def _same_state(a, b, rows=None):
    for name in STATE:
        left = np.asarray(a[name]) if rows is None else np.asarray(a[name])[rows]
        assert np.array_equal(left, np.asarray(b[name])), name
    assert int(a["sweeps_done"]) == int(b["sweeps_done"])


def _form(ham):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    spins, wgs = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(lib.asp_sa_last_shuffled_blocks(ham.plan(), ctypes.byref(spins), ctypes.byref(wgs)))
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return lib.asp_sa_last_layout(ham.plan()), spins.value, m.value


# ---- the ladder law ------------------------------------------------------------------------------------
N1, NMID, N2 = 7, 5, 6


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("R", [1, 3, 13])
@pytest.mark.parametrize("K", [40, 300])
def test_ladder_law(order, K, R):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(K, seed=K + R)
    off, seed = 5, 1234 + R
    betas = _chain_betas(info, R)
    middle = sa.make_schedule(max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6), NMID)
    name = ORDERS[order]
    for x0 in (None, _random_x0(K, 3, R)):
        with sa.Chains(ham, seed=seed, repetitions=R, x0=x0, replica_offset=off) as chains:
            trace1 = chains.advance_ladder(betas, N1, sweep_order=name, trace=True)
            state1 = chains.state()
            chains.advance(middle, sweep_order=name)
            trace2 = chains.advance_ladder(betas, N2, sweep_order=name, trace=True)
            state2 = chains.state()
            xs, es = chains.result()
        assert trace1.shape == (R, N1 + 1) and trace2.shape == (R, N2 + 1)
        assert int(state1["sweeps_done"]) == N1 and int(state2["sweeps_done"]) == N1 + NMID + N2
        for r in range(R):
            start = None if x0 is None else x0[r]
            with sa.Chains(ham, seed=seed, repetitions=1, x0=start, replica_offset=off + r) as alone:
                row1 = alone.advance(np.full(N1, betas[r]), sweep_order=name, trace=True)
                _same_state(state1, alone.state(), rows=slice(r, r + 1))
                alone.advance(middle, sweep_order=name)
                row2 = alone.advance(np.full(N2, betas[r]), sweep_order=name, trace=True)
                _same_state(state2, alone.state(), rows=slice(r, r + 1))
            assert np.array_equal(trace1[r], row1[0]) and np.array_equal(trace2[r], row2[0])
            # ... and the CPU oracle's chain on the same schedule
            schedule = np.concatenate([np.full(N1, betas[r]), middle, np.full(N2, betas[r])])
            run = oracle.sa_anneal_shuffled if order == 1 else oracle.sa_anneal
            ox, oe, otracked, oaccepted = run(J, h, seed, schedule, 1, off + r, start, info.energy_scale_exp)
            assert np.array_equal(xs[r], ox[0]) and es[r:r + 1].tobytes() == oe.tobytes()
            assert state2["tracked_best"][r] == otracked[0] and state2["accepted"][r] == oaccepted[0]
        # a frozen chain accepts no uphill flip, a chain at beta = 0 every proposal
        if R >= 3:
            assert np.all(np.diff(trace1[2]) <= 0)
            assert state1["accepted"][1] == N1 * K


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("K,R", [(40, 1), (300, 13)])
def test_equal_betas_are_advance_bit_for_bit(order, K, R):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(K, seed=K)
    beta = float(np.sqrt(max(info.beta0_auto, 1e-3) * min(max(info.beta1_auto, 1.0), 1e6)))
    x0 = _random_x0(K, 4, R)
    with sa.Chains(ham, seed=77, repetitions=R, x0=x0, replica_offset=2) as ladder:
        got = ladder.advance_ladder(np.full(R, beta), 9, sweep_order=ORDERS[order], trace=True)
        state = ladder.state()
    with sa.Chains(ham, seed=77, repetitions=R, x0=x0, replica_offset=2) as plain:
        want = plain.advance(np.full(9, beta), sweep_order=ORDERS[order], trace=True)
        _same_state(state, plain.state())
    assert np.array_equal(got, want)


_LARGE = {}


def _large(k):
    """The cluster of tests/test_gpu_sa_trace_shuffled.py::test_trace_in_the_layouts_of_large_clusters (mean
    degree 6), built once per size."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    if k not in _LARGE:
        J, h, _ = synthetic.planted_cluster(k, seed=5, mean_degree=6.0)
        ham = sa.Hamiltonian(J, h)
        info = ham.info()
        _LARGE[k] = ham, float(np.sqrt(max(info.beta0_auto, 1e-3) * min(max(info.beta1_auto, 1.0), 1e6)))
    return _LARGE[k]


@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("k,forced_m,expect_m", [(70000, 4, 4), (170000, 4, 4), (300000, 0, 1)])
def test_equal_betas_are_advance_in_the_layouts_of_large_clusters(k, forced_m, expect_m, trace):
    """The ladder kernels in a byte, four bits and one bit per spin (clusters beyond a word per spin; the
    layout is whatever fits the LDS), five chains — at four per group the last group is ragged —: the
    shuffled ladder segment with equal betas is the plain segment, in state and in trace."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham, beta = _large(k)
    _lib.check(_lib.load().asp_sa_set_shuffled_launch(ham.plan(), forced_m, 0))
    R, sweeps = 5, 5
    with sa.Chains(ham, seed=4321, repetitions=R, replica_offset=2) as ladder:
        got = ladder.advance_ladder(np.full(R, beta), sweeps, sweep_order="shuffled", trace=trace)
        assert _form(ham)[2] == expect_m
        state = ladder.state()
    with sa.Chains(ham, seed=4321, repetitions=R, replica_offset=2) as plain:
        want = plain.advance(np.full(sweeps, beta), sweep_order="shuffled", trace=trace)
        assert _form(ham)[2] == expect_m
        _same_state(state, plain.state())
    if trace:
        assert got.shape == (R, sweeps + 1) and np.array_equal(got, want)


def test_zero_sweeps_write_column_zero_only():
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(65, seed=1)
    with sa.Chains(ham, seed=3, repetitions=3) as chains:
        chains.advance_ladder([0.5, 0.1, 2.0], 4, sweep_order="colour")
        before = chains.state()
        trace = chains.advance_ladder([0.5, 0.1, 2.0], 0, sweep_order="shuffled", trace=True)
        assert trace.shape == (3, 1) and np.array_equal(trace[:, 0], before["tracked_current"])
        _same_state(chains.state(), before)


# ---- launch forms --------------------------------------------------------------------------------------
FORMS_K, FORMS_R, FORMS_SWEEPS = 900, 13, 12
_UNFORCED = {}


def _forms_run(order, prepare=None):
    """(state, trace, form) of a ladder segment, a plain segment and a second ladder segment of 13 chains
    on the 900-spin problem, on a plan of its own that `prepare` may force a launch form on."""
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(FORMS_K, seed=17)
    if prepare is not None:
        prepare(ham.plan())
    betas = _chain_betas(info, FORMS_R)
    with sa.Chains(ham, seed=4242, repetitions=FORMS_R, x0=_random_x0(FORMS_K, 5, FORMS_R), replica_offset=3) as chains:
        first = chains.advance_ladder(betas, FORMS_SWEEPS, sweep_order=ORDERS[order], trace=True)
        form = _form(ham)
        chains.advance(betas[3:8], sweep_order=ORDERS[order])
        second = chains.advance_ladder(betas[::-1].copy(), 5, sweep_order=ORDERS[order], trace=True)
        state = chains.state()
    return state, np.concatenate([first, second], axis=1), form


def _unforced(order):
    if order not in _UNFORCED:
        _UNFORCED[order] = _forms_run(order)
    return _UNFORCED[order]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("m", [2, 4, 8])
def test_forced_chains_per_group_give_the_unforced_bits(order, m):
    """asp_sa_set_launch / asp_sa_set_shuffled_launch: 2, 4 (colour: the word layout) and 8 chains per
    workgroup for 13 chains — the last group is padded, its chains run at beta = 0."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()

    def prepare(plan):
        _lib.check(lib.asp_sa_set_launch(plan, m, 0))
        _lib.check(lib.asp_sa_set_shuffled_launch(plan, m, 0))

    state, trace, (layout, spins_per_block, chains) = _forms_run(order, prepare)
    assert chains == m, "the forced group size was honoured"
    if order == 0:
        assert layout == (2 if m == 4 else 0)
    want_state, want_trace, _ = _unforced(order)
    _same_state(state, want_state)
    assert np.array_equal(trace, want_trace)


@pytest.mark.parametrize("packed", [1, 2])
def test_forced_bit_layouts_give_the_unforced_bits(packed):
    """asp_sa_set_packed(1) / (2): a bit per position in LDS / in HBM (colour order)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    state, trace, (layout, _, chains) = _forms_run(0, lambda plan: _lib.check(lib.asp_sa_set_packed(plan, packed)))
    assert layout == (1 if packed == 1 else 3) and chains == 1
    want_state, want_trace, _ = _unforced(0)
    _same_state(state, want_state)
    assert np.array_equal(trace, want_trace)


def test_lane_packed_shuffled_ladder_gives_the_unpacked_bits():
    """The shuffled order packs several groups of chains into a wavefront on a small cluster (blocks of
    fewer than 64 spins); with four wavefronts' worth of chains per group forced apart it does not."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(300, seed=9)
    betas = _chain_betas(info, 13)
    results = []
    for m in (0, 8):  # automatic (lane packing), eight chains per group (bytes: never packed)
        J, h, ham, info, _ = _case(300, seed=9)
        if m:
            _lib.check(_lib.load().asp_sa_set_shuffled_launch(ham.plan(), m, 0))
        with sa.Chains(ham, seed=8, repetitions=13, replica_offset=1) as chains:
            trace = chains.advance_ladder(betas, 10, sweep_order="shuffled", trace=True)
            results.append((chains.state(), trace, _form(ham)))
    assert results[0][2][1] < 64 and results[1][2][1] == 64, "the first run was lane-packed, the second not"
    _same_state(results[0][0], results[1][0])
    assert np.array_equal(results[0][1], results[1][1])


# ---- the exchange law ----------------------------------------------------------------------------------

def _pairs(R, parity):
    return len(law.pairs(R, parity))


@pytest.mark.parametrize("R", [1, 2, 3, 64, 257])
@pytest.mark.parametrize("K", [40, 65, 300])
def test_exchange_law(K, R):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(K, seed=K + 1)
    lo, hi = max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6)
    ladder = sa.make_schedule(lo, hi, R)
    seed = 900 + R
    swapped = kept = 0
    with sa.Chains(ham, seed=seed, repetitions=R, replica_offset=2) as chains:
        for sweeps in (0, 16):
            if sweeps:
                chains.advance_ladder(ladder, sweeps, sweep_order="colour")
            for parity in (0, 1):
                for draw in (0, 7):
                    before = chains.state()
                    source, energies, accepted = chains.exchange(ladder, parity, draw)
                    assert source.dtype == np.uint32 and energies.dtype == np.float64
                    assert energies.tobytes() == ham.energies(before["x_current"]).tobytes()
                    want_source, want_accepted = law.exchange(energies, ladder, parity, seed, sweeps, draw)
                    assert np.array_equal(source, want_source) and accepted == want_accepted
                    after = chains.state()
                    _same_state(after, population_law.gathered(before, source))
                    assert int(after["sweeps_done"]) == sweeps
                    swapped += accepted
                    kept += _pairs(R, parity) - accepted
        if R == 1:
            assert swapped == 0 and kept == 0
        # all betas equal: every pair swaps
        before = chains.state()
        source, energies, accepted = chains.exchange(np.full(R, 0.3), 0, 0)
        assert accepted == _pairs(R, 0) and np.array_equal(source, law.exchange(energies, np.full(R, 0.3), 0, seed, 16, 0)[0])
        _same_state(chains.state(), population_law.gathered(before, source))
        # the next segment's trace starts from the energies that moved with the configurations
        trace = chains.advance_ladder(ladder, 1, sweep_order="shuffled", trace=True)
        assert np.array_equal(trace[:, 0], population_law.gathered(before, source)["tracked_current"])
    if R >= 64:
        assert swapped > 0 and kept > 0  # (a condition on the inputs: both outcomes were seen)


@pytest.mark.parametrize("R", [3, 64])
def test_a_huge_gap_against_an_energy_ordered_population_swaps_nothing(R):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, _ = _case(65, seed=2)
    with sa.Chains(ham, seed=31, repetitions=R) as chains:
        energies = ham.energies(chains.state()["x_current"])
        order = np.argsort(-energies, kind="stable")  # the colder the slot, the lower its energy
        chains.gather(order)
        ordered = energies[order]
        assert np.all(np.diff(ordered) < 0.0), "a condition on the inputs: no two chains share an energy"
        betas = 1e12 * np.arange(R, dtype=np.float64)  # every x_k >= 23 by far
        for parity in (0, 1):
            before = chains.state()
            source, got, accepted = chains.exchange(betas, parity, 3)
            assert got.tobytes() == ordered.tobytes()
            assert accepted == 0 and np.array_equal(source, np.arange(R))
            assert np.array_equal(source, law.exchange(got, betas, parity, 31, 0, 3)[0])
            _same_state(chains.state(), before)
        # ... and turned round every pair swaps: the colder slot holds the higher energy
        source, _, accepted = chains.exchange(betas[::-1].copy(), 0, 3)
        assert accepted == _pairs(R, 0)


# ---- validation ----------------------------------------------------------------------------------------

def test_invalid_arguments_return_before_any_launch():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    J, h, ham, info, _ = _case(65, seed=3)
    R = 4
    good = np.array([0.5, 0.0, 2.0, 1.0])
    u32 = ctypes.c_uint32
    with sa.Chains(ham, seed=1, repetitions=R) as chains:
        chains.advance_ladder(good, 3, sweep_order="colour")
        before = chains.state()
        handle = chains._live()
        trace = np.full((R, 4), 77, dtype=np.int64)
        source = np.full(R, 77, dtype=np.uint32)
        energy = np.full(R, -77.0)
        accepted = u32(12345)

        def ladder(betas, sweeps=3, order=0):
            return lib.asp_sa_chains_advance_ladder(handle, _lib.ptr(betas), u32(sweeps), u32(order), _lib.ptr(trace))

        def exchange(betas, parity=0):
            return lib.asp_sa_chains_exchange(handle, _lib.ptr(betas), u32(parity), u32(0), _lib.ptr(source),
                                              _lib.ptr(energy), ctypes.byref(accepted))

        bad = [np.array([0.5, -1.0, 2.0, 1.0]), np.array([0.5, np.nan, 2.0, 1.0]), np.array([0.5, 0.1, np.inf, 1.0])]
        for betas in bad:
            assert ladder(betas) == INVALID and "chain_betas" in _lib.last_error()
            assert exchange(betas) == INVALID and "chain_betas" in _lib.last_error()
        assert ladder(None) == INVALID and "null chain_betas" in _lib.last_error()
        assert exchange(None) == INVALID and "null chain_betas" in _lib.last_error()
        assert ladder(good, order=2) == INVALID and "order" in _lib.last_error()
        assert exchange(good, parity=2) == INVALID and "parity" in _lib.last_error()
        _same_state(chains.state(), before)
        assert np.all(trace == 77) and np.all(source == 77) and np.all(energy == -77.0) and accepted.value == 12345
        # a segment that would pass sweep index 2^32 - 2
        late = dict(before)
        late["sweeps_done"] = 2 ** 32 - 4
        chains.load_state(late)
        assert ladder(good, sweeps=3) == INVALID and "sweep indices" in _lib.last_error()
        assert np.all(trace == 77) and chains.sweeps_done == 2 ** 32 - 4
        assert ladder(good, sweeps=2) == 0 and chains.sweeps_done == 2 ** 32 - 2
        # NULL outputs are allowed: the step still runs
        state = chains.state()
        assert lib.asp_sa_chains_exchange(handle, _lib.ptr(np.full(R, 0.3)), u32(0), u32(0), None, None, None) == 0
        _same_state(chains.state(), population_law.gathered(state, [1, 0, 3, 2]))


# ---- the driver ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_parallel_tempering(order):
    from annealing_sign_problem_amd import annealer as sa

    rounds, per, R, seed = 6, 4, 8, 5
    J, h, _, info, _ = _case(300, seed=70)
    make = lambda: sa.Hamiltonian(J, h)
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, R)
    kw = dict(seed=seed, number_rounds=rounds, sweeps_per_round=per, repetitions=R, sweep_order=order)
    # without exchange: R independent constant-temperature chains — the closed calls (the ladder law)
    xs, es = sa.parallel_tempering(make(), only_best=False, exchange=False, **kw)
    ham = make()
    for k in range(R):
        cx, ce = sa.anneal_raw(ham, seed, np.full(rounds * per, ladder[k]), 1, k, shuffled=order == "shuffled")
        assert np.array_equal(xs[k], cx[0]) and es[k:k + 1].tobytes() == ce.tobytes()
    plain = (xs, es)
    # with it: the same rounds through the host — state(), the law in numpy, load_state()
    xs, es = sa.parallel_tempering(make(), only_best=False, **kw)
    ham = make()
    swapped = 0
    with sa.Chains(ham, seed=seed, repetitions=R) as chains:
        for j in range(rounds):
            chains.advance_ladder(ladder, per, sweep_order=order)
            if j + 1 < rounds:
                state = chains.state()
                energies = oracle.sa_energy(J, h, state["x_current"])
                source, accepted = law.exchange(energies, ladder, j & 1, seed, (j + 1) * per, 0)
                swapped += accepted
                chains.load_state(population_law.gathered(state, source))
        hxs, hes = chains.result()
    assert swapped > 0  # (a condition on the inputs: the exchange did something)
    assert np.array_equal(xs, hxs) and es.tobytes() == hes.tobytes()
    assert es.tobytes() == ham.energies(xs).tobytes()
    assert not (np.array_equal(xs, plain[0]) and es.tobytes() == plain[1].tobytes())
    x, e = sa.parallel_tempering(make(), **kw)
    best = int(np.argmin(es))
    assert np.array_equal(x, xs[best]) and np.float64(e).tobytes() == es[best].tobytes()


def test_parallel_tempering_reaches_the_planted_energy():
    """300 spins, the default ladder of 64 temperatures and the default order, 64 rounds of 10 sweeps."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, h, planted = synthetic.planted_cluster(300, seed=11)
    ham = sa.Hamiltonian(J, h)
    planted_energy = ham.energy(sa.signs_to_bits(planted))
    x, e = sa.parallel_tempering(ham, seed=1, number_rounds=64)
    assert e == ham.energy(x)
    assert e <= planted_energy + 1e-9 * abs(planted_energy)
