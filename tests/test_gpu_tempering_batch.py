"""Batched parallel tempering (asp_sa_chains_advance_ladder_batch / _exchange_batch, annealer
.advance_ladder_chains / .exchange_chains / .parallel_tempering_batch, common.solve_ising_models(method=...);
DESIGN.md §4.12 "Batched forms").

Every comparison is exact: np.array_equal on words and integers, energies compared as bytes.  The
reference for a batch is a set of twin handles advanced one at a time with the single calls; for the
exchange law also tests/tempering_law.py, Hamiltonian.energies and numpy indexing of the exported state
(tests/population_law.gathered); for the small plans the CPU oracle (oracle.sa_anneal,
oracle.sa_anneal_shuffled) on the constant per-chain schedule.  Problems come from
synthetic.planted_cluster with a small random field, as in tests/test_gpu_tempering.py.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import oracle
import population_law
import tempering_law as law

pytestmark = pytest.mark.gpu

INVALID = -3
ORDERS = {0: "colour", 1: "shuffled"}
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")
u32 = ctypes.c_uint32


def _problem(n, seed):
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(n, seed=seed)
    h = np.random.default_rng(seed).normal(size=n) * 0.01
    return J, h


def _case(n, seed):
    from annealing_sign_problem_amd import annealer as sa

    J, h = _problem(n, seed)
    ham = sa.Hamiltonian(J, h)
    return J, h, ham, ham.info()


def _random_x0(n, seed, rows=None):
    from annealing_sign_problem_amd import annealer as sa

    rng = np.random.default_rng(seed)
    if rows is None:
        return sa.signs_to_bits(np.where(rng.random(n) < 0.5, 1.0, -1.0))
    return np.stack([sa.signs_to_bits(np.where(rng.random(n) < 0.5, 1.0, -1.0)) for _ in range(rows)])


def _range(info):
    return max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6)


def _chain_betas(info, R):
    """R distinct, unsorted inverse temperatures around the plan's automatic range, among them (from
    three chains on) a 0 and one that freezes every proposal with dE > 0 (tests/test_gpu_tempering.py)."""
    lo, hi = _range(info)
    pool = list(np.geomspace(lo, hi, 13))
    pool = [pool[k] for k in (6, 12, 0, 9, 3, 11, 1, 7, 4, 10, 2, 8, 5)]
    pool[1], pool[2] = 0.0, 1e9
    return np.array(pool[:R], dtype=np.float64)


def _many_betas(info, R, seed):
    """R distinct inverse temperatures of the automatic range in a shuffled order."""
    lo, hi = _range(info)
    return np.random.default_rng(seed).permutation(np.geomspace(lo, hi, R))


def _same_state(a, b):
    sa_, sb = a.state(), b.state()
    for name in STATE:
        assert np.array_equal(sa_[name], sb[name]), name
    assert int(sa_["sweeps_done"]) == int(sb["sweeps_done"])


def _same_dict(a, b):
    for name in STATE:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name])), name
    assert int(a["sweeps_done"]) == int(b["sweeps_done"])


def _launch(ham):
    from annealing_sign_problem_amd import _lib

    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return m.value, threads.value


# ---- 1. the batch is the singles -----------------------------------------------------------------------
SIZES = (40, 65, 130, 700, 3000)
REPS = (3, 5, 8, 1, 6)
OFFSETS = (0, 7, 0, 3, 1)
SEEDS = (101, 202, 303, 404, 505)
SPLIT = (0, 1, 7, 16)


def _starts():
    return [_random_x0(SIZES[0], 1), _random_x0(SIZES[1], 2, rows=REPS[1]), None, None, None]


@pytest.mark.parametrize("order", [0, 1])
def test_batched_ladder_segments_are_the_single_segments(order):
    from annealing_sign_problem_amd import annealer as sa

    name = ORDERS[order]
    cases_a = [_case(n, 50 + k) for k, n in enumerate(SIZES)]
    cases_b = [_case(n, 50 + k) for k, n in enumerate(SIZES)]
    starts = _starts()
    make = lambda cases: [sa.Chains(c[2], seed=SEEDS[k], repetitions=REPS[k], x0=starts[k], replica_offset=OFFSETS[k])
                          for k, c in enumerate(cases)]
    set_a, set_b = make(cases_a), make(cases_b)
    ladders = [_chain_betas(c[3], REPS[k]) for k, c in enumerate(cases_a)]
    done = 0
    for n in SPLIT:
        before = [c.state()["tracked_best"] for c in set_a]
        told = sa.advance_ladder_chains(set_a, ladders, n, sweep_order=name, progress=True)
        for k, c in enumerate(set_b):
            c.advance_ladder(ladders[k], n, sweep_order=name)
        done += n
        for k in range(len(SIZES)):
            _same_state(set_a[k], set_b[k])
            assert set_a[k].sweeps_done == done
            after = set_a[k].state()["tracked_best"]
            best, improved = told[k]
            assert best.dtype == np.int64 and np.array_equal(best, after)
            assert improved == int(np.sum(after < before[k]))
            if n == 0:
                assert improved == 0
    # every chain of the small plans against the CPU oracle on its constant schedule
    run = oracle.sa_anneal_shuffled if order == 1 else oracle.sa_anneal
    for k in range(3):
        J, h, _, info = cases_a[k]
        xs, es = set_a[k].result()
        state = set_a[k].state()
        for r in range(REPS[k]):
            x0 = starts[k]
            start = None if x0 is None else (x0 if x0.ndim == 1 else x0[r])
            ox, oe, otracked, oaccepted = run(J, h, SEEDS[k], np.full(done, ladders[k][r]), 1, OFFSETS[k] + r, start,
                                              info.energy_scale_exp)
            assert np.array_equal(xs[r], ox[0]) and es[r:r + 1].tobytes() == oe.tobytes()
            assert state["tracked_best"][r] == otracked[0] and state["accepted"][r] == oaccepted[0]
    for c in set_a + set_b:
        c.close()


LARGE_REPS, LARGE_SWEEPS = 5, 5
_LARGE = {}


def _large_chains(ham, j):
    from annealing_sign_problem_amd import annealer as sa

    return sa.Chains(ham, seed=4321 + j, repetitions=LARGE_REPS, replica_offset=2 + j)


def _large(k):
    """Two plans of the cluster of tests/test_gpu_sa_trace_shuffled.py::test_trace_in_the_layouts_of_large_clusters
    (mean degree 6), a ladder, and the state of five chains per plan after the single-handle ladder segment:
    the reference, built once per size."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    if k not in _LARGE:
        J, h, _ = synthetic.planted_cluster(k, seed=5, mean_degree=6.0)
        hams = [sa.Hamiltonian(J, h) for _ in range(2)]
        ladder = _chain_betas(hams[0].info(), LARGE_REPS)
        want = []
        for j, ham in enumerate(hams):
            with _large_chains(ham, j) as single:
                single.advance_ladder(ladder, LARGE_SWEEPS, sweep_order="shuffled")
                want.append(single.state())
        _LARGE[k] = hams, ladder, want
    return _LARGE[k]


@pytest.mark.parametrize("k,forced_m,expect_m", [(170000, 4, 4), (170000, 0, 1), (300000, 0, 1)])
def test_batched_ladder_segments_in_the_layouts_of_large_clusters(k, forced_m, expect_m):
    """The batched ladder kernels in four bits (four chains per group, the last group ragged, and one chain)
    and one bit per spin — the layout is whatever fits the LDS —: two handles in one call are their
    single-handle ladder segments."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    hams, ladder, want = _large(k)
    for ham in hams:
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), forced_m, 0))
    chains = [_large_chains(ham, j) for j, ham in enumerate(hams)]
    try:
        sa.advance_ladder_chains(chains, [ladder, ladder], LARGE_SWEEPS, sweep_order="shuffled")
        for j, c in enumerate(chains):
            assert _launch(hams[j])[0] == expect_m
            _same_dict(c.state(), want[j])
    finally:
        for c in chains:
            c.close()
        for ham in hams:
            _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), 0, 0))


# ---- 2. mixed call -------------------------------------------------------------------------------------

def _raw_chains(ham, seed, repetitions):
    """A handle through the C ABI: annealer.Chains refuses repetitions = 0."""
    from annealing_sign_problem_amd import _lib

    handle = ctypes.c_void_p()
    _lib.check(_lib.load().asp_sa_chains_create(ham.plan(), ctypes.c_uint64(seed), u32(repetitions), u32(0), None,
                                                ctypes.c_uint64(0), ctypes.byref(handle)))
    return handle


def _raw_sweeps_done(handle):
    from annealing_sign_problem_amd import _lib

    snap = _lib.SaChainsSnapshot()
    _lib.check(_lib.load().asp_sa_chains_export(handle, ctypes.byref(snap)))
    return int(snap.sweeps_done)


def test_mixed_call():
    """Both orders, three lengths (two of them shared by several shuffled items, one alone), handles at
    different sweeps_done, a traced item, a handle without chains, a plan without spins and a plan with
    a forced launch in ONE batch, against handles advanced one at a time.

      shuffled, 9 sweeps: items 1, 8, 9 at sweeps_done 4, 2, 0 share launches; item 4 is traced: alone;
      shuffled, 5 sweeps: items 3, 6 at 0, 1;
      shuffled, 3 sweeps: item 10, the only one of its length: alone;
      colour: items 0, 5, 7 at 0, 3, 6 share launches; item 2 has a forced launch: alone;
      item 11: no chains; item 12: no spins."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    sizes = (40, 65, 130, 700, 130, 40, 65, 700, 130, 300, 65)
    orders = (0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1)
    lengths = (5, 9, 9, 5, 9, 5, 5, 9, 9, 9, 3)
    first = (0, 4, 0, 0, 0, 3, 1, 6, 2, 0, 0)  # sweeps every handle has run, alone, before the batch
    traced, forced = 4, 2
    n = len(sizes)
    reps = [3 + k % 4 for k in range(n)]
    sets = []
    for _ in range(2):
        cases = [_case(size, 70 + k) for k, size in enumerate(sizes)]
        _lib.check(lib.asp_sa_set_launch(cases[forced][2].plan(), 2, 0))
        chains = [sa.Chains(c[2], seed=900 + k, repetitions=reps[k], replica_offset=k) for k, c in enumerate(cases)]
        ladders = [_chain_betas(c[3], reps[k]) for k, c in enumerate(cases)]
        for k, c in enumerate(chains):
            if first[k]:
                c.advance_ladder(ladders[k][::-1].copy(), first[k], sweep_order=ORDERS[orders[k]])
        spare = _case(65, 7)[2]  # (kept alive: the handle below belongs to its plan)
        without_chains = _raw_chains(spare, 5, 0)
        no_spins = sa.Hamiltonian(scipy.sparse.csr_matrix((0, 0)), np.zeros(0))
        without_spins = sa.Chains(no_spins, seed=6, repetitions=3)
        sets.append((cases, chains, ladders, without_chains, without_spins, spare))
    (cases_a, set_a, ladders, none_a, empty_a, _), (cases_b, set_b, _, none_b, empty_b, _) = sets
    total = n + 2
    items = (_lib.SaChainsLadderItem * total)()
    rows = np.full((set_a[traced].repetitions, lengths[traced] + 1), -1, dtype=np.int64)
    empty_rows = np.full((3, 5), -1, dtype=np.int64)
    empty_betas = np.array([0.5, 0.0, 2.0])
    for k, c in enumerate(set_a):
        items[k].chains = c._live()
        items[k].chain_betas = ladders[k].ctypes.data
        items[k].num_sweeps = lengths[k]
        items[k].order = orders[k]
        if k == traced:
            items[k].out_trace = rows.ctypes.data
    items[n].chains = none_a
    items[n].num_sweeps = 4
    items[n].order = 1
    items[n + 1].chains = empty_a._live()
    items[n + 1].chain_betas = empty_betas.ctypes.data
    items[n + 1].num_sweeps = 4
    items[n + 1].order = 0
    items[n + 1].out_trace = empty_rows.ctypes.data
    _lib.check(lib.asp_sa_chains_advance_ladder_batch(items, u32(total)))
    assert lib.asp_sa_chains_batch_last_ms() > 0.0
    assert _launch(cases_a[forced][2])[0] == 2, "the forced group size was honoured"
    for k, c in enumerate(set_b):
        part = c.advance_ladder(ladders[k], lengths[k], sweep_order=ORDERS[orders[k]], trace=k == traced)
        if k == traced:
            assert np.array_equal(part, rows)
        _same_state(set_a[k], c)
        assert set_a[k].sweeps_done == first[k] + lengths[k]
    _lib.check(lib.asp_sa_chains_advance_ladder(none_b, None, u32(4), u32(1), None))
    assert _raw_sweeps_done(none_a) == _raw_sweeps_done(none_b) == 4
    single_rows = empty_b.advance_ladder(empty_betas, 4, sweep_order="colour", trace=True)
    assert np.array_equal(empty_rows, single_rows) and np.all(empty_rows == 0)
    _same_state(empty_a, empty_b)
    assert empty_a.sweeps_done == 4
    for handle in (none_a, none_b):
        lib.asp_sa_chains_destroy(handle)
    for c in set_a + set_b + [empty_a, empty_b]:
        c.close()


# ---- 3. chains per group -------------------------------------------------------------------------------

@pytest.mark.parametrize("per_group", [4, 2])
@pytest.mark.parametrize("order", [0, 1])
def test_chains_per_group(order, per_group):
    """The construction of tests/test_gpu_chains_batch.py::test_chains_per_group — enough chains in the
    batch that the launcher packs four, or exactly two, per workgroup, with a repetition count that is no
    multiple of it — with a beta of its own for every chain: the padded chain's beta slot and the
    (handle, group) -> chain indexing of the concatenated betas are what can go wrong here."""
    import torch

    from annealing_sign_problem_amd import annealer as sa

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [_case(40, 30 + k) for k in range(8)]
    if order == 1:
        need, waves = 2 * cus, [1] * 8
    else:
        probe = [_case(40, 30 + k) for k in range(8)]
        with_one = [sa.Chains(c[2], seed=1, repetitions=1) for c in probe]
        sa.advance_ladder_chains(with_one, [[0.5]] * 8, 1, sweep_order="colour")
        need, waves = 4 * cus, [_launch(c[2])[1] // 64 for c in probe]
        for c in with_one:
            c.close()
        assert all(1 <= w <= 16 for w in waves)
    if per_group == 4:
        reps = (16 * cus + 7) // 8 + 1  # 16 x CUs chains in all, and one more per handle: odd
    else:
        reps = 2 * (-(-need // sum(waves))) - 1  # the fewest pairs that reach `need`, less one chain: odd
    total = lambda m: sum(-(-reps // m) * w for w in waves)
    assert reps % per_group != 0 and total(per_group) >= need and (per_group == 4 or total(4) < need)
    ladders = [_many_betas(c[3], reps, 11 + k) for k, c in enumerate(cases)]
    chains = [sa.Chains(c[2], seed=40 + k, repetitions=reps) for k, c in enumerate(cases)]
    sa.advance_ladder_chains(chains, ladders, 6, sweep_order=ORDERS[order])
    for c in cases:
        assert _launch(c[2])[0] == per_group
    for k in (0, 5):
        other = _case(40, 30 + k)
        with sa.Chains(other[2], seed=40 + k, repetitions=reps) as single:
            single.advance_ladder(ladders[k], 6, sweep_order=ORDERS[order])
            _same_state(chains[k], single)
    for c in chains:
        c.close()


# ---- 4. equal betas ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
def test_equal_betas_are_advance_chains_bit_for_bit(order):
    from annealing_sign_problem_amd import annealer as sa

    sizes, reps = (40, 130, 700), (4, 6, 3)
    sets = []
    for _ in range(2):
        cases = [_case(n, 80 + k) for k, n in enumerate(sizes)]
        sets.append((cases, [sa.Chains(c[2], seed=60 + k, repetitions=reps[k], replica_offset=2 * k,
                                       x0=_random_x0(sizes[k], k, reps[k])) for k, c in enumerate(cases)]))
    (cases, ladder), (_, plain) = sets
    betas = [float(np.sqrt(_range(c[3])[0] * _range(c[3])[1])) for c in cases]
    told = sa.advance_ladder_chains(ladder, [np.full(reps[k], betas[k]) for k in range(3)], 9,
                                    sweep_order=ORDERS[order], progress=True)
    want = sa.advance_chains(plain, [np.full(9, betas[k]) for k in range(3)], sweep_order=ORDERS[order], progress=True)
    for k in range(3):
        _same_state(ladder[k], plain[k])
        assert np.array_equal(told[k][0], want[k][0]) and told[k][1] == want[k][1]
    for c in ladder + plain:
        c.close()


# ---- 5. the exchange batch -----------------------------------------------------------------------------
EX_REPS = (1, 2, 3, 13, 257)  # 257 crosses the 256-thread workgroup of the selection kernel
EX_SIZES = (40, 65, 130, 300, 65)
EX_SWEEPS = (2, 5, 3, 0, 4)


def _exchange_sets():
    from annealing_sign_problem_amd import annealer as sa

    sets = []
    for _ in range(2):
        cases = [_case(n, 20 + k) for k, n in enumerate(EX_SIZES)]
        chains = [sa.Chains(c[2], seed=700 + k, repetitions=EX_REPS[k], replica_offset=k) for k, c in enumerate(cases)]
        ladders = [sa.make_schedule(*_range(c[3]), EX_REPS[k]) for k, c in enumerate(cases)]
        for k, c in enumerate(chains):
            c.advance_ladder(ladders[k], EX_SWEEPS[k], sweep_order="colour")
        sets.append((cases, chains, ladders))
    return sets


def test_exchange_batch():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    (cases, set_a, ladders), (_, set_b, _) = _exchange_sets()
    n = len(EX_REPS)
    swapped = kept = 0
    for step, (picked, parities, draws) in enumerate([
            (list(range(n)), [0, 0, 1, 0, 1], [0, 3, 7, 11, 2]),       # the whole batch
            (list(range(n))[::-1], [1, 1, 0, 1, 0], [5, 0, 1, 9, 4]),  # its items in reversed order
            ([3], [0], [6]),                                           # a batch of one
            ([4, 0, 2], 1, 8)]):                                       # one parity and one draw for all
        before = {k: set_a[k].state() for k in picked}
        got = sa.exchange_chains([set_a[k] for k in picked], [ladders[k] for k in picked], parities, draws)
        assert _lib.load().asp_sa_chains_exchange_last_ms() > 0.0
        for at, k in enumerate(picked):
            parity = parities if np.ndim(parities) == 0 else parities[at]
            draw = draws if np.ndim(draws) == 0 else draws[at]
            source, energies, accepted = got[at]
            want = set_b[k].exchange(ladders[k], parity, draw)
            assert source.dtype == np.uint32 and np.array_equal(source, want[0])
            assert energies.tobytes() == want[1].tobytes() and accepted == want[2]
            _same_state(set_a[k], set_b[k])
            # ... and the law restated, on the energies of the exported state
            assert energies.tobytes() == cases[k][2].energies(before[k]["x_current"]).tobytes()
            law_source, law_accepted = law.exchange(energies, ladders[k], parity, 700 + k, EX_SWEEPS[k], draw)
            assert np.array_equal(source, law_source) and accepted == law_accepted
            _same_dict(set_a[k].state(), population_law.gathered(before[k], source))
            swapped += accepted
            kept += len(law.pairs(EX_REPS[k], parity)) - accepted
    assert swapped > 0 and kept > 0  # (a condition on the inputs: both outcomes were seen)
    for c in set_a + set_b:
        c.close()


# ---- 6. alternation ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
def test_alternation_with_the_other_calls(order):
    """ladder batch, plain batch, exchange batch, resample batch, export -> import into fresh handles,
    ladder batch — against the same sequence of single calls."""
    from annealing_sign_problem_amd import annealer as sa

    name = ORDERS[order]
    sizes, reps = (40, 130, 700), (4, 7, 3)
    sets = []
    for _ in range(2):
        cases = [_case(n, 90 + k) for k, n in enumerate(sizes)]
        sets.append((cases, [sa.Chains(c[2], seed=31 + k, repetitions=reps[k], replica_offset=k)
                             for k, c in enumerate(cases)]))
    (cases, batch), (_, single) = sets
    ladders = [sa.make_schedule(*_range(c[3]), reps[k]) for k, c in enumerate(cases)]
    plain = [sa.make_schedule(*_range(c[3]), 5) for c in cases]

    def fresh(chains, these_cases):
        states = [c.state() for c in chains]
        for c in chains:
            c.close()
        out = [sa.Chains(c[2], seed=31 + k, repetitions=reps[k], replica_offset=k) for k, c in enumerate(these_cases)]
        for c, state in zip(out, states):
            c.load_state(state)
        return out

    sa.advance_ladder_chains(batch, ladders, 6, sweep_order=name)
    sa.advance_chains(batch, plain, sweep_order=name)
    sa.exchange_chains(batch, ladders, 1, 3)
    sa.resample_chains(batch, [0.25, 0.5, 0.125], 2)
    batch = fresh(batch, cases)
    sa.advance_ladder_chains(batch, ladders, [4, 4, 7], sweep_order=name)
    for k, c in enumerate(single):
        c.advance_ladder(ladders[k], 6, sweep_order=name)
        c.advance(plain[k], sweep_order=name)
        c.exchange(ladders[k], 1, 3)
        c.resample((0.25, 0.5, 0.125)[k], 2)
    single = fresh(single, sets[1][0])
    for k, c in enumerate(single):
        c.advance_ladder(ladders[k], (4, 4, 7)[k], sweep_order=name)
        _same_state(batch[k], c)
        assert c.sweeps_done == 11 + (4, 4, 7)[k]
    for c in batch + single:
        c.close()


# ---- 7. the drivers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_parallel_tempering_batch(order):
    from annealing_sign_problem_amd import annealer as sa

    sizes = (40, 300, 700)
    problems = [_problem(n, 60 + k) for k, n in enumerate(sizes)]
    make = lambda: [sa.Hamiltonian(J, h) for J, h in problems]
    kw = dict(seed=5, number_rounds=6, sweeps_per_round=3, repetitions=5, sweep_order=order)
    got = sa.parallel_tempering_batch(make(), only_best=False, **kw)
    for (xs, es), ham in zip(got, make()):
        sxs, ses = sa.parallel_tempering(ham, only_best=False, **kw)
        assert np.array_equal(xs, sxs) and es.tobytes() == ses.tobytes()
    best = sa.parallel_tempering_batch(make(), **kw)
    for (x, e), (xs, es) in zip(best, got):
        at = int(np.argmin(es))
        assert np.array_equal(x, xs[at]) and np.float64(e).tobytes() == es[at].tobytes()
    # per-problem seeds
    seeded = sa.parallel_tempering_batch(make(), only_best=False, **dict(kw, seed=[5, 6, 7]))
    assert np.array_equal(seeded[0][0], got[0][0])
    sxs, ses = sa.parallel_tempering(make()[2], only_best=False, **dict(kw, seed=7))
    assert np.array_equal(seeded[2][0], sxs) and seeded[2][1].tobytes() == ses.tobytes()
    # without exchange: independent constant-temperature chains — the closed calls
    free = sa.parallel_tempering_batch(make(), only_best=False, exchange=False, **kw)
    for (xs, es), ham in zip(free, make()):
        info = ham.info()
        ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, 5)
        for k in range(5):
            cx, ce = sa.anneal_raw(ham, 5, np.full(18, ladder[k]), 1, k, shuffled=order == "shuffled")
            assert np.array_equal(xs[k], cx[0]) and es[k:k + 1].tobytes() == ce.tobytes()
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(got, free))  # (the exchange did something)


def test_solve_ising_models_methods():
    """method="tempering" / "population" equal the direct batch calls followed by the projection on the
    frozen spins, with number_sweeps // 10 rounds / steps of ten sweeps."""
    from annealing_sign_problem_amd import annealer as sa, common

    rng = np.random.default_rng(5)
    problems = [_problem(n, 40 + k) for k, n in enumerate((40, 65, 130))]

    def models():
        return [common.IsingModel(np.arange(J.shape[0], dtype=np.uint64) * 3 + 1, None, sa.Hamiltonian(J, h), None)
                for J, h in problems]

    frozen = []
    for J, _ in problems:
        n = J.shape[0]
        keep = np.sort(rng.choice(n, size=max(1, n // 3), replace=False))
        frozen.append((keep * 3 + 1).astype(np.uint64))
    frozen[0] = None
    kw = dict(seed=9, repetitions=4, sweep_order="shuffled")
    for method, direct in (("tempering", lambda hams: sa.parallel_tempering_batch(
                                hams, number_rounds=3, sweeps_per_round=10, only_best=True, **kw)),
                           ("population", lambda hams: sa.population_anneal_batch(
                                hams, number_steps=3, sweeps_per_step=10, only_best=True, **kw))):
        got = common.solve_ising_models(models(), frozen, number_sweeps=35, method=method, **kw)
        want = direct([m.ising_hamiltonian for m in models()])
        assert len(got) == len(want) == 3
        for model, x, (wx, _), f in zip(models(), got, want, frozen):
            assert np.array_equal(x, common._project_on_frozen(model, wx, f))
    plain = common.solve_ising_models(models(), frozen, number_sweeps=35, **kw)
    again = common.solve_ising_models(models(), frozen, number_sweeps=35, method="anneal", **kw)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))


# ---- 8. errors change nothing --------------------------------------------------------------------------

def test_errors_change_nothing():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    cases = [_case(n, 10 + k) for k, n in enumerate((40, 65, 130))]
    reps = (4, 3, 4)
    chains = [sa.Chains(c[2], seed=3 + k, repetitions=reps[k]) for k, c in enumerate(cases)]
    twin = sa.Chains(cases[0][2], seed=9, repetitions=4)  # a second handle of plan 0
    good = [np.array([0.5, 0.0, 2.0, 1.0][:r]) for r in reps]
    sa.advance_ladder_chains(chains, good, 3, sweep_order="colour")
    before = [c.state() for c in chains]
    traces = [np.full((r, 4), 77, dtype=np.int64) for r in reps]
    bests = [np.full(r, 77, dtype=np.int64) for r in reps]
    improved = [u32(12345) for _ in reps]
    sources = [np.full(r, 77, dtype=np.uint32) for r in reps]
    energies = [np.full(r, -77.0) for r in reps]
    accepted = [u32(12345) for _ in reps]

    def ladder_items():
        items = (_lib.SaChainsLadderItem * 3)()
        for k, c in enumerate(chains):
            items[k].chains = c._live()
            items[k].chain_betas = good[k].ctypes.data
            items[k].num_sweeps = 3
            items[k].order = k % 2
            items[k].out_trace = traces[k].ctypes.data
            items[k].out_tracked_best = bests[k].ctypes.data
            items[k].out_improved = ctypes.addressof(improved[k])
        return items

    def exchange_items():
        items = (_lib.SaChainsExchangeItem * 3)()
        for k, c in enumerate(chains):
            items[k].chains = c._live()
            items[k].chain_betas = good[k].ctypes.data
            items[k].parity = k % 2
            items[k].draw = k
            items[k].out_source = sources[k].ctypes.data
            items[k].out_energy = energies[k].ctypes.data
            items[k].out_accepted = ctypes.addressof(accepted[k])
        return items

    def untouched():
        for k, c in enumerate(chains):
            _same_dict(c.state(), before[k])
            assert np.all(traces[k] == 77) and np.all(bests[k] == 77) and improved[k].value == 12345
            assert np.all(sources[k] == 77) and np.all(energies[k] == -77.0) and accepted[k].value == 12345

    def attempt(make, call, change, *words):
        items = make()
        keep = change(items[2])  # (the error sits at the LAST item; `keep` holds its arrays alive)
        assert call(items, u32(3)) == INVALID
        assert lib.asp_last_error_code() == INVALID
        message = _lib.last_error()
        for word in words:
            assert word in message, (word, message)
        untouched()
        return keep

    def set_betas(values):
        def change(item):
            array = np.array(values, dtype=np.float64)
            item.chain_betas = array.ctypes.data
            return array
        return change

    def set_field(name, value):
        def change(item):
            setattr(item, name, value)
        return change

    for make, call in ((ladder_items, lib.asp_sa_chains_advance_ladder_batch),
                       (exchange_items, lib.asp_sa_chains_exchange_batch)):
        attempt(make, call, set_field("chains", None), "item 2", "null chains handle")
        attempt(make, call, set_field("chain_betas", None), "item 2", "null chain_betas")
        for bad in ([0.5, -1.0, 2.0, 1.0], [0.5, np.nan, 2.0, 1.0], [0.5, 0.1, np.inf, 1.0]):
            attempt(make, call, set_betas(bad), "item 2", "chain_betas[")
        attempt(make, call, set_field("flags", 1), "item 2", "flags")
        attempt(make, call, set_field("chains", chains[1]._live()), "items 1 and 2", "same handle")
        attempt(make, call, set_field("chains", twin._live()), "items 0 and 2", "one plan")
    attempt(ladder_items, lib.asp_sa_chains_advance_ladder_batch, set_field("order", 2), "item 2", "order")
    attempt(exchange_items, lib.asp_sa_chains_exchange_batch, set_field("parity", 2), "item 2", "parity")
    # a segment that would pass sweep index 2^32 - 2, at the last item
    late = dict(before[2])
    late["sweeps_done"] = 2 ** 32 - 4
    chains[2].load_state(late)
    before[2] = chains[2].state()
    attempt(ladder_items, lib.asp_sa_chains_advance_ladder_batch, set_field("num_sweeps", 3), "item 2", "sweep indices")
    # ... and the same batches are fine afterwards
    items = ladder_items()
    items[2].num_sweeps = 2
    items[2].out_trace = None
    _lib.check(lib.asp_sa_chains_advance_ladder_batch(items, u32(3)))
    assert chains[2].sweeps_done == 2 ** 32 - 2 and chains[0].sweeps_done == 6
    _lib.check(lib.asp_sa_chains_exchange_batch(exchange_items(), u32(3)))
    assert all(np.array_equal(np.sort(s), np.arange(r)) for s, r in zip(sources, reps))
    for c in chains + [twin]:
        c.close()
