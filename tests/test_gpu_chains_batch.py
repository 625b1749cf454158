"""Batched segments of resumable chains (asp_sa_chains_advance_batch, annealer.advance_chains,
anneal_batch_until).

Every comparison is exact: np.array_equal on words and integers, energies compared as bytes.  The law
— a batched segment is the single segment of every handle — is checked against handles advanced one at
a time, against the closed calls, and for the small plans against the CPU oracle (oracle.sa_anneal,
oracle.sa_anneal_shuffled), so that it is not the code against itself.  Problems come from
synthetic.planted_cluster with a small random field, as in tests/test_gpu_chains.py.
"""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

INVALID = -3
ORDERS = {0: "colour", 1: "shuffled"}
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def _problem(n, seed):
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(n, seed=seed)
    h = np.random.default_rng(seed).normal(size=n) * 0.01
    return J, h


def _case(n, sweeps, seed):
    from annealing_sign_problem_amd import annealer as sa

    J, h = _problem(n, seed)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = sa.make_schedule(max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6), sweeps)
    return J, h, ham, info, betas


def _random_x0(n, seed, rows=None):
    from annealing_sign_problem_amd import annealer as sa

    rng = np.random.default_rng(seed)
    if rows is None:
        return sa.signs_to_bits(np.where(rng.random(n) < 0.5, 1.0, -1.0))
    return np.stack([sa.signs_to_bits(np.where(rng.random(n) < 0.5, 1.0, -1.0)) for _ in range(rows)])


def _same_state(a, b):
    sa_, sb = a.state(), b.state()
    for name in STATE:
        assert np.array_equal(sa_[name], sb[name]), name
    assert int(sa_["sweeps_done"]) == int(sb["sweeps_done"])


def _launch(ham):
    from annealing_sign_problem_amd import _lib

    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return m.value, threads.value


SIZES = (40, 65, 130, 700, 3000)
REPS = (3, 5, 8, 1, 6)  # (23 chains never fill a chip: one chain per group here; test_chains_per_group pads)
OFFSETS = (0, 7, 0, 3, 1)
SEEDS = (101, 202, 303, 404, 505)
SPLIT = (0, 1, 7, 16)


def _starts():
    return [_random_x0(SIZES[0], 1), _random_x0(SIZES[1], 2, rows=REPS[1]), None, None, None]


@pytest.mark.parametrize("order", [0, 1])
def test_batched_segments_are_the_single_segments(order):
    from annealing_sign_problem_amd import annealer as sa

    sweeps = sum(SPLIT)
    cases_a = [_case(n, sweeps, 50 + k) for k, n in enumerate(SIZES)]
    cases_b = [_case(n, sweeps, 50 + k) for k, n in enumerate(SIZES)]
    starts = _starts()
    make = lambda cases: [sa.Chains(c[2], seed=SEEDS[k], repetitions=REPS[k], x0=starts[k], replica_offset=OFFSETS[k])
                          for k, c in enumerate(cases)]
    set_a, set_b = make(cases_a), make(cases_b)
    done = 0
    for n in SPLIT:
        before = [c.state()["tracked_best"] for c in set_a]
        told = sa.advance_chains(set_a, [c[4][done:done + n] for c in cases_a], sweep_order=ORDERS[order],
                                 progress=True)
        for k, c in enumerate(set_b):
            c.advance(cases_b[k][4][done:done + n], sweep_order=ORDERS[order])
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
    for k, n in enumerate(SIZES):
        xs, es = set_a[k].result()
        J, h, _, info, betas = _case(n, sweeps, 50 + k)[:5]
        third = _case(n, sweeps, 50 + k)[2]
        x0 = starts[k]
        if x0 is None or x0.ndim == 1:
            cxs, ces = sa.anneal_raw(third, SEEDS[k], betas, REPS[k], OFFSETS[k], x0, shuffled=order == 1)
        else:  # (per-chain starts: chain r is the closed call of one chain at replica offset + r)
            parts = [sa.anneal_raw(third, SEEDS[k], betas, 1, OFFSETS[k] + r, x0[r], shuffled=order == 1)
                     for r in range(REPS[k])]
            cxs, ces = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        assert np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes()
        if k < 3:
            fn = oracle.sa_anneal_shuffled if order == 1 else oracle.sa_anneal
            if x0 is None or x0.ndim == 1:
                oxs, oes, _, _ = fn(J, h, SEEDS[k], betas, REPS[k], OFFSETS[k], x0, info.energy_scale_exp, num_threads=8)
            else:
                parts = [fn(J, h, SEEDS[k], betas, 1, OFFSETS[k] + r, x0[r], info.energy_scale_exp) for r in range(REPS[k])]
                oxs, oes = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            assert np.array_equal(oxs, xs) and oes.tobytes() == es.tobytes()
    for c in set_a + set_b:
        c.close()


def test_mixed_call():
    """Different orders, lengths and sweeps_done, a traced item, a forced layout and a forced shuffled
    geometry in ONE batch, against handles advanced one at a time and against the closed calls.

    Handles at DIFFERENT sweeps_done share launches in both orders — what separates a batched segment
    from the closed batch, whose problems all start at sweep 0:
      shuffled, 9 sweeps: items 1, 8, 9 (untraced, geometry not forced) at sweeps_done 4, 2, 0;
      shuffled, 5 sweeps: items 3 (forced geometry), 6 at 0, 1;
      colour: items 0, 5, 7 at 0, 3, 6 (0 and 5 have one size: one launch class).
    Item 4 is traced and item 2 has a forced layout: both run alone inside the call."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    sizes = (40, 65, 130, 700, 130, 40, 65, 700, 130, 300)
    orders = (0, 1, 0, 1, 1, 0, 1, 0, 1, 1)
    lengths = (5, 9, 9, 5, 9, 5, 5, 9, 9, 9)
    first = (0, 4, 0, 0, 0, 3, 1, 6, 2, 0)  # sweeps every handle has run, alone, before the batch
    traced = 4
    n = len(sizes)
    reps = [3 + k % 4 for k in range(n)]
    sets = []
    for _ in range(2):
        cases = [_case(size, 16, 70 + k) for k, size in enumerate(sizes)]
        _lib.check(lib.asp_sa_set_packed(cases[2][2].plan(), 1))
        _lib.check(lib.asp_sa_set_shuffled_launch(cases[3][2].plan(), 2, 1))
        chains = [sa.Chains(c[2], seed=900 + k, repetitions=reps[k], replica_offset=k) for k, c in enumerate(cases)]
        for k, c in enumerate(chains):
            if first[k]:
                c.advance(cases[k][4][:first[k]], sweep_order=ORDERS[orders[k]])
        sets.append((cases, chains))
    (cases_a, set_a), (cases_b, set_b) = sets
    # the batch, with item `traced` traced through the C ABI
    items = (_lib.SaChainsItem * n)()
    keep = []
    rows = np.full((set_a[traced].repetitions, lengths[traced] + 1), -1, dtype=np.int64)
    for k, c in enumerate(set_a):
        betas = np.ascontiguousarray(cases_a[k][4][first[k]:first[k] + lengths[k]])
        keep.append(betas)
        items[k].chains = c._live()
        items[k].betas = betas.ctypes.data
        items[k].num_sweeps = lengths[k]
        items[k].order = orders[k]
        if k == traced:
            items[k].out_trace = rows.ctypes.data
    _lib.check(lib.asp_sa_chains_advance_batch(items, ctypes.c_uint32(n)))
    assert lib.asp_sa_chains_batch_last_ms() > 0.0
    for k, c in enumerate(set_b):
        part = c.advance(cases_b[k][4][first[k]:first[k] + lengths[k]], sweep_order=ORDERS[orders[k]], trace=k == traced)
        if k == traced:
            assert np.array_equal(part, rows)
        _same_state(set_a[k], c)
        assert set_a[k].sweeps_done == first[k] + lengths[k]
    # ... and the closed call of the ladder's first sweeps_done sweeps (every handle ran one order)
    for k, c in enumerate(set_a):
        xs, es = c.result()
        third = _case(sizes[k], 16, 70 + k)
        cxs, ces = sa.anneal_raw(third[2], 900 + k, third[4][:first[k] + lengths[k]], reps[k], k, None,
                                 shuffled=orders[k] == 1)
        assert np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes(), k
    for c in set_a + set_b:
        c.close()


@pytest.mark.parametrize("per_group", [4, 2])
@pytest.mark.parametrize("order", [0, 1])
def test_chains_per_group(order, per_group):
    """Enough chains in the batch that the launcher's rule packs four — or exactly two — per workgroup,
    with a repetition count that is no multiple of it: the last group of every handle is padded.

    The rules (csrc/sa_shuffled.hip, csrc/sa_sweep.hip): the largest m of 4, 2 with
    sum_k ceil(reps_k / m) * w_k >= need, where shuffled: w_k = 1, need = 2 x CUs; colour: w_k = the
    wavefronts of plan k's launch class (read back from a small batch first), need = 4 x CUs."""
    import torch

    from annealing_sign_problem_amd import annealer as sa

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [_case(40, 6, 30 + k) for k in range(8)]
    if order == 1:
        need, waves = 2 * cus, [1] * 8
    else:
        probe = [_case(40, 6, 30 + k) for k in range(8)]
        with_one = [sa.Chains(c[2], seed=1, repetitions=1) for c in probe]
        sa.advance_chains(with_one, [c[4][:1] for c in probe], sweep_order="colour")
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
    chains = [sa.Chains(c[2], seed=40 + k, repetitions=reps) for k, c in enumerate(cases)]
    sa.advance_chains(chains, [c[4] for c in cases], sweep_order=ORDERS[order])
    for c in cases:
        assert _launch(c[2])[0] == per_group
    for k in (0, 5):
        other = _case(40, 6, 30 + k)
        with sa.Chains(other[2], seed=40 + k, repetitions=reps) as single:
            single.advance(other[4], sweep_order=ORDERS[order])
            _same_state(chains[k], single)
    for c in chains:
        c.close()


LARGE_REPS, LARGE_SWEEPS = 5, 5
_LARGE = {}


def _large_chains(ham, j):
    from annealing_sign_problem_amd import annealer as sa

    return sa.Chains(ham, seed=4321 + j, repetitions=LARGE_REPS, replica_offset=2 + j)


def _large(k):
    """Two plans of the cluster of tests/test_gpu_sa_trace_shuffled.py::test_trace_in_the_layouts_of_large_clusters
    (mean degree 6), a schedule, and the state of five chains per plan after the single-handle segment: the
    reference, built once per size."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    if k not in _LARGE:
        J, h, _ = synthetic.planted_cluster(k, seed=5, mean_degree=6.0)
        hams = [sa.Hamiltonian(J, h) for _ in range(2)]
        info = hams[0].info()
        betas = sa.make_schedule(max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6), LARGE_SWEEPS)
        want = []
        for j, ham in enumerate(hams):
            with _large_chains(ham, j) as single:
                single.advance(betas, sweep_order="shuffled")
                want.append(single.state())
        _LARGE[k] = hams, betas, want
    return _LARGE[k]


@pytest.mark.parametrize("k,forced_m,expect_m", [(170000, 4, 4), (170000, 0, 1), (300000, 0, 1)])
def test_batched_segments_in_the_layouts_of_large_clusters(k, forced_m, expect_m):
    """The batched kernels in four bits (four chains per group, the last group ragged, and one chain) and
    one bit per spin — the layout is whatever fits the LDS —: two handles of equal segment length in one
    call are their single-handle segments."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    hams, betas, want = _large(k)
    for ham in hams:
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), forced_m, 0))
    chains = [_large_chains(ham, j) for j, ham in enumerate(hams)]
    try:
        sa.advance_chains(chains, [betas, betas], sweep_order="shuffled")
        for j, c in enumerate(chains):
            assert _launch(hams[j])[0] == expect_m
            got = c.state()
            for name in STATE:
                assert np.array_equal(got[name], want[j][name]), (j, name)
            assert int(got["sweeps_done"]) == LARGE_SWEEPS
    finally:
        for c in chains:
            c.close()
        for ham in hams:
            _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), 0, 0))


@pytest.mark.parametrize("order", [0, 1])
def test_alternation_and_snapshots(order):
    from annealing_sign_problem_amd import annealer as sa

    sizes, reps = (40, 130, 700), (4, 6, 3)
    cases = [_case(n, 20, 80 + k) for k, n in enumerate(sizes)]
    chains = [sa.Chains(c[2], seed=60 + k, repetitions=reps[k], replica_offset=2 * k) for k, c in enumerate(cases)]
    name = ORDERS[order]
    sa.advance_chains(chains, [c[4][:6] for c in cases], sweep_order=name)
    for k, c in enumerate(chains):
        c.advance(cases[k][4][6:11], sweep_order=name)
    states = [c.state() for c in chains]
    for c in chains:
        c.close()
    chains = [sa.Chains(c[2], seed=60 + k, repetitions=reps[k], replica_offset=2 * k) for k, c in enumerate(cases)]
    for c, state in zip(chains, states):
        c.load_state(state)
    sa.advance_chains(chains, [c[4][11:] for c in cases], sweep_order=name)
    for k, c in enumerate(chains):
        xs, es = c.result()
        cxs, ces = sa.anneal_raw(_case(sizes[k], 20, 80 + k)[2], 60 + k, cases[k][4], reps[k], 2 * k, None,
                                 shuffled=order == 1)
        assert np.array_equal(xs, cxs) and es.tobytes() == ces.tobytes()
        c.close()


# (cluster size, problem seed) and the sweeps the CPU oracle says each runs with seed 11, four chains,
# the automatic ladder of 256 sweeps in segments of 32, patience 2, in the shuffled order
# (oracle.sa_anneal_shuffled on truncated ladders): one runs the full ladder, three stop early.
EARLY = ((40, 5, 192), (130, 6, 224), (300, 7, 224), (700, 20, 256))


def test_early_stop():
    from annealing_sign_problem_amd import annealer as sa

    hams = lambda: [sa.Hamiltonian(*_problem(n, seed)) for n, seed, _ in EARLY]
    kw = dict(seed=11, number_sweeps=256, repetitions=4, sweep_order="shuffled", check_every=32)
    batch = sa.anneal_batch_until(hams(), patience=2, **kw)
    single = [sa.anneal_until(h, patience=2, **kw) for h in hams()]
    assert len(batch) == len(single) == len(EARLY)
    for (x, e, ran), (sx, se, sran) in zip(batch, single):
        assert np.array_equal(x, sx) and np.float64(e).tobytes() == np.float64(se).tobytes() and ran == sran
    ran = [r for _, _, r in batch]
    print("sweeps run:", ran)
    assert min(ran) < 256 and max(ran) == 256  # (a condition on the inputs: both branches are exercised)
    assert ran == [expected for _, _, expected in EARLY]
    full = sa.anneal_batch_until(hams(), patience=None, **kw)
    closed = sa.anneal_batch(hams(), seed=11, number_sweeps=256, repetitions=4, sweep_order="shuffled")
    for (x, e, ran_full), (cx, ce) in zip(full, closed):
        assert ran_full == 256
        assert np.array_equal(x, cx) and np.float64(e).tobytes() == np.float64(ce).tobytes()


def test_errors_change_nothing():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    cases = [_case(40, 8, 90), _case(65, 8, 91), _case(130, 8, 92)]
    chains = [sa.Chains(c[2], seed=7 + k, repetitions=3) for k, c in enumerate(cases)]
    twin = sa.Chains(cases[0][2], seed=99, repetitions=2)  # a second handle of plan 0
    sa.advance_chains(chains, [c[4][:3] for c in cases], sweep_order="colour")
    everyone = chains + [twin]
    before = [c.state() for c in everyone]
    nan_betas = cases[2][4][3:8].copy()
    nan_betas[-1] = np.nan

    def call(handles, orders=None, flags=None, betas=None):
        n = len(handles)
        items = (_lib.SaChainsItem * n)()
        keep = []
        for k, c in enumerate(handles):
            b = np.ascontiguousarray(cases[min(k, 2)][4][3:8] if betas is None or betas[k] is None else betas[k])
            best = np.full(c.repetitions, -77, dtype=np.int64)
            rows = np.full((c.repetitions, b.shape[0] + 1), -77, dtype=np.int64)
            improved = ctypes.c_uint32(12345)
            keep.append((b, best, rows, improved))
            items[k].chains = c._live()
            items[k].betas = b.ctypes.data
            items[k].num_sweeps = b.shape[0]
            items[k].order = 0 if orders is None else orders[k]
            items[k].flags = 0 if flags is None else flags[k]
            items[k].out_trace = rows.ctypes.data
            items[k].out_tracked_best = best.ctypes.data
            items[k].out_improved = ctypes.addressof(improved)
        rc = lib.asp_sa_chains_advance_batch(items, ctypes.c_uint32(n))
        message = _lib.last_error()
        for _, best, rows, improved in keep:
            assert np.all(best == -77) and np.all(rows == -77) and improved.value == 12345
        for c, state in zip(everyone, before):
            now = c.state()
            for name in STATE + ("sweeps_done",):
                assert np.array_equal(now[name], state[name])
        return rc, message

    rc, message = call([chains[0], chains[1], chains[0]])
    assert rc == INVALID and "same handle" in message and "0" in message and "2" in message
    rc, message = call([chains[0], chains[1], twin])
    assert rc == INVALID and "one plan" in message and "0" in message and "2" in message
    rc, message = call(chains, orders=[0, 2, 1])
    assert rc == INVALID and "item 1" in message
    rc, message = call(chains, flags=[0, 0, 1])
    assert rc == INVALID and "item 2" in message
    rc, message = call(chains, betas=[None, None, nan_betas])
    assert rc == INVALID and "item 2" in message and "betas[4]" in message
    for c in everyone:
        c.close()
