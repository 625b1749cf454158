"""Resumable annealing chains (asp_sa_chains, annealer.Chains, anneal_until).

Every comparison is exact — np.array_equal on words and traces, energies compared as bytes — except
the one energy identity, which uses the 1e-12 relative tolerance of the energy tests.  The
continuation law is checked against the closed calls AND against the CPU oracle (oracle.sa_anneal,
oracle.sa_anneal_shuffled, oracle.sa_anneal_trace), so that it is not the code against itself.
Problems come from synthetic.planted_cluster, like those of tests/test_gpu_sa.py.
"""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

INVALID = -3
ORDERS = {0: "colour", 1: "shuffled"}


def _case(n, sweeps, seed=5, degree=None):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    kw = {} if degree is None else {"mean_degree": degree}
    J, h, _ = synthetic.planted_cluster(n, seed=seed, **kw)
    h = np.random.default_rng(seed).normal(size=n) * 0.01
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


def _stats(ham, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(ham.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _closed(ham, seed, betas, reps, offset, x0, order):
    """The closed traced call and its asp_sa_last_stats: (xs, es, trace, tracked_best, accepted)."""
    from annealing_sign_problem_amd import annealer as sa

    xs, es, trace = sa.anneal_trace_raw(ham, seed, betas, reps, offset, x0, shuffled=order == 1)
    pxs, pes = sa.anneal_raw(ham, seed, betas, reps, offset, x0, shuffled=order == 1)
    tracked, accepted = _stats(ham, reps)
    assert np.array_equal(xs, pxs) and es.tobytes() == pes.tobytes()
    return xs, es, trace, tracked, accepted


def _form(ham):
    """What the launcher picked for the last call or segment: (asp_sa_last_layout, spins per block of
    the shuffled order's stream, chains per group)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    spins, wgs = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(lib.asp_sa_last_shuffled_blocks(ham.plan(), ctypes.byref(spins), ctypes.byref(wgs)))
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return lib.asp_sa_last_layout(ham.plan()), spins.value, m.value


SEGMENT_FORMS = []  # (order, layout, spins per block, chains per group) of every segment _run_split ran


def _run_split(ham, seed, betas, reps, offset, x0, order, split, checkpoint_after=None, tmp_path=None):
    """create, advance every segment of `split` (tracing), result: (xs, es, trace, final state).
    checkpoint_after = i: after segment i the state is exported, the handle destroyed, and a NEW
    handle continues from the imported state (through np.savez when tmp_path is given)."""
    from annealing_sign_problem_amd import annealer as sa

    assert sum(split) == len(betas)
    chains = sa.Chains(ham, seed=seed, repetitions=reps, x0=x0, replica_offset=offset)
    rows, done, last = [], 0, None
    for i, n in enumerate(split):
        orders = order if isinstance(order, int) else order[i]
        part = chains.advance(betas[done:done + n], sweep_order=ORDERS[orders], trace=True)
        assert part.shape == (reps, n + 1) and part.dtype == np.int64
        if n:
            SEGMENT_FORMS.append((orders,) + _form(ham))
        if rows:
            assert np.array_equal(part[:, 0], last), "entry 0 of a segment is where the last one ended"
        else:
            assert np.all(part[:, 0] == 0)
        rows.append(part if not rows else part[:, 1:])
        last = part[:, -1].copy()
        done += n
        assert chains.sweeps_done == done
        if checkpoint_after == i:
            state = chains.state()
            chains.close()
            if tmp_path is not None:
                np.savez(tmp_path / "chains.npz", **state)
                with np.load(tmp_path / "chains.npz") as loaded:
                    state = {k: loaded[k] for k in loaded.files}
            chains = sa.Chains(ham, seed=seed, repetitions=reps, x0=None, replica_offset=offset)
            chains.load_state(state)
            assert chains.sweeps_done == done
    xs, es = chains.result()
    state = chains.state()
    chains.close()
    return xs, es, np.concatenate(rows, axis=1), state


def _splits(n):
    out = [[n], [n - 1, 1]]
    if n >= 200:
        out.append([7, 0, 64, 129, n - 200])
    return out


def _check_law(J, h, ham, info, betas, seed, reps, offset, x0, orders=(0, 1), splits=None, threads=8,
               form=None):
    """Every split of the schedule, in every order of `orders`, is the closed call and the oracle.
    form(order, layout, spins_per_block, m) -> bool: the launch form the case is there to reach; it
    must hold for every segment the handle ran."""
    S = info.energy_scale_exp
    del SEGMENT_FORMS[:]
    for order in orders:
        xs, es, trace, tracked, accepted = _closed(ham, seed, betas, reps, offset, x0, order)
        ofn = oracle.sa_anneal_shuffled if order == 1 else oracle.sa_anneal
        oxs, oes, otracked, oaccepted = ofn(J, h, seed, betas, reps, offset, x0, S, num_threads=threads)
        otrace = None
        if order == 0:
            txs, tes, otrace = oracle.sa_anneal_trace(J, h, seed, betas, reps, offset, x0, S, num_threads=threads)
            assert np.array_equal(txs, oxs) and tes.tobytes() == oes.tobytes()
        for split in (splits or _splits(len(betas))):
            cxs, ces, ctrace, state = _run_split(ham, seed, betas, reps, offset, x0, order, split)
            what = "order %d split %s" % (order, split if len(split) < 8 else "[1] * %d" % len(split))
            # ... the closed call
            assert np.array_equal(cxs, xs) and ces.tobytes() == es.tobytes(), what
            assert np.array_equal(ctrace, trace), what
            assert np.array_equal(state["tracked_best"], tracked), what
            assert np.array_equal(state["accepted"], accepted), what
            # ... and the oracle
            assert np.array_equal(cxs, oxs) and ces.tobytes() == oes.tobytes(), what
            assert np.array_equal(state["tracked_best"], otracked), what
            assert np.array_equal(state["accepted"], oaccepted), what
            assert np.array_equal(ctrace.min(axis=1), otracked), what
            if otrace is not None:
                assert np.array_equal(ctrace, otrace), what
            assert np.array_equal(state["x_best"], cxs) and int(state["sweeps_done"]) == len(betas)
            assert np.array_equal(state["tracked_current"], ctrace[:, -1])
    assert SEGMENT_FORMS and all(f[1] == (5 if f[0] == 1 else f[1]) for f in SEGMENT_FORMS)
    if form is not None:
        assert all(form(*f) for f in SEGMENT_FORMS), sorted(set(SEGMENT_FORMS))


# ---- the continuation law ------------------------------------------------------------------------
def _packs_lanes(order, layout, spins_per_block, m):
    """Shuffled segments cut their levels into blocks of fewer than 64 spins (lane packing)."""
    return order == 0 or (layout == 5 and spins_per_block < 64)


def _bytes_and_whole_blocks(order, layout, spins_per_block, m):
    """Colour segments keep a byte per position; shuffled ones blocks of 64 spins."""
    return layout == 0 if order == 0 else (layout == 5 and spins_per_block == 64)


@pytest.mark.parametrize("n,degree,sweeps,reps,offset,with_x0,form", [
    (40, 5.0, 260, 64, 0, False, _packs_lanes),
    (200, 8.0, 260, 5, 3, True, _packs_lanes),
    (200, 8.0, 260, 1, 0, False, None),
    (3000, None, 260, 5, 3, False, None),
    (3000, None, 260, 64, 0, True, None),
    # shuffled: the order build as grids over the chunk (forced below, whatever the LDS thresholds
    # are); colour: a byte per position
    (20000, None, 260, 1, 3, False, _bytes_and_whole_blocks),
    (20000, None, 260, 5, 0, True, _bytes_and_whole_blocks),
])
def test_any_split_is_the_closed_call_and_the_oracle(monkeypatch, n, degree, sweeps, reps, offset, with_x0, form):
    if n == 20000:
        # the order build's arrays in HBM: priorities, counts and the stream from grids over the
        # chunk's sweeps (csrc/sa_shuffled.hip, wide_orders) — the path that takes a first sweep t0
        # through a descriptor table
        monkeypatch.setenv("ASP_SHUFFLED_ORDER_IN_HBM", "1")
    J, h, ham, info, betas = _case(n, sweeps, seed=11 + n, degree=degree)
    x0 = _random_x0(n, 3) if with_x0 else None
    _check_law(J, h, ham, info, betas, 20251 + n, reps, offset, x0, form=form)


@pytest.mark.parametrize("n,reps,offset,with_x0", [(200, 5, 3, False), (900, 1, 0, True)])
def test_one_sweep_per_segment(n, reps, offset, with_x0):
    J, h, ham, info, betas = _case(n, 12, seed=n)
    x0 = _random_x0(n, 4) if with_x0 else None
    _check_law(J, h, ham, info, betas, 77, reps, offset, x0, splits=[[1] * 12, [12]])


@pytest.mark.parametrize("packed", [1, 2])
def test_forced_bit_layouts(packed):
    """asp_sa_set_packed(1) / (2): a bit per position in LDS / in HBM (colour order)."""
    from annealing_sign_problem_amd import _lib

    J, h, ham, info, betas = _case(3000, 260, seed=packed)
    _lib.check(_lib.load().asp_sa_set_packed(ham.plan(), packed))
    _check_law(J, h, ham, info, betas, 555, 5, 3, _random_x0(3000, 8) if packed == 2 else None)
    chains_layout = None
    from annealing_sign_problem_amd import annealer as sa

    with sa.Chains(ham, seed=1, repetitions=2) as chains:
        chains.advance(betas[:3], sweep_order="colour")
        chains_layout = _lib.load().asp_sa_last_layout(ham.plan())
    assert chains_layout == (1 if packed == 1 else 3)


def test_forced_team_is_honoured_by_the_closed_call_and_ignored_by_the_handle():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(3000, 260, seed=21)
    lib = _lib.load()
    _lib.check(lib.asp_sa_set_team(ham.plan(), 2))
    sa.anneal_raw(ham, 1, betas[:4], 5)
    assert lib.asp_sa_last_layout(ham.plan()) == 4, "the closed call runs teams"
    _check_law(J, h, ham, info, betas, 999, 5, 0, None, orders=(0,))
    with sa.Chains(ham, seed=1, repetitions=5) as chains:
        chains.advance(betas[:4], sweep_order="colour")
        assert lib.asp_sa_last_layout(ham.plan()) != 4, "a handle runs no team launches"


@pytest.mark.parametrize("m", [2, 4, 8])
def test_forced_chains_per_group_with_a_ragged_last_group(m):
    """asp_sa_set_launch / asp_sa_set_shuffled_launch: 2, 4 (the word layouts) and 8 chains per
    workgroup, 13 chains — the last group is padded."""
    from annealing_sign_problem_amd import _lib

    J, h, ham, info, betas = _case(900, 260, seed=m)
    lib = _lib.load()
    _lib.check(lib.asp_sa_set_launch(ham.plan(), m, 0))
    _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, 0))
    def forced(order, layout, spins_per_block, chains):
        # m chains per group in both orders; the colour order's word layout at four
        return chains == m and (order == 1 or layout == (2 if m == 4 else 0))

    _check_law(J, h, ham, info, betas, 4242, 13, 3, _random_x0(900, 5) if m == 4 else None, form=forced)
    if m == 4:  # ... and two teams of two chains per shuffled workgroup
        _lib.check(lib.asp_sa_set_shuffled_teams(ham.plan(), 2))
        _check_law(J, h, ham, info, betas, 4243, 13, 0, None, orders=(1,), splits=[[7, 0, 64, 129, 60]],
                   form=lambda order, layout, spins_per_block, chains: chains == 4)


# ---- export / import -----------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n,reps,offset", [(200, 5, 3), (3000, 64, 0)])
def test_export_destroy_import_continue(tmp_path, order, n, reps, offset):
    J, h, ham, info, betas = _case(n, 160, seed=n + order)
    x0 = _random_x0(n, 6)
    split = [50, 0, 70, 40]
    direct = _run_split(ham, 31, betas, reps, offset, x0, order, split)
    xs, es, trace, tracked, accepted = _closed(ham, 31, betas, reps, offset, x0, order)
    for after, path in ((0, None), (2, tmp_path)):
        resumed = _run_split(ham, 31, betas, reps, offset, x0, order, split, checkpoint_after=after, tmp_path=path)
        for got in (direct, resumed):
            assert np.array_equal(got[0], xs) and got[1].tobytes() == es.tobytes()
            assert np.array_equal(got[2], trace)
            assert np.array_equal(got[3]["tracked_best"], tracked) and np.array_equal(got[3]["accepted"], accepted)
        for key in direct[3]:
            assert np.array_equal(np.asarray(resumed[3][key]), np.asarray(direct[3][key])), key


# ---- per-chain starts ----------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_per_chain_starts_are_single_chains_with_that_start(order):
    from annealing_sign_problem_amd import annealer as sa

    n, reps, offset = 900, 5, 3
    J, h, ham, info, betas = _case(n, 60, seed=9)
    x0 = _random_x0(n, 12, rows=reps)
    assert len({row.tobytes() for row in x0}) == reps
    with sa.Chains(ham, seed=8, repetitions=reps, x0=x0, replica_offset=offset) as chains:
        assert np.array_equal(chains.state()["x_current"], x0)
        trace = np.concatenate([chains.advance(betas[:25], sweep_order=ORDERS[order], trace=True),
                                chains.advance(betas[25:], sweep_order=ORDERS[order], trace=True)[:, 1:]], axis=1)
        xs, es = chains.result()
        state = chains.state()
    ofn = oracle.sa_anneal_shuffled if order == 1 else oracle.sa_anneal
    for r in range(reps):
        with sa.Chains(ham, seed=8, repetitions=1, x0=x0[r], replica_offset=offset + r) as one:
            one_trace = one.advance(betas, sweep_order=ORDERS[order], trace=True)
            one_xs, one_es = one.result()
            one_state = one.state()
        assert np.array_equal(one_xs[0], xs[r]) and one_es.tobytes() == es[r:r + 1].tobytes()
        assert np.array_equal(one_trace[0], trace[r])
        for key in ("x_current", "x_best", "tracked_current", "tracked_best", "accepted"):
            assert np.array_equal(one_state[key][0], state[key][r]), key
        # ... which is the closed call with that shared start, and the oracle's
        cxs, ces = sa.anneal_raw(ham, 8, betas, 1, offset + r, x0[r], shuffled=order == 1)
        assert np.array_equal(cxs[0], xs[r]) and ces.tobytes() == es[r:r + 1].tobytes()
        oxs, oes, otracked, oaccepted = ofn(J, h, 8, betas, 1, offset + r, x0[r], info.energy_scale_exp)
        assert np.array_equal(oxs[0], xs[r]) and oes.tobytes() == es[r:r + 1].tobytes()
        assert otracked[0] == state["tracked_best"][r] and oaccepted[0] == state["accepted"][r]


# ---- mixed orders --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,reps", [(200, 5), (3000, 13)])
def test_segments_may_change_the_order(tmp_path, n, reps):
    """shuffled, colour, shuffled: no closed call does this, so the run is pinned by export/import
    in mid-run reproducing the direct run and by the energy identity after every segment."""
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(n, 150, seed=3 * n)
    x0 = _random_x0(n, 2, rows=reps)
    split, orders = [60, 50, 40], [1, 0, 1]
    unit = 2.0 ** -info.energy_scale_exp
    chains = sa.Chains(ham, seed=5, repetitions=reps, x0=x0, replica_offset=2)
    e_start = ham.energies(x0)
    done = 0
    for count, order in zip(split, orders):
        chains.advance(betas[done:done + count], sweep_order=ORDERS[order])
        done += count
        state = chains.state()
        for key, tracked in (("x_current", "tracked_current"), ("x_best", "tracked_best")):
            want = e_start + state[tracked].astype(np.float64) * unit
            got = ham.energies(state[key])
            worst = float(np.max(np.abs(got - want) / np.abs(want)))
            print("energy identity, %s after %d sweeps: worst relative difference %.3g" % (key, done, worst))
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (key, done, worst)
        assert np.all(state["tracked_best"] <= state["tracked_current"]) and np.all(state["tracked_best"] <= 0)
    direct_xs, direct_es = chains.result()
    direct_state = chains.state()
    chains.close()
    assert direct_es.tobytes() == ham.energies(direct_xs).tobytes()
    for after in (0, 1):
        xs, es, _, state = _run_split(ham, 5, betas, reps, 2, x0, orders, split, checkpoint_after=after,
                                      tmp_path=tmp_path)
        assert np.array_equal(xs, direct_xs) and es.tobytes() == direct_es.tobytes()
        for key in direct_state:
            assert np.array_equal(np.asarray(state[key]), np.asarray(direct_state[key])), key


# ---- anneal_until --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_anneal_until_without_patience_is_anneal(order):
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(900, 8, seed=17)
    x, e = sa.anneal(ham, seed=3, number_sweeps=300, repetitions=7, sweep_order=order, distributed=False)
    ux, ue, sweeps = sa.anneal_until(ham, seed=3, number_sweeps=300, repetitions=7, sweep_order=order,
                                     check_every=64, patience=None)
    assert sweeps == 300 and np.array_equal(ux, x) and ue == e
    xs, es = sa.anneal(ham, seed=3, number_sweeps=300, repetitions=7, sweep_order=order, only_best=False,
                       distributed=False)
    uxs, ues, _ = sa.anneal_until(ham, seed=3, number_sweeps=300, repetitions=7, sweep_order=order,
                                  check_every=299, only_best=False)
    assert np.array_equal(uxs, xs) and ues.tobytes() == es.tobytes()


def test_anneal_until_stops_early_on_a_planted_cluster():
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(300, 8, seed=23)
    number_sweeps, every = 6000, 250
    xs, es, sweeps = sa.anneal_until(ham, seed=9, number_sweeps=number_sweeps, repetitions=6, check_every=every,
                                     patience=2, only_best=False, sweep_order="shuffled")
    assert sweeps < number_sweeps and sweeps % every == 0
    # the same segments by hand
    info = ham.info()
    ladder = sa.make_schedule(info.beta0_auto, info.beta1_auto, number_sweeps)
    with sa.Chains(ham, seed=9, repetitions=6) as chains:
        for first in range(0, sweeps, every):
            chains.advance(ladder[first:first + every], sweep_order="shuffled")
        hxs, hes = chains.result()
        tracked = chains.state()["tracked_best"]
    assert np.array_equal(hxs, xs) and hes.tobytes() == es.tobytes()
    # ... which had indeed stopped improving: the last two segments changed no chain's best
    with sa.Chains(ham, seed=9, repetitions=6) as chains:
        for first in range(0, sweeps - 2 * every, every):
            chains.advance(ladder[first:first + every], sweep_order="shuffled")
        assert np.array_equal(chains.state()["tracked_best"], tracked)
    oxs, oes, _, _ = oracle.sa_anneal_shuffled(J, h, 9, ladder[:sweeps], 6, 0, None, info.energy_scale_exp,
                                               num_threads=8)
    assert np.array_equal(oxs, xs) and oes.tobytes() == es.tobytes()


# ---- argument checks that need a plan ------------------------------------------------------------
def test_invalid_arguments_return_before_any_launch_and_write_nothing():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(200, 8, seed=1)  # 4 words
    lib = _lib.load()
    plan = ham.plan()

    def invalid(rc):
        assert rc == INVALID and lib.asp_last_error_code() == INVALID and _lib.last_error()

    x0 = _random_x0(200, 1, rows=3)
    handle = ctypes.c_void_p(0x5A5A)
    for stride in (1, 3):
        invalid(lib.asp_sa_chains_create(plan, ctypes.c_uint64(1), ctypes.c_uint32(3), ctypes.c_uint32(0),
                                         _lib.ptr(x0), ctypes.c_uint64(stride), ctypes.byref(handle)))
    invalid(lib.asp_sa_chains_create(plan, ctypes.c_uint64(1), ctypes.c_uint32(3), ctypes.c_uint32(0),
                                     None, ctypes.c_uint64(0), None))
    invalid(lib.asp_sa_chains_create(plan, ctypes.c_uint64(1), ctypes.c_uint32(3), ctypes.c_uint32(2**32 - 4),
                                     None, ctypes.c_uint64(0), ctypes.byref(handle)))
    assert handle.value == 0x5A5A

    chains = sa.Chains(ham, seed=1, repetitions=3, x0=x0)
    before = chains.state()
    trace = np.full((3, 9), 77, dtype=np.int64)
    raw = chains._handle
    invalid(lib.asp_sa_chains_advance(raw, None, ctypes.c_uint32(8), ctypes.c_uint32(0), _lib.ptr(trace)))
    for order in (2, 7, 2**32 - 1):
        invalid(lib.asp_sa_chains_advance(raw, _lib.ptr(betas), ctypes.c_uint32(8), ctypes.c_uint32(order),
                                          _lib.ptr(trace)))
    bad = betas.copy()
    bad[5] = np.nan
    invalid(lib.asp_sa_chains_advance(raw, _lib.ptr(bad), ctypes.c_uint32(8), ctypes.c_uint32(1), _lib.ptr(trace)))
    xs, es = np.full((3, 4), 5, dtype=np.uint64), np.full(3, 5.0)
    invalid(lib.asp_sa_chains_result(raw, None, _lib.ptr(es)))
    invalid(lib.asp_sa_chains_result(raw, _lib.ptr(xs), None))
    invalid(lib.asp_sa_chains_export(raw, None))
    invalid(lib.asp_sa_chains_import(raw, None))
    # a snapshot that lacks one of its five arrays
    names = ["x_current", "x_best", "tracked_current", "tracked_best", "accepted"]
    for missing in names:
        snap = _lib.SaChainsSnapshot()
        for name in names:
            if name != missing:
                setattr(snap, name, before[name].ctypes.data)
        snap.sweeps_done = 99
        invalid(lib.asp_sa_chains_import(raw, ctypes.byref(snap)))
    assert np.all(trace == 77) and np.all(xs == 5) and np.all(es == 5.0)
    after = chains.state()
    for key in before:
        assert np.array_equal(np.asarray(after[key]), np.asarray(before[key])), key
    assert chains.sweeps_done == 0

    # the sweep index is 32 bits with 2^32 - 1 reserved: a snapshot far into a run leaves room for
    # exactly 2^32 - 2 - sweeps_done more sweeps
    huge = dict(before, sweeps_done=np.uint32(2**32 - 2 - 5))
    chains.load_state(huge)
    assert chains.sweeps_done == 2**32 - 7
    invalid(lib.asp_sa_chains_advance(raw, _lib.ptr(betas), ctypes.c_uint32(6), ctypes.c_uint32(0), None))
    invalid(lib.asp_sa_chains_advance(raw, _lib.ptr(betas), ctypes.c_uint32(6), ctypes.c_uint32(1), None))
    assert chains.sweeps_done == 2**32 - 7
    with pytest.raises(_lib.AspError) as err:
        chains.advance(betas[:8], sweep_order="colour")
    assert err.value.code == INVALID
    # ... and the last five sweep indices are usable, in either order
    chains.advance(betas[:2], sweep_order="shuffled")
    chains.advance(betas[2:5], sweep_order="colour")
    assert chains.sweeps_done == 2**32 - 2
    chains.advance(betas[:0])  # no sweeps: fine
    with pytest.raises(_lib.AspError):
        chains.advance(betas[:1])
    with pytest.raises(ValueError, match="sweeps_done"):
        chains.load_state(dict(before, sweeps_done=2**32))
    with pytest.raises(ValueError, match="shape"):
        chains.load_state(dict(before, accepted=np.zeros(2, dtype=np.uint64)))
    chains.close()
    with pytest.raises(ValueError, match="closed"):
        chains.advance(betas[:1])
    chains.close()  # twice is fine


def test_the_sweep_counter_enters_the_random_words_and_the_orders_whatever_the_launch_form():
    """Sweep k of a segment draws with t = sweeps_done + k.  No closed call starts at t > 0, so a
    handle whose counter was moved far out (import) is pinned from two sides: its chains are the same
    in every launch form (one and four chains per workgroup, both orders), and they are NOT the
    chains of the handle whose counter stayed at 0."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(900, 40, seed=2)
    x0 = _random_x0(900, 3)
    lib = _lib.load()
    results = {}
    for moved in (0, 3_000_000_000):
        for m in (0, 4):
            _lib.check(lib.asp_sa_set_launch(ham.plan(), m, 0))
            _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, 0))
            for order in (0, 1):
                with sa.Chains(ham, seed=6, repetitions=6, x0=x0) as chains:
                    chains.load_state(dict(chains.state(), sweeps_done=np.uint32(moved)))
                    trace = chains.advance(betas, sweep_order=ORDERS[order], trace=True)
                    results[(moved, m, order)] = (trace, chains.result()[0])
    for moved in (0, 3_000_000_000):
        for order in (0, 1):
            a, b = results[(moved, 0, order)], results[(moved, 4, order)]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for order in (0, 1):
        assert not np.array_equal(results[(0, 0, order)][0], results[(3_000_000_000, 0, order)][0])


def test_plans_without_spins():
    """K = 0 behaves as in the closed calls: nothing runs, energies 0, traces of zeros."""
    import scipy.sparse

    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(scipy.sparse.csr_matrix((0, 0)), np.zeros(0))
    with sa.Chains(ham, seed=1, repetitions=3) as chains:
        trace = chains.advance(np.ones(4), sweep_order="shuffled", trace=True)
        assert trace.shape == (3, 5) and np.all(trace == 0)
        assert np.all(chains.advance(np.ones(2), sweep_order="colour", trace=True) == 0)
        xs, es = chains.result()
        assert xs.shape == (3, 0) and np.all(es == 0.0) and chains.sweeps_done == 6
        state = chains.state()
        chains.load_state(state)
        assert chains.sweeps_done == 6
