"""Per-sweep energy traces of the shuffled (default) sweep order: asp_sa_anneal_shuffled_trace and
the Python surface on top of it (anneal_trace_raw(shuffled=True), anneal_traces,
anneal_with_traces(sweep_order=)).

The oracle has no shuffled trace (only its colour-ordered chain reports one), so the trace is pinned
from several sides: the traced call is the untraced call and the oracle's chains; the running
minimum of the trace is the oracle's tracked best of every PREFIX of the ladder (the orders and
random words of sweep t depend on t alone, so betas[:t] is a prefix of the run); at record sweeps
the current energy is the oracle's reported energy of that prefix; where the order cannot matter
(no couplings) the trace is the oracle's colour trace at every sweep; and every launch form —
chunks, chains per group, wavefronts, teams, lane packing, ragged groups, replica offsets — writes
the same rows.  Problems come from synthetic.planted_cluster, like those of tests/test_gpu_sa.py.
"""
import ctypes
import re
import os

import numpy as np
import pytest
import scipy.sparse

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planted(n, seed, **kw):
    from annealing_sign_problem_amd import synthetic

    return synthetic.planted_cluster(n, seed=seed, **kw)


def _case(n, degree, sweeps, seed=5, field_sigma=0.0, **kw):
    from annealing_sign_problem_amd import annealer as sa

    J, h, _ = _planted(n, seed, mean_degree=degree, **kw)
    if field_sigma:
        h = np.random.default_rng(seed).normal(size=n) * field_sigma
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = sa.make_schedule(max(info.beta0_auto, 1e-3), min(max(info.beta1_auto, 1.0), 1e6), sweeps)
    return J, h, ham, info, betas


def _stats(ham, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(ham.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _form(ham):
    """What the launcher picked for the last call: (layout, spins per block, workgroups, chains per
    group, threads, groups)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    spins, wgs = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(lib.asp_sa_last_shuffled_blocks(ham.plan(), ctypes.byref(spins), ctypes.byref(wgs)))
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return (lib.asp_sa_last_layout(ham.plan()), spins.value, wgs.value, m.value, threads.value, groups.value)


def _random_x0(n, seed):
    from annealing_sign_problem_amd import annealer as sa

    return sa.signs_to_bits(np.where(np.random.default_rng(seed).random(n) < 0.5, 1.0, -1.0))


def _traced_equals_untraced(ham, seed, betas, reps, offset, x0):
    """Runs both calls; asserts test 1's equalities and test 6's (same form); returns the traced
    call's (xs, es, trace, tracked, accepted)."""
    from annealing_sign_problem_amd import annealer as sa

    pxs, pes = sa.anneal_raw(ham, seed, betas, reps, offset, x0, shuffled=True)
    ptracked, paccepted = _stats(ham, reps)
    plain_form = _form(ham)
    xs, es, trace = sa.anneal_trace_raw(ham, seed, betas, reps, offset, x0, shuffled=True)
    tracked, accepted = _stats(ham, reps)
    assert _form(ham) == plain_form, "tracing changed the kernel form"
    assert plain_form[0] == 5
    assert np.array_equal(xs, pxs) and es.tobytes() == pes.tobytes()
    assert np.array_equal(tracked, ptracked) and np.array_equal(accepted, paccepted)
    assert trace.shape == (reps, len(betas) + 1) and trace.dtype == np.int64
    assert np.array_equal(trace.min(axis=1), tracked), "the trace's minimum is the tracked best"
    return xs, es, trace, tracked, accepted


# 1 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,degree,sweeps,reps,offset,with_x0", [
    (900, 12.0, 30, 7, 0, False),
    (900, 12.0, 30, 7, 3, False),
    (900, 12.0, 24, 5, 6, True),
    (70, 5.0, 36, 13, 2, False),     # packs lanes by itself
    (6000, 23.0, 24, 4, 1, True),
])
def test_traced_call_runs_the_same_chains(n, degree, sweeps, reps, offset, with_x0):
    """Same arguments: xs, es, tracked best and accepted counts of the traced call are those of
    anneal_raw(shuffled=True) bit for bit, and the oracle's."""
    J, h, ham, info, betas = _case(n, degree, sweeps, seed=70 + n, field_sigma=0.01)
    x0 = _random_x0(n, 2) if with_x0 else None
    xs, es, trace, tracked, accepted = _traced_equals_untraced(ham, 31337, betas, reps, offset, x0)
    oxs, oes, otracked, oaccepted = oracle.sa_anneal_shuffled(J, h, 31337, betas, reps, offset, x0,
                                                             info.energy_scale_exp, num_threads=4)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    assert np.array_equal(tracked, otracked) and np.array_equal(accepted, oaccepted)
    assert np.all(trace[:, 0] == 0)


# 2 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,degree,sweeps,reps,offset", [(900, 12.0, 24, 7, 3), (150, 15.0, 40, 10, 0)])
def test_running_minimum_is_the_oracles_tracked_best_of_every_prefix(n, degree, sweeps, reps, offset):
    """For every t in 0..T: min(trace[r, :t + 1]) == out_tracked[r] of the oracle's run of betas[:t]."""
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(n, degree, sweeps, seed=n, field_sigma=0.01)
    _, _, trace = sa.anneal_trace_raw(ham, 99, betas, reps, offset, None, shuffled=True)
    assert np.all(trace[:, 0] == 0)
    running = np.minimum.accumulate(trace, axis=1)
    for t in range(sweeps + 1):
        _, _, otracked, _ = oracle.sa_anneal_shuffled(J, h, 99, betas[:t], reps, offset, None,
                                                      info.energy_scale_exp, num_threads=4)
        assert np.array_equal(running[:, t], otracked), "prefix of %d sweeps" % t


# 3 -------------------------------------------------------------------------------------------
def test_current_energy_at_record_sweeps():
    """Where trace[r, t] is a strict new minimum, the oracle's best configuration of the prefix
    betas[:t] is the state after sweep t - 1 (the t-th), so its reported energy is the chain's
    current energy there: E(x0) + trace[r, t] 2^-S must agree with it.

    The tolerance is the rounding of the bookkeeping, nothing measured:
      * an accepted flip adds q = rint(dE 2^S), so q 2^-S differs from the dE the
        kernel computed by at most 1/2 2^-S;
      * that dE is itself rounded: acc is a sequential f64 sum over the d couplings of the row and
        g = acc + h_i one more add (dE = +-2 g is exact), so |computed dE - exact dE| <=
        2 d u (sum_j |A_ij| + |h_i|) < d 2^-53 2^e1 with u = 2^-53 and e1 of §4.5
        (max_i 2 (sum_j |A_ij| + |h_i|) < 2^e1).  S <= 50 - e1, hence this is <= d / 8 2^-S, and
        the problem below has rows of at most d = 4 couplings: <= 1/2 2^-S;
      together at most 2^-S per accepted flip: `accepted` flips x 2^-S, with the oracle's accepted
      count of the prefix run;
      * E(x0) (oracle.sa_energy) and the oracle's out_e are f64 sums of the nnz + K terms
        J_ij s_i s_j and h_i s_i: in any summation order the error of one such sum is at most
        (terms - 1) u / (1 - (terms - 1) u) x sum |term| (Higham, Accuracy and Stability of Numerical
        Algorithms, §4.2); a term may carry one more rounding (A_ij = J_ij + J_ji, §4.2; the halving
        of §4.6 is exact), so (1 + u)^(terms + 1) - 1 <= (terms + 2) u for terms x u << 1:
        (terms + 2) 2^-53 (sum |J_ij| + sum |h_i|) per sum, two sums."""
    from annealing_sign_problem_amd import annealer as sa

    n, sweeps, reps = 600, 32, 8
    J, h, ham, info, betas = _case(n, 3.0, sweeps, seed=12, field_sigma=0.01, max_degree=4)
    A = (J + J.T).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    assert np.diff(A.indptr).max() <= 4, "the derivation above needs rows of at most four couplings"
    S = info.energy_scale_exp
    unit = 2.0 ** -S
    x0 = _random_x0(n, 7)
    e0 = float(oracle.sa_energy(J, h, x0)[0])
    terms = J.nnz + n
    summation = 2.0 * (terms + 2) * 2.0 ** -53 * (np.abs(J.data).sum() + np.abs(h).sum())
    _, _, trace = sa.anneal_trace_raw(ham, 4242, betas, reps, 1, x0, shuffled=True)
    running = np.minimum.accumulate(trace, axis=1)
    records = 0
    for t in range(1, sweeps + 1):
        new_minimum = trace[:, t] < running[:, t - 1]
        if not new_minimum.any():
            continue
        _, oe, otracked, oaccepted = oracle.sa_anneal_shuffled(J, h, 4242, betas[:t], reps, 1, x0, S, num_threads=4)
        for r in np.nonzero(new_minimum)[0]:
            assert otracked[r] == trace[r, t]
            got = e0 + float(trace[r, t]) * unit
            bound = float(oaccepted[r]) * unit + summation
            print("chain %d sweep %d: |%.17g - %.17g| = %.3g <= %.3g" % (r, t, got, oe[r], abs(got - oe[r]), bound))
            assert abs(got - oe[r]) <= bound
            records += 1
    assert records >= reps  # every chain improves on a random start at least once


# 4 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,reps,offset", [(333, 9, 0), (64, 5, 2), (1000, 70, 5)])
def test_without_couplings_the_trace_is_the_colour_trace(n, reps, offset):
    """A field and no off-diagonal couplings: no spin sees another, the random word is keyed by
    (spin, sweep, replica), so the shuffled and the colour chain coincide spin by spin and the
    shuffled trace is oracle.sa_anneal_trace's at every sweep."""
    from annealing_sign_problem_amd import annealer as sa

    rng = np.random.default_rng(n)
    J = scipy.sparse.diags(rng.integers(-3, 4, size=n).astype(np.float64)).tocsr()
    field = rng.normal(size=n)
    betas = np.geomspace(0.1, 20.0, 28)
    ham = sa.Hamiltonian(J, field)
    S = ham.info().energy_scale_exp
    for x0 in (None, _random_x0(n, 3)):
        xs, es, trace = sa.anneal_trace_raw(ham, 17, betas, reps, offset, x0, shuffled=True)
        oxs, oes, otrace = oracle.sa_anneal_trace(J, field, 17, betas, reps, offset, x0, S, num_threads=4)
        assert np.array_equal(trace, otrace)
        assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
        assert trace.min() < 0 and np.any(np.diff(trace, axis=1) > 0)  # the chains move, up as well


# 5 and 6 -------------------------------------------------------------------------------------
def _max_chunk_sweeps():
    """The most sweeps of one chunk of visiting orders, read from the launcher's source."""
    source = open(os.path.join(ROOT, "annealing_sign_problem_amd", "csrc", "sa_shuffled.hip")).read()
    found = re.search(r"chunk = static_cast<uint32_t>\(std::max<uint64_t>\(1, std::min<uint64_t>\((\d+), budget / per_sweep\)\)\);",
                      source)
    assert found, "the chunk size moved: update this pattern"
    return int(found.group(1))


def test_every_launch_form_writes_the_same_trace(monkeypatch):
    """One problem with couplings, more sweeps than a chunk can hold: chains per group, wavefronts,
    two teams, the forced spin layouts of the plan, small chunks, ragged last groups and a split
    into two calls with a replica offset all give the same rows, bit for bit; and (test 6) the
    traced call reports the form of the untraced one every time."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    sweeps = _max_chunk_sweeps() + 14
    assert sweeps > 256
    J, h, ham, info, betas = _case(1300, 9.0, sweeps, seed=5, field_sigma=0.01)
    lib = _lib.load()
    reps, seed = 67, 77

    def run(count=reps, offset=0):
        return _traced_equals_untraced(ham, seed, betas, count, offset, None)[2]

    reference = run()
    auto_form = _form(ham)
    assert reference.min() < 0 and len({row.tobytes() for row in reference}) == reps
    forms = {auto_form}
    for m, waves in [(1, 1), (1, 8), (2, 3), (4, 1), (4, 5), (8, 2), (8, 8)]:
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, waves))
        assert np.array_equal(run(), reference), (m, waves)
        assert _form(ham)[3:5] == (m, 64 * waves)
        forms.add(_form(ham))
    for m, waves in [(2, 2), (4, 4), (8, 3)]:
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, waves))
        _lib.check(lib.asp_sa_set_shuffled_teams(ham.plan(), 2))
        assert np.array_equal(run(), reference), ("teams", m, waves)
        assert _form(ham)[3:5] == (m, 128 * waves)
        _lib.check(lib.asp_sa_set_shuffled_teams(ham.plan(), 0))
    _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), 0, 0))
    # the plan's forced spin layouts (the shuffled sweep picks its own layout by size and chains per
    # group — words above for 1, 2, 4 chains, bytes for 8 —, whatever these say)
    for setter, value, restore in ((lib.asp_sa_set_packed, 1, 0), (lib.asp_sa_set_packed, 2, 0),
                                   (lib.asp_sa_set_wide, 0, 1)):
        _lib.check(setter(ham.plan(), value))
        assert np.array_equal(run(), reference), (setter.__name__, value)
        _lib.check(setter(ham.plan(), restore))
    # chunks of a few sweeps (a small budget of order bytes per buffer set)
    monkeypatch.setenv("ASP_SHUFFLED_BYTES", str(8 << 20))
    assert np.array_equal(run(), reference)
    monkeypatch.delenv("ASP_SHUFFLED_BYTES")
    # repetitions that do not fill the last group: rows are those of the same global replicas
    for m in (0, 4, 8):
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, 0))
        assert np.array_equal(run(5), reference[:5]), m
        assert np.array_equal(run(3, 64), reference[64:]), m
    _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), 0, 0))
    # a split into two calls
    assert np.array_equal(np.concatenate([run(30), run(37, 30)]), reference)
    assert len(forms) >= 7


def test_lane_packing_writes_the_same_trace(monkeypatch):
    """A small-level problem that packs lanes by itself (several chain groups per wavefront), with
    more sweeps than a chunk holds: packed and unpacked calls, block sizes, chains per group, ragged
    counts (5, 67) and a split with replica_offset write the same rows; the traced call packs
    exactly as the untraced one does."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    sweeps = _max_chunk_sweeps() + 14
    J, h, ham, info, betas = _case(90, 20.0, sweeps, seed=90)
    lib = _lib.load()
    reps, seed = 67, 4711

    def run(count=reps, offset=0):
        return _traced_equals_untraced(ham, seed, betas, count, offset, None)[2]

    reference = run()
    assert _form(ham)[1] < 64, "expected a call that packs lanes by itself"
    monkeypatch.setenv("ASP_SHUFFLED_NO_PACKING", "1")
    assert np.array_equal(run(), reference)
    assert _form(ham)[1] == 64
    monkeypatch.delenv("ASP_SHUFFLED_NO_PACKING")
    for m, log_s in [(1, 2), (2, 3), (4, 2), (4, 4), (4, 5)]:
        _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, 0))
        monkeypatch.setenv("ASP_SHUFFLED_LOG_S", str(log_s))
        assert np.array_equal(run(), reference), (m, log_s)
        assert _form(ham)[1] == 1 << log_s and _form(ham)[3] == m
        assert np.array_equal(run(5), reference[:5]), (m, log_s)
        assert np.array_equal(np.concatenate([run(30), run(37, 30)]), reference), (m, log_s)
    monkeypatch.delenv("ASP_SHUFFLED_LOG_S")
    _lib.check(lib.asp_sa_set_shuffled_launch(ham.plan(), 0, 0))
    # against the oracle, once: the minimum of every row
    _, _, otracked, _ = oracle.sa_anneal_shuffled(J, h, seed, betas, reps, 0, None, info.energy_scale_exp,
                                                  num_threads=8)
    assert np.array_equal(reference.min(axis=1), otracked)


@pytest.mark.parametrize("k,forced_m,expect_m", [(70000, 4, 4), (170000, 4, 4), (300000, 0, 1)])
def test_trace_in_the_layouts_of_large_clusters(k, forced_m, expect_m):
    """A byte, four bits and one bit per spin (clusters beyond a word per spin): the traced call is
    the untraced one, in the same form, and the running minimum is the oracle's tracked best of the
    whole run and of a prefix."""
    from annealing_sign_problem_amd import _lib

    J, h, ham, info, betas = _case(k, 6.0, 5, seed=5)
    _lib.check(_lib.load().asp_sa_set_shuffled_launch(ham.plan(), forced_m, 0))
    xs, es, trace, tracked, accepted = _traced_equals_untraced(ham, 4321, betas, 5, 2, None)
    assert _form(ham)[3] == expect_m
    running = np.minimum.accumulate(trace, axis=1)
    for t in (2, 5):
        _, _, otracked, _ = oracle.sa_anneal_shuffled(J, h, 4321, betas[:t], 5, 2, None, info.energy_scale_exp,
                                                      num_threads=8)
        assert np.array_equal(running[:, t], otracked)


# 7 -------------------------------------------------------------------------------------------
def test_python_surface(monkeypatch):
    from annealing_sign_problem_amd import annealer as sa

    monkeypatch.delenv("ASP_SWEEP_ORDER", raising=False)
    J, h, ham, info, _ = _case(500, 8.0, 1, seed=31, field_sigma=0.02)
    T, s = 36, 2024
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, T)
    unit = 2.0 ** -info.energy_scale_exp

    def anchored(es, trace):
        best = np.minimum.accumulate(trace)
        return es + (trace - best[-1]).astype(np.float64) * unit, es + (best - best[-1]).astype(np.float64) * unit

    # the default is unchanged: the colour chain, anchored at the returned configuration's energy
    x, e_current, e_best = sa.anneal_with_traces(ham, seed=s, number_sweeps=T)
    cxs, ces, ctrace = sa.anneal_trace_raw(ham, s, betas, 1, 0, None)
    want_current, want_best = anchored(ces[0], ctrace[0])
    assert np.array_equal(x, cxs[0])
    assert e_current.tobytes() == want_current.tobytes() and e_best.tobytes() == want_best.tobytes()
    # the shuffled order by name, and through None (what anneal() runs)
    ax, ae = sa.anneal(ham, seed=s, number_sweeps=T, repetitions=1, sweep_order="shuffled")
    for order in ("shuffled", None):
        x, e_current, e_best = sa.anneal_with_traces(ham, seed=s, number_sweeps=T, sweep_order=order)
        assert np.array_equal(x, ax)
        assert e_current.shape == (T + 1,) and e_best.shape == (T + 1,)
        assert np.all(np.diff(e_best) <= 0)
        assert e_best[-1] == ae
        assert np.all(e_current >= e_best)
    assert not np.array_equal(ax, cxs[0])
    monkeypatch.setenv("ASP_SWEEP_ORDER", "colour")
    x, _, _ = sa.anneal_with_traces(ham, seed=s, number_sweeps=T, sweep_order=None)
    assert np.array_equal(x, cxs[0])
    monkeypatch.delenv("ASP_SWEEP_ORDER")
    # anneal_traces: rows are single calls with replica_offset 0, 1, 2; default order = anneal()'s
    xs, es, cur, best = sa.anneal_traces(ham, seed=s, number_sweeps=T, repetitions=3)
    axs, aes = sa.anneal(ham, seed=s, number_sweeps=T, repetitions=3, only_best=False)
    assert np.array_equal(xs, axs) and es.tobytes() == aes.tobytes()
    assert cur.shape == (3, T + 1) and best.shape == (3, T + 1)
    for r in range(3):
        rxs, res, rtrace = sa.anneal_trace_raw(ham, s, betas, 1, r, None, shuffled=True)
        want_current, want_best = anchored(res[0], rtrace[0])
        assert np.array_equal(xs[r], rxs[0]) and es[r] == res[0]
        assert cur[r].tobytes() == want_current.tobytes() and best[r].tobytes() == want_best.tobytes()
    # one repetition in the same order: the chain of anneal_with_traces
    for order in ("colour", "shuffled"):
        x, e_current, e_best = sa.anneal_with_traces(ham, seed=s, number_sweeps=T, sweep_order=order)
        xs, es, cur, best = sa.anneal_traces(ham, seed=s, number_sweeps=T, repetitions=1, sweep_order=order)
        assert np.array_equal(xs[0], x) and cur[0].tobytes() == e_current.tobytes()
        assert best[0].tobytes() == e_best.tobytes() and best[0, -1] == es[0]


# 8 and the edges -------------------------------------------------------------------------------
def test_errors_and_empty_ladders():
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    J, h, ham, info, betas = _case(300, 6.0, 8, seed=3)
    lib = _lib.load()
    words = (300 + 63) // 64
    xs = np.full((4, words), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    es = np.full(4, -123.25)
    rc = lib.asp_sa_anneal_shuffled_trace(ham.plan(), ctypes.c_uint64(1), _lib.ptr(betas), ctypes.c_uint32(8),
                                          ctypes.c_uint32(4), ctypes.c_uint32(0), None, _lib.ptr(xs), _lib.ptr(es),
                                          None)
    assert rc == -3 and "null trace pointer" in _lib.last_error()
    assert np.all(xs == 0xA5A5A5A5A5A5A5A5) and np.all(es == -123.25)
    for call in (sa.anneal_with_traces, sa.anneal_traces):
        with pytest.raises(ValueError):
            call(ham, seed=1, number_sweeps=4, sweep_order="bogus")
    # no sweeps: the single 0 of every chain, and the initial configurations
    xs0, es0, trace0 = sa.anneal_trace_raw(ham, 9, np.zeros(0), 5, 1, None, shuffled=True)
    pxs, pes = sa.anneal_raw(ham, 9, np.zeros(0), 5, 1, None, shuffled=True)
    assert trace0.shape == (5, 1) and np.all(trace0 == 0)
    assert np.array_equal(xs0, pxs) and es0.tobytes() == pes.tobytes()
    # no spins: rows of zeros (written: the buffer starts out non-zero)
    empty = sa.Hamiltonian(scipy.sparse.csr_matrix((0, 0)), np.zeros(0))
    ladder = np.ones(6)
    xe, ee, te = np.zeros((3, 1), np.uint64), np.full(3, 7.5), np.full((3, 7), 99, np.int64)
    _lib.check(lib.asp_sa_anneal_shuffled_trace(empty.plan(), ctypes.c_uint64(9), _lib.ptr(ladder), ctypes.c_uint32(6),
                                                ctypes.c_uint32(3), ctypes.c_uint32(0), None, _lib.ptr(xe),
                                                _lib.ptr(ee), _lib.ptr(te)))
    assert np.all(te == 0) and np.all(ee == 0.0)
