"""The visit of the colour sweep outside its k-loop, against the CPU oracle bit
for bit:

* ALIGNMENT — groups of four replicas that start on a multiple of four run the visit that takes
  replica m's random word as word m & 3 of one Philox call; any other first replica runs the generic
  visit, which finds call and word at run time.  The same chains through both, in every layout.
* BOOKKEEPING — the tracked energy adds bit patterns of dE * 2^S + 1.5 * 2^52 and takes the
  constants off once per sweep, modulo 2^64.  One wavefront visits all 45 blocks in a sweep, hot (every
  visit adds to every replica's sum, which wraps from the fourth visit on) and cold, with the
  couplings as planted and scaled by 2^-300 and 2^+300 (energy_scale_exp at both ends).
* EXACT BAND — the middle of the automatic ladder, where a third of the proposals draw and a few of
  those fall between the two bounds of the hardware-exp filter and are decided by the exact exp
  (a host replay of the chains counts both).

Every reference is computed once per module and frozen."""
import numpy as np
import pytest
import scipy.sparse

import oracle

RUN_SEED = 777


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _with_isolated_spins(J, count=3):
    """J with `count` more spins that have an empty row (and field 0: dE = +-0 for them)."""
    n = J.shape[0]
    big = scipy.sparse.csr_matrix(J, copy=True)
    big.resize((n + count, n + count))
    return big, np.zeros(n + count)


def _stats(ham, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(ham.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


# ---------------------------------------------------------------------------------------------
# Alignment
# ---------------------------------------------------------------------------------------------

ALIGNED = (4, 8)   # replica_offset, repetitions: chains 4..11, groups start on a Philox call
GENERIC = (3, 9)   # chains 3..11: every group of four straddles two calls


class _AlignmentCase:
    """A cluster with three isolated spins, 24 sweeps of which the first is at beta = 0, and the
    oracle's chains 3..11 on it."""

    def __init__(self, spins, **cluster):
        from annealing_sign_problem_amd import annealer as sa
        from annealing_sign_problem_amd import synthetic

        J, _, _ = synthetic.planted_cluster(spins, **cluster)
        self.J, self.field = _with_isolated_spins(J)
        ham = sa.Hamiltonian(self.J, self.field)
        info = ham.info()
        ham.release()
        self.S = info.energy_scale_exp
        self.betas = np.concatenate([[0.0], sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 23)])
        offset, reps = GENERIC
        self.oracle = _freeze(oracle.sa_anneal(self.J, self.field, RUN_SEED, self.betas, reps, offset, None,
                                               self.S, num_threads=8))

    def expected(self, first, count):
        lo = first - GENERIC[0]
        return [a[lo:lo + count] for a in self.oracle]


@pytest.fixture(scope="module")
def small():
    case = _AlignmentCase(200, seed=17)
    assert case.J.shape[0] == 203  # not a multiple of 64: some block has dummy lanes
    return case


@pytest.fixture(scope="module")
def large():
    # beyond the capacity of a byte per position: the launcher takes the nibble layout
    return _AlignmentCase(150000, seed=22, mean_degree=6.0)


def _prepare(ham, m, threads, wide):
    from annealing_sign_problem_amd import _lib

    _lib.check(_lib.load().asp_sa_set_wide(ham.plan(), 1 if wide else 0))
    _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), m, threads))


def _closed_call(case, m, threads, wide, layout, first, count):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(case.J, case.field)
    _prepare(ham, m, threads, wide)
    xs, es = sa.anneal_raw(ham, RUN_SEED, case.betas, count, first, None)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == layout
    tracked, accepted = _stats(ham, count)
    ham.release()
    return xs, es, tracked, accepted


def _assert_same(got, want, what):
    names = ("configurations", "energies", "tracked energies", "accepted counts")
    for g, w, name in zip(got, want, names):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: %s differ" % (what, name)


def _check_alignment(case, m, threads, wide, layout):
    aligned = _closed_call(case, m, threads, wide, layout, *ALIGNED)
    generic = _closed_call(case, m, threads, wide, layout, *GENERIC)
    _assert_same(aligned, case.expected(*ALIGNED), "aligned launch against the oracle")
    _assert_same(generic, case.expected(*GENERIC), "generic launch against the oracle")
    _assert_same(aligned, [a[1:] for a in generic], "aligned against generic launch")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["m4_bytes", "m4_words", "m8_bytes"])
def test_aligned_and_generic_visit_agree(small, form):
    """Chains 4..11 from a launch that starts on replica 4 and from one that starts on replica 3."""
    m, wide, layout = {"m4_bytes": (4, False, 0), "m4_words": (4, True, 2), "m8_bytes": (8, False, 0)}[form]
    _check_alignment(small, m, 128, wide, layout)


@pytest.mark.gpu
def test_aligned_and_generic_visit_agree_in_nibbles(large):
    _check_alignment(large, 4, 512, False, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
def test_aligned_and_generic_resumed_handle(small, wide):
    """The same pair through a handle in two segments (k_sa_sweep_resume shares the body)."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    got = {}
    for first, count in (ALIGNED, GENERIC):
        ham = sa.Hamiltonian(small.J, small.field)
        _prepare(ham, 4, 128, wide)
        with sa.Chains(ham, seed=RUN_SEED, repetitions=count, replica_offset=first) as chains:
            for part in (small.betas[:9], small.betas[9:]):
                chains.advance(part, sweep_order="colour")
                assert _lib.load().asp_sa_last_layout(ham.plan()) == (2 if wide else 0)
            xs, es = chains.result()
            state = chains.state()
        ham.release()
        got[first] = (xs, es, state["tracked_best"], state["accepted"])
        _assert_same(got[first], small.expected(first, count), "handle from replica %d against the oracle" % first)
    _assert_same(got[ALIGNED[0]], [a[1:] for a in got[GENERIC[0]]], "aligned against generic handle")


# ---------------------------------------------------------------------------------------------
# Bookkeeping
# ---------------------------------------------------------------------------------------------

BOOK_SPINS, BOOK_CHAINS = 2560, 8
SCALES = {"planted": 0, "tiny": -300, "huge": 300}


class _BookCase:
    def __init__(self, exponent):
        from annealing_sign_problem_amd import annealer as sa
        from annealing_sign_problem_amd import synthetic

        J, h, _ = synthetic.planted_cluster(BOOK_SPINS, seed=29)
        self.J = scipy.sparse.csr_matrix(J * np.ldexp(1.0, exponent))  # exact: a power of two
        self.field = h
        ham = sa.Hamiltonian(self.J, self.field)
        info = ham.info()
        ham.release()
        self.S = info.energy_scale_exp
        # hot: beta = 0 accepts every proposal, a thousandth of the ladder's start nearly every one;
        # then the automatic ladder down to its cold end
        self.betas = np.concatenate([np.zeros(5), np.full(5, 1e-3 * info.beta0_auto),
                                     sa.make_schedule(info.beta0_auto, info.beta1_auto, 14)])
        hot = oracle.sa_anneal(self.J, self.field, RUN_SEED, self.betas[:10], BOOK_CHAINS + 1, 0, None, self.S,
                               num_threads=8)[3]
        assert hot.min() > 0.95 * 10 * BOOK_SPINS, "the hot sweeps do not accept nearly every proposal"
        self.trace = _freeze(oracle.sa_anneal_trace(self.J, self.field, RUN_SEED, self.betas, BOOK_CHAINS + 1, 0,
                                                    None, self.S, num_threads=8))
        self.final = _freeze(oracle.sa_anneal(self.J, self.field, RUN_SEED, self.betas, BOOK_CHAINS + 1, 0, None,
                                              self.S, num_threads=8))


@pytest.fixture(scope="module")
def book_cases():
    cases = {name: _BookCase(exponent) for name, exponent in SCALES.items()}
    # the three scalings put the fixed point at three different places, 600 binary digits apart
    assert cases["tiny"].S - cases["planted"].S == 300 and cases["planted"].S - cases["huge"].S == 300
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, 1], ids=["aligned", "generic"])
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_tracked_energy_of_one_wavefront(book_cases, scale, wide, first):
    """threads = 64: one wavefront visits all 45 blocks, so a lane adds 45 bit patterns per replica
    and sweep.  Traces sweep by sweep, then the best tracked energies and flip counts."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    case = book_cases[scale]
    ham = sa.Hamiltonian(case.J, case.field)
    _prepare(ham, 4, 64, wide)
    xs, es, trace = sa.anneal_trace_raw(ham, RUN_SEED, case.betas, BOOK_CHAINS, first, None)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == (2 if wide else 0)
    tracked, accepted = _stats(ham, BOOK_CHAINS)
    ham.release()
    rows = slice(first, first + BOOK_CHAINS)
    oxs, oes, otrace = (a[rows] for a in case.trace)
    _, _, otracked, oaccepted = (a[rows] for a in case.final)
    assert np.array_equal(trace, otrace), "per-sweep tracked energies differ"
    assert np.array_equal(tracked, otracked) and np.array_equal(accepted, oaccepted)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_descent_on_the_same_instances(book_cases, scale):
    """asp_sa_greedy (the descent instantiation of the body) at the three fixed-point scales."""
    from annealing_sign_problem_amd import annealer as sa

    case = book_cases[scale]
    ham = sa.Hamiltonian(case.J, case.field)
    x, e = sa.greedy_solve(ham)
    ham.release()
    ox, oe = oracle.greedy_solve(case.J, case.field)
    assert np.array_equal(x, ox) and e == oe


# ---------------------------------------------------------------------------------------------
# Exact band
# ---------------------------------------------------------------------------------------------

def _host_info(J, field):
    """The plan's summary (automatic ladder, energy scale) from the host layout: no GPU."""
    import ctypes

    from annealing_sign_problem_amd import _lib

    Jc = scipy.sparse.csr_matrix(J)
    n = Jc.shape[0]
    info = _lib.SaInfo()
    colors = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(
        n, _lib.ptr(np.ascontiguousarray(Jc.indptr, np.int64)), _lib.ptr(np.ascontiguousarray(Jc.indices, np.int32)),
        _lib.ptr(np.ascontiguousarray(Jc.data, np.float64)), _lib.ptr(np.ascontiguousarray(field, np.float64)),
        ctypes.byref(info), _lib.ptr(colors), _lib.ptr(position)))
    return info


@pytest.fixture(scope="module")
def band():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, h, _ = synthetic.planted_cluster(2048, seed=31)
    info = _host_info(J, h)
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, 128)[48:80]
    runs = {first: _freeze(oracle.sa_anneal(J, h, RUN_SEED, betas, 16, first, None, info.energy_scale_exp,
                                            num_threads=8)) for first in (0, 1)}
    return J, h, betas, runs


def _philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays: the four words along a last axis."""
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3)]
    low = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & low, p1 & low, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & low, p0 & low
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & low, (k1 + np.uint64(0xBB67AE85)) & low
    return np.stack([c0, c1, c2, c3], -1)


def _replay(J, h, seed, betas, reps, first):
    """The chains of DESIGN.md §4.2-4.4 colour by colour in numpy (row sums in ascending column
    order; exp through numpy, through the oracle's expneg within 1e-4 of the random number).
    Returns the accepted flips per chain, the proposals, those that need a random number, and those
    whose word lies within 1.7e-5 of expneg * 2^32 — inside the hardware-exp filter's band of 2e-5
    whatever the estimate's error (2.63e-6, sa_device.hpp), so surely decided by the exact exp."""
    n = J.shape[0]
    A = scipy.sparse.csr_matrix(J + J.T)
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    colors = np.asarray(oracle.sa_layout(J)[0])[:n]
    degree = np.diff(A.indptr)
    col = np.zeros((n, degree.max()), np.int64)
    val = np.zeros((n, degree.max()))
    for i in range(n):
        col[i, :degree[i]] = A.indices[A.indptr[i]:A.indptr[i + 1]]
        val[i, :degree[i]] = A.data[A.indptr[i]:A.indptr[i + 1]]
    r = first + np.arange(reps)

    def words(spins, t):
        w = _philox(spins[:, None], t, (r >> 2)[None, :], 0, seed)
        return np.take_along_axis(w, np.broadcast_to((r & 3)[None, :, None], (len(spins), reps, 1)), -1)[..., 0]

    s = np.where(words(np.arange(n), 0xFFFFFFFF) & np.uint64(1), 1.0, -1.0)
    accepted = np.zeros(reps, np.int64)
    proposals = draws = in_band = 0
    for t, beta in enumerate(betas):
        for c in range(colors.max() + 1):
            idx = np.nonzero(colors == c)[0]
            acc = np.zeros((len(idx), reps))
            for k in range(col.shape[1]):
                live = idx[degree[idx] > k]
                acc[degree[idx] > k] += val[live, k][:, None] * s[col[live, k]]
            g = acc + h[idx][:, None]
            de = np.where(s[idx] > 0, -2.0 * g, 2.0 * g)
            x = beta * de
            need = (de > 0) & (x < 23.0)
            word = words(idx, t).astype(np.float64)
            p = np.exp(-np.where(need, x, 0.0))
            u = (word + 0.5) * 2.0 ** -32
            below = u < p
            for a, b in zip(*np.nonzero(need & (np.abs(u - p) <= 1e-4 * p))):
                below[a, b] = u[a, b] < oracle.expneg(float(x[a, b]))
            accept = (de <= 0) | (need & below)
            s[idx] = np.where(accept, -s[idx], s[idx])
            accepted += accept.sum(0)
            proposals += need.size
            draws += int(need.sum())
            in_band += int((need & (np.abs(word + 0.5 - p * 2.0 ** 32) <= 1.7e-5 * p * 2.0 ** 32)).sum())
    return accepted, proposals, draws, in_band


@pytest.mark.parametrize("first", [0, 1], ids=["aligned", "generic"])
def test_middle_of_the_ladder_reaches_the_exact_exp(band, first):
    """(no GPU) What test_middle_of_the_ladder covers, counted on the host: a replay of the same
    chains that flips what the oracle flips finds 37 % of the 1e6 proposals drawing a random word and
    two of them surely inside the filter's band.  (The band is +-2e-5 of expneg * 2^32, so its share
    of the draws is 4e-5 times the mean acceptance probability of a draw — a few, not the dozen
    that 4e-5 of the draws would be.)"""
    J, h, betas, runs = band
    accepted, proposals, draws, in_band = _replay(J, h, RUN_SEED, betas, 16, first)
    assert np.array_equal(accepted, runs[first][3].astype(np.int64)), "the replay is not the oracle's chain"
    assert proposals == 2048 * 16 * 32
    assert 0.3 < draws / proposals < 0.45
    assert in_band >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, 1], ids=["aligned", "generic"])
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
def test_middle_of_the_ladder(band, wide, first):
    """2048 spins x 16 chains x 32 sweeps = 1e6 proposals in the middle of the automatic ladder: 37 %
    draw a random word and at least two fall inside the filter's band, where the exact exp decides
    (counted on the host by test_middle_of_the_ladder_reaches_the_exact_exp)."""
    from annealing_sign_problem_amd import annealer as sa

    J, h, betas, runs = band
    ham = sa.Hamiltonian(J, h)
    _prepare(ham, 4, 256, wide)
    xs, es = sa.anneal_raw(ham, RUN_SEED, betas, 16, first, None)
    tracked, accepted = _stats(ham, 16)
    ham.release()
    oxs, oes, otracked, oaccepted = runs[first]
    assert np.array_equal(xs, oxs), "configurations differ"
    assert es.tobytes() == oes.tobytes()
    assert np.array_equal(tracked, otracked) and np.array_equal(accepted, oaccepted)
