"""Tail sweeps of the colour sweep (asp_sa_set_tail, asp_sa_last_tail) against the CPU
oracle bit for bit: once a sweep flips few spins the closed call of four chains per workgroup keeps a
`todo` bit per position and evaluates only the listed rows, compacted into visits of 64 rows.

Every case forces four chains per group, runs in words (the default at these sizes) and in bytes (a
lowered asp_sa_set_lds_limit), compares configurations, energies, tracked energies and accepted counts
with oracle.sa_anneal and the trace at every sweep with oracle.sa_anneal_trace, and asserts through
asp_sa_last_tail that tail sweeps really ran.

Every reference is computed once per module and frozen."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import oracle

RUN_SEED = 4242
ALWAYS = 2 ** 31 - 1  # a threshold every sweep stays below: tail sweeps from the second sweep on
LAYOUTS = {"words": 2, "bytes": 0}


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _host_info(J, field):
    """The plan's summary (automatic ladder, energy scale, blocks) from the host layout."""
    from annealing_sign_problem_amd import _lib

    n = J.shape[0]
    info = _lib.SaInfo()
    colors = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(
        n, _lib.ptr(np.ascontiguousarray(J.indptr, np.int64)), _lib.ptr(np.ascontiguousarray(J.indices, np.int32)),
        _lib.ptr(np.ascontiguousarray(J.data, np.float64)), _lib.ptr(field), ctypes.byref(info), _lib.ptr(colors),
        _lib.ptr(position)))
    return info


class _Case:
    """A model, a ladder, a range of chains, and the oracle's closed call and trace of them."""

    def __init__(self, J, field, betas=None, sweeps=96, first=0, count=8, x0=None):
        from annealing_sign_problem_amd import annealer as sa

        self.J, self.field = scipy.sparse.csr_matrix(J), np.ascontiguousarray(field, np.float64)
        info = _host_info(self.J, self.field)
        self.S, self.blocks = info.energy_scale_exp, info.num_blocks
        self.auto = (info.beta0_auto, info.beta1_auto)
        self.betas = sa.make_schedule(*self.auto, sweeps) if betas is None else betas(*self.auto)
        self.first, self.count, self.x0 = first, count, x0
        self.final = _freeze(oracle.sa_anneal(self.J, self.field, RUN_SEED, self.betas, count, first, x0, self.S,
                                              num_threads=8))
        self.trace = _freeze(oracle.sa_anneal_trace(self.J, self.field, RUN_SEED, self.betas, count, first, x0,
                                                    self.S, num_threads=8))

    def bytes_limit(self):
        """The LDS of the byte layout's sweep (csrc/sa_sweep.hip, sweep_lds_bytes; SweepLds in csrc/sa_colour.hpp): words do not fit it."""
        nb = self.blocks
        return nb * 64 + 34 * 8 + nb * 8 + 16 + 2 * ((nb + 15) // 16 * 16)


def _run(case, layout, threads, tail):
    """The closed call and its trace variant: (xs, es, tracked, accepted), trace, and what
    asp_sa_last_tail reports after each."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    ham = sa.Hamiltonian(case.J, case.field)
    _lib.check(lib.asp_sa_set_launch(ham.plan(), 4, threads))
    if layout == "bytes":
        _lib.check(lib.asp_sa_set_lds_limit(ham.plan(), ctypes.c_uint64(case.bytes_limit())))
    sa.set_tail(ham, tail)
    xs, es = sa.anneal_raw(ham, RUN_SEED, case.betas, case.count, case.first, case.x0)
    assert lib.asp_sa_last_layout(ham.plan()) == LAYOUTS[layout]
    tracked = np.zeros(case.count, np.int64)
    accepted = np.zeros(case.count, np.uint64)
    _lib.check(lib.asp_sa_last_stats(ham.plan(), case.count, _lib.ptr(tracked), _lib.ptr(accepted)))
    ran_closed = sa.last_tail(ham)
    txs, tes, trace = sa.anneal_trace_raw(ham, RUN_SEED, case.betas, case.count, case.first, case.x0)
    assert lib.asp_sa_last_layout(ham.plan()) == LAYOUTS[layout]
    ran_trace = sa.last_tail(ham)
    ham.release()
    assert ran_closed == ran_trace, "the trace variant ran other tail sweeps than the closed call"
    assert np.array_equal(txs, xs) and tes.tobytes() == es.tobytes()
    return (xs, es, tracked, accepted), trace, ran_closed


def _assert_oracle(case, got, trace, what):
    names = ("configurations", "energies", "tracked energies", "accepted counts")
    for g, w, name in zip(got, case.final, names):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: %s differ from the oracle" % (what, name)
    sweeps = np.nonzero((trace != case.trace[2]).any(axis=0))[0]
    assert sweeps.size == 0, "%s: the trace differs from the oracle's first at sweep %d" % (what, sweeps[0])


def _planted(spins, **kw):
    from annealing_sign_problem_amd import synthetic

    J, h, _ = synthetic.planted_cluster(spins, **kw)
    return J, h


# ---------------------------------------------------------------------------------------------
# Automatic ladder
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ladder_cases():
    return {600: _Case(*_planted(600, mean_degree=6.0)), 10000: _Case(*_planted(10000))}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("spins", [600, 10000])
def test_automatic_ladder(ladder_cases, spins, layout):
    """96 sweeps of the automatic ladder, 8 chains: the automatic threshold enters tail sweeps in every
    group, and the outputs are those without tail sweeps and with thresholds 1 and 2^31 - 1."""
    case = ladder_cases[spins]
    got, trace, (sweeps_min, sweeps_max, entries) = _run(case, layout, 0, -1)
    print("K = %d %s: tail sweeps %d..%d of 96, entries %d" % (spins, layout, sweeps_min, sweeps_max, entries))
    assert sweeps_min > 0 and entries >= 1, "the automatic threshold never entered tail sweeps"
    _assert_oracle(case, got, trace, "automatic threshold")
    for tail in (0, 1, ALWAYS):
        other, other_trace, ran = _run(case, layout, 0, tail)
        if tail == 0:
            assert ran == (0, 0, 0)
        if tail == ALWAYS:
            assert ran == (95, 95, 1)
        for a, b in zip(got, other):
            assert a.tobytes() == b.tobytes(), "threshold %d differs from the automatic one" % tail
        assert np.array_equal(trace, other_trace)


# ---------------------------------------------------------------------------------------------
# Edge shapes
# ---------------------------------------------------------------------------------------------

def _circulant(spins, seed):
    """Spin i coupled to i +- 1, 2, 3 (mod spins) where those exist, random couplings, diagonal and field."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in (1, 2, 3):
        if 2 * d >= spins:  # (i + d and i - d would be one spin, or i itself)
            continue
        i = np.arange(spins)
        w = rng.normal(size=spins)
        rows += [i, (i + d) % spins]
        cols += [(i + d) % spins, i]
        vals += [w, w]
    rows.append(np.arange(spins))
    cols.append(np.arange(spins))
    vals.append(rng.normal(size=spins))
    J = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                                shape=(spins, spins)).tocsr()
    return J, rng.normal(size=spins)


def _hand_built():
    """200 spins: spin 0 a hub of degree 150 (a colour of one row), spins 1..197 a ring (colours of about
    a hundred rows: a whole block and a partial one), spins 198 and 199 isolated (rows of width 0), one
    with a field and one without."""
    rng = np.random.default_rng(5)
    ring = np.arange(1, 198)
    lo = np.concatenate([np.zeros(150, np.int64), ring])
    hi = np.concatenate([np.arange(1, 151), np.roll(ring, -1)])
    w = rng.normal(size=lo.size)
    J = scipy.sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))),
                                shape=(200, 200)).tocsr()
    field = rng.normal(size=200)
    field[199] = 0.0
    return J, field


def _edge_betas(beta0, beta1):
    from annealing_sign_problem_amd import annealer as sa

    # hot sweeps first (every listed row flips and lists its neighbours), then down the ladder
    return np.concatenate([np.full(3, 1e-3 * beta0), sa.make_schedule(beta0, beta1, 13)])


EDGE_SHAPES = ["1", "63", "64", "65", "130", "4097", "hand"]
_edge_cache = {}


def _edge_case(shape):
    if shape not in _edge_cache:
        model = _hand_built() if shape == "hand" else (
            _planted(4097, mean_degree=8.0, seed=3) if shape == "4097" else _circulant(int(shape), int(shape)))
        _edge_cache[shape] = _Case(*model, betas=_edge_betas)
    return _edge_cache[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_every_row_listed(shape, threads, layout):
    """Tail sweeps from the second sweep on, so every row is listed at first: one wavefront scanning
    every block, and more wavefronts than blocks."""
    case = _edge_case(shape)
    got, trace, ran = _run(case, layout, threads, ALWAYS)
    assert ran == (15, 15, 1), "sweeps 1..15 are tail sweeps"
    _assert_oracle(case, got, trace, "%s spins, %d threads" % (shape, threads))


# ---------------------------------------------------------------------------------------------
# Reheat
# ---------------------------------------------------------------------------------------------

def _reheat_betas(beta0, beta1):
    from annealing_sign_problem_amd import annealer as sa

    down = sa.make_schedule(beta0, beta1, 40)
    return np.concatenate([down, down[::-6][1:], down[4:]])  # freeze, reheat over six sweeps, freeze again


@pytest.fixture(scope="module")
def reheat():
    case = _Case(*_planted(600, mean_degree=6.0, seed=11), betas=_reheat_betas)
    assert (np.diff(case.betas) < 0).sum() >= 5
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_reheat_leaves_and_enters_again(reheat, layout):
    got, trace, (sweeps_min, _, entries) = _run(reheat, layout, 0, -1)
    assert entries >= 2 and sweeps_min > 0, "tail sweeps were not entered on both sides of the reheating"
    _assert_oracle(reheat, got, trace, "reheated ladder")


# ---------------------------------------------------------------------------------------------
# Chain ranges
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ranges():
    model = _planted(600, mean_degree=6.0, seed=13)
    return {4: _Case(*model, first=4, count=8), 3: _Case(*model, first=3, count=9)}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_aligned_and_generic_chains(ranges, layout):
    """Chains 4..11 from a launch that starts on replica 4 (the aligned kernel) and from one that starts
    on replica 3 (the generic one)."""
    got = {}
    for first, case in ranges.items():
        got[first], trace, (sweeps_min, _, _) = _run(case, layout, 0, -1)
        assert sweeps_min > 0, "no tail sweeps from replica %d" % first
        _assert_oracle(case, got[first], trace, "from replica %d" % first)
    for a, b in zip(got[4], got[3]):
        assert a.tobytes() == b[1:].tobytes(), "aligned and generic launches differ"


# ---------------------------------------------------------------------------------------------
# Start configuration
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def from_minimum():
    J, h = _planted(600, mean_degree=6.0, seed=17)
    x0, _ = oracle.greedy_solve(scipy.sparse.csr_matrix(J), h)
    return _Case(J, h, betas=lambda beta0, beta1: np.full(24, beta1), x0=np.ascontiguousarray(x0, np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_start_from_the_greedy_minimum(from_minimum, layout):
    """Cold sweeps from a local minimum: tail sweeps from the second sweep on with next to nothing listed."""
    got, trace, ran = _run(from_minimum, layout, 0, -1)
    assert ran == (23, 23, 1)
    _assert_oracle(from_minimum, got, trace, "x0 start")
