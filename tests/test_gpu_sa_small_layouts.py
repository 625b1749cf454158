"""The packed and HBM spin layouts of the sweeps — four bits per spin, one bit per spin in LDS, 32-bit
words in HBM — at SMALL sizes, where every edge of a kernel is cheap to reach: chosen through the plan's
layout limit (asp_sa_set_lds_limit), observed through asp_sa_last_spin_layout (include/asp.h, DESIGN.md
§4.9, §5.2).  Without the limit these layouts run only on clusters of 1.5e5 spins and more, which the
other modules can afford once or twice each.

Every comparison is bit for bit: np.array_equal on words and integers, energies compared as bytes.  The
references are the CPU oracle (oracle.sa_anneal_shuffled / sa_anneal), the same call at the device's
own limit (the word and byte layouts: compared with the oracle here and in tests/test_gpu_sa.py), and
one-chain handles for the ladder law (tests/test_gpu_tempering.py).

The limits are never computed here: `_scan` bisects the limit with one-sweep calls and reads the layout
that ran.  ASP_SHUFFLED_LEVEL_CAP pins the capacity of the per-sweep level tables for the module — by
default it follows the number of levels of the plan's previous call, and with it the LDS that the
tables take beside the spins, by more than the 16 bytes that separate two layouts of a tiny cluster."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import oracle
from test_gpu_tempering import _chain_betas, _same_state

pytestmark = pytest.mark.gpu

TOO_LARGE = -4
WORDS, BYTES, NIBBLES, BITS, HBM = 2, 0, 6, 1, 3  # asp_sa_last_layout's codes
RANK = {WORDS: 0, BYTES: 1, NIBBLES: 2, BITS: 3, HBM: 4, None: 5}  # (None: the call was refused)
NAMES = {WORDS: "words", BYTES: "bytes", NIBBLES: "nibbles", BITS: "bits", HBM: "hbm", None: "refused"}
LEVEL_CAP = 96  # levels a sweep may have: 2.5 x the mean degree is usual, "mixed" has ~20
REPS, OFFSET, SEED = 5, 5, 2024  # a ragged group of four, from replica offset 5
TINY = (1, 2, 63, 64, 65)


@pytest.fixture(autouse=True)
def _pinned_level_cap(monkeypatch):
    monkeypatch.setenv("ASP_SHUFFLED_LEVEL_CAP", str(LEVEL_CAP))


# ---- the cases, built once ------------------------------------------------------------------------------

def _csr(n, rows, cols, vals):
    m = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def _symmetric(n, lo, hi, w, diagonal=None):
    rows, cols, vals = [lo, hi], [hi, lo], [w, w]
    if diagonal is not None:
        rows.append(np.arange(n)), cols.append(np.arange(n)), vals.append(diagonal)
    return _csr(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


N_PLANTED, N_ISOLATED, HUB, HUB_DEGREE = 2000, 131, 7, 64


def _mixed():
    """A planted cluster of 2000 spins at mean degree 6, one hub row of more than 60 couplings (the
    registers hold 48: the rest streams), and 131 isolated spins behind it — 66 with a field, 65 with
    none (dE = 0: always accepted).  K = 2131: odd, K % 8 = 3."""
    from annealing_sign_problem_amd import synthetic

    rng = np.random.default_rng(17)
    planted, _, _ = synthetic.planted_cluster(N_PLANTED, seed=5, mean_degree=6.0)
    coo = planted.tocoo()
    scale = float(np.median(np.abs(coo.data[coo.row != coo.col])))
    known = set(planted[HUB].indices.tolist()) | {HUB}
    fresh = np.array([j for j in rng.permutation(N_PLANTED) if j not in known][:HUB_DEGREE])
    w = rng.normal(size=HUB_DEGREE) * scale
    K = N_PLANTED + N_ISOLATED
    J = _csr(K, np.concatenate([coo.row, np.full(HUB_DEGREE, HUB), fresh]),
             np.concatenate([coo.col, fresh, np.full(HUB_DEGREE, HUB)]), np.concatenate([coo.data, w, w]))
    h = rng.normal(size=K) * scale * 0.5
    h[N_PLANTED + (N_ISOLATED + 1) // 2:] = 0.0
    degree = np.diff((J - scipy.sparse.diags(J.diagonal())).tocsr().indptr)
    assert K % 2 == 1 and K % 8 != 0 and degree[HUB] > 60 and np.all(degree[N_PLANTED:] == 0)
    assert np.count_nonzero(h[N_PLANTED:]) == 66
    return J, h


def _leaves():
    """37 paths of 9 spins: every row has one or two couplings, every block is one quad wide."""
    rng = np.random.default_rng(23)
    K = 333
    lo = np.array([i for i in range(K - 1) if (i + 1) % 9 != 0])
    return _symmetric(K, lo, lo + 1, rng.normal(size=lo.shape[0])), rng.normal(size=K) * 0.3


def _field_only():
    """A diagonal J and fields: one level, one colour, no couplings."""
    rng = np.random.default_rng(29)
    K = 200
    return _csr(K, np.arange(K), np.arange(K), rng.normal(size=K)), rng.normal(size=K)


def _tiny(K):
    rng = np.random.default_rng(100 + K)
    if K == 1:
        return scipy.sparse.csr_matrix(np.array([[0.5]])), np.array([0.3])
    if K == 2:
        return _symmetric(2, np.array([0]), np.array([1]), np.array([0.75]), np.array([0.25, -0.5])), np.array([0.3, -0.2])
    ring = np.arange(K)
    a, b = rng.integers(0, K, size=(2, 24))
    keep = a != b
    lo = np.concatenate([ring, np.minimum(a, b)[keep]])
    hi = np.concatenate([(ring + 1) % K, np.maximum(a, b)[keep]])
    return _symmetric(K, lo, hi, rng.normal(size=lo.shape[0]), rng.normal(size=K) * 0.1), rng.normal(size=K) * 0.2


BUILDERS = {"mixed": _mixed, "leaves": _leaves, "field_only": _field_only}
BUILDERS.update({"k%d" % K: (lambda K=K: _tiny(K)) for K in TINY})
SWEEPS = {"mixed": 24}  # (the others: 16)
_CASES, _ORACLE, _SCANS = {}, {}, {}


class Case:
    def __init__(self, name):
        from annealing_sign_problem_amd import annealer as sa

        self.name = name
        self.J, self.h = BUILDERS[name]()
        self.K = self.J.shape[0]
        self.ham = sa.Hamiltonian(self.J, self.h)
        self.info = self.ham.info()
        sweeps = SWEEPS.get(name, 16)
        betas = sa.make_schedule(max(self.info.beta0_auto, 1e-3), min(max(self.info.beta1_auto, 1.0), 1e6), sweeps)
        betas[sweeps // 2] = 0.0  # one sweep in the middle that accepts everything
        betas[-3:] = 1e12         # and an end that accepts nothing uphill
        self.betas = betas
        self.x0 = sa.signs_to_bits(np.where(np.random.default_rng(len(name)).random(self.K) < 0.5, 1.0, -1.0))
        for a in (self.betas, self.x0, self.h):
            a.setflags(write=False)

    def fresh(self):
        """Another plan of the same problem (the batched calls refuse one plan twice; settings do not leak)."""
        from annealing_sign_problem_amd import annealer as sa

        return sa.Hamiltonian(self.J, self.h)


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _oracle(name, shuffled, with_x0, betas=None):
    """(xs, es, tracked, accepted) of the case's REPS chains from OFFSET: computed once, read-only."""
    key = (name, shuffled, with_x0, None if betas is None else betas.tobytes())
    if key not in _ORACLE:
        c = _case(name)
        run = oracle.sa_anneal_shuffled if shuffled else oracle.sa_anneal
        out = run(c.J, c.h, SEED, c.betas if betas is None else betas, REPS, OFFSET, c.x0 if with_x0 else None,
                  c.info.energy_scale_exp, num_threads=4)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


# ---- the plan's settings and reports ----------------------------------------------------------------------

def _lib():
    from annealing_sign_problem_amd import _lib as lib_module

    return lib_module


def _set_limit(ham, limit):
    _lib().check(_lib().load().asp_sa_set_lds_limit(ham.plan(), ctypes.c_uint64(int(limit))))


def _set_shuffled_launch(ham, m, waves=0):
    _lib().check(_lib().load().asp_sa_set_shuffled_launch(ham.plan(), m, waves))


def _set_launch(ham, m, threads=0):
    _lib().check(_lib().load().asp_sa_set_launch(ham.plan(), m, threads))


def _set_packed(ham, packed):
    _lib().check(_lib().load().asp_sa_set_packed(ham.plan(), packed))


def _spin_layout(ham):
    return _lib().load().asp_sa_last_spin_layout(ham.plan())


def _last_m(ham):
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib().check(_lib().load().asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return m.value


def _stats(ham, count):
    tracked, accepted = np.zeros(count, np.int64), np.zeros(count, np.uint64)
    _lib().check(_lib().load().asp_sa_last_stats(ham.plan(), count, _lib().ptr(tracked), _lib().ptr(accepted)))
    return tracked, accepted


def _same_as_oracle(got, stats, want, label):
    xs, es = got
    oxs, oes, otracked, oaccepted = want
    assert np.array_equal(xs, oxs), label + ": configurations"
    assert es.tobytes() == oes.tobytes(), label + ": energies"
    assert np.array_equal(stats[0], otracked), label + ": tracked energies"
    assert np.array_equal(stats[1], oaccepted), label + ": accepted counts"


# ---- finding the limits -------------------------------------------------------------------------------------

def _scan(ham, chains, shuffled=True):
    """Which spin layout one sweep of `chains` chains runs in at every limit: the boundaries by bisection
    between a limit of one byte and the device's, every probe a real call.  Returns the probes in
    DESCENDING limit, [(limit, layout or None when the call was refused with ASP_ERR_TOO_LARGE, chains per
    workgroup)], and per layout seen the middle of the limits that run it."""
    from annealing_sign_problem_amd import annealer as sa

    probes = {}
    one_sweep = np.array([1.0])

    def probe(limit):
        if limit not in probes:
            _set_limit(ham, limit)
            try:
                sa.anneal_raw(ham, 1, one_sweep, chains, 0, None, shuffled=shuffled)
                probes[limit] = (_spin_layout(ham), _last_m(ham))
            except _lib().AspError as error:
                assert error.code == TOO_LARGE, error
                probes[limit] = (None, 0)
        return RANK[probes[limit][0]]

    top = 1 << 20  # (above the device's: clamped to it)
    assert probe(top) == RANK[WORDS]
    bottom_rank = probe(1)
    first = {0: top}  # per rank r > 0: the largest limit that runs rank r or a later one
    for r in range(1, bottom_rank + 1):
        lo, hi = 1, top  # rank(lo) >= r > rank(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if probe(mid) >= r:
                lo = mid
            else:
                hi = mid
        first[r] = lo
    _set_limit(ham, 0)
    ordered = [(limit,) + probes[limit] for limit in sorted(probes, reverse=True)]
    ranks = [RANK[layout] for _, layout, _ in ordered]
    assert ranks == sorted(ranks), "a smaller limit never runs an earlier layout"
    middle = {}
    for layout, r in RANK.items():
        if layout is None or r > bottom_rank or r not in ranks:
            continue
        smallest = first[r + 1] + 1 if r + 1 in first else 1
        middle[layout] = (smallest + min(first[r], top)) // 2 if r else 0
    return ordered, middle


def _limits(name):
    """The limit that runs the case's shuffled sweeps in each layout (one chain per workgroup; nibbles need
    the same LDS whatever the chains per workgroup, and every test asserts the layout that ran)."""
    if name not in _SCANS:
        _SCANS[name] = _scan(_case(name).ham, 1)
    return _SCANS[name][1]


def _distinct(ordered):
    seen = []
    for _, layout, m in ordered:
        if not seen or seen[-1][0] != layout:
            seen.append((layout, m))
    return seen


def test_scan_reaches_every_layout_on_two_thousand_spins():
    """The scan is the first test.  With one chain per workgroup "mixed" runs, from the device's limit
    downwards, in words, bytes, nibbles, bits, HBM and is then refused; with four chains per workgroup in
    words, bytes and nibbles, and then the launcher's existing cut to one chain takes over (bits, HBM, the
    refusal).  A refusal leaves the error code ASP_ERR_TOO_LARGE (asserted by the probe)."""
    c = _case("mixed")
    _set_shuffled_launch(c.ham, 1)
    ordered, middle = _scan(c.ham, 1)
    _SCANS["mixed"] = (ordered, middle)
    print("one chain per workgroup:", [(limit, NAMES[layout]) for limit, layout, _ in ordered])
    assert [layout for layout, _ in _distinct(ordered)] == [WORDS, BYTES, NIBBLES, BITS, HBM, None]
    assert set(middle) == {WORDS, BYTES, NIBBLES, BITS, HBM}
    _set_shuffled_launch(c.ham, 4)
    four, _ = _scan(c.ham, 4)
    _set_shuffled_launch(c.ham, 0)
    print("four chains per workgroup:", [(limit, NAMES[layout], m) for limit, layout, m in four])
    assert _distinct(four) == [(WORDS, 4), (BYTES, 4), (NIBBLES, 4), (BITS, 1), (HBM, 1), (None, 0)]
    # the limit chooses, it does not compute: the same limits with either geometry
    bounds = lambda probes, layout: [limit for limit, seen, _ in probes if seen == layout]
    for layout in (NIBBLES, BITS, HBM):
        assert min(bounds(ordered, layout)) == min(bounds(four, layout)), NAMES[layout]


@pytest.mark.parametrize("K", [1, 2])
def test_scan_of_one_and_two_spins(K):
    """One or two spins take 16 bytes of LDS as words, bytes, nibbles or bits alike (the spins are padded
    to 16 bytes), so the launcher never prefers a packed layout to words there: the limit reaches words,
    HBM and the refusal, and the closed-call test below runs these two sizes in HBM only."""
    c = _case("k%d" % K)
    ordered, middle = _scan(c.ham, 1)
    assert [layout for layout, _ in _distinct(ordered)] == [WORDS, HBM, None]
    assert set(middle) == {WORDS, HBM}


# ---- the shuffled order, closed call ------------------------------------------------------------------------

FORMS = {"nibbles-1": (NIBBLES, 1), "nibbles-2": (NIBBLES, 2), "nibbles-4": (NIBBLES, 4), "bits": (BITS, 1),
         "hbm": (HBM, 1)}
CLOSED = [(form, name) for form in FORMS for name in BUILDERS if form == "hbm" or name not in ("k1", "k2")]


def _closed_shuffled(c, layout, m, waves, with_x0):
    from annealing_sign_problem_amd import annealer as sa

    _set_limit(c.ham, _limits(c.name)[layout])
    _set_shuffled_launch(c.ham, m, waves)
    try:
        got = sa.anneal_raw(c.ham, SEED, c.betas, REPS, OFFSET, c.x0 if with_x0 else None, shuffled=True)
        return got, _stats(c.ham, REPS), _spin_layout(c.ham), _last_m(c.ham)
    finally:
        _set_shuffled_launch(c.ham, 0, 0)
        _set_limit(c.ham, 0)


@pytest.mark.parametrize("form,name", CLOSED)
def test_shuffled_closed_call(form, name):
    """Five chains from replica offset 5, from a random start and from a shared x0, in every case and
    every packed or HBM form: words, energies, tracked energies and accepted counts are the oracle's."""
    layout, m = FORMS[form]
    c = _case(name)
    for with_x0 in (False, True):
        got, stats, ran, ran_m = _closed_shuffled(c, layout, m, 0, with_x0)
        assert (ran, ran_m) == (layout, m), (NAMES[ran], ran_m)
        _same_as_oracle(got, stats, _oracle(name, True, with_x0), "%s %s x0=%s" % (form, name, with_x0))


def test_mixed_really_has_a_block_of_isolated_spins():
    """How we know that "mixed" visits a block without couplings (held_quads == 0 in the sweep kernel):
    an isolated spin has no earlier neighbour, so all 131 are in level 0 of every sweep — checked here
    with the host's restatement of the order, asp_sa_shuffled_order_host —, the order kernel sorts a
    level by descending row length (its step 5), which puts the rows without couplings last, and a block
    is 64 consecutive positions of a level: the last block of level 0 holds at most 64 spins, all of them
    among those 131.  The fill report agrees: fewer coupling slots are used than the blocks have."""
    c = _case("mixed")
    lib = _lib().load()
    indptr, indices = c.J.indptr.astype(np.int64), c.J.indices.astype(np.int32)
    data = np.ascontiguousarray(c.J.data, dtype=np.float64)
    for sweep in (0, 11, 23):
        order, level = np.zeros(c.K, np.uint32), np.zeros(c.K, np.uint32)
        levels = ctypes.c_uint32(0)
        _lib().check(lib.asp_sa_shuffled_order_host(ctypes.c_uint64(c.K), _lib().ptr(indptr), _lib().ptr(indices),
                                                    _lib().ptr(data), _lib().ptr(np.ascontiguousarray(c.h)),
                                                    ctypes.c_uint64(SEED), ctypes.c_uint32(sweep), _lib().ptr(order),
                                                    _lib().ptr(level), ctypes.byref(levels)))
        level_of_spin = np.zeros(c.K, np.uint32)
        level_of_spin[order] = level
        assert np.all(level_of_spin[N_PLANTED:] == 0) and levels.value > 1
        assert np.count_nonzero(level == 0) > N_ISOLATED  # ... behind rows that do have couplings
    _closed_shuffled(c, HBM, 1, 0, False)
    lane, row = ctypes.c_double(0), ctypes.c_double(0)
    _lib().check(lib.asp_sa_last_shuffled_fill(c.ham.plan(), ctypes.byref(lane), ctypes.byref(row)))
    assert 0.0 < lane.value < 1.0 and 0.0 < row.value < 1.0


@pytest.mark.parametrize("waves", [1, 3, 8])
@pytest.mark.parametrize("form", list(FORMS))
def test_shuffled_closed_call_wavefronts(form, waves):
    """One, three and eight wavefronts per workgroup on "mixed": a wavefront alone walks every block of a
    level, eight mostly find none — the oracle's chains either way."""
    layout, m = FORMS[form]
    got, stats, ran, ran_m = _closed_shuffled(_case("mixed"), layout, m, waves, True)
    assert (ran, ran_m) == (layout, m)
    _same_as_oracle(got, stats, _oracle("mixed", True, True), "%s, %d wavefronts" % (form, waves))


# ---- traces ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [NIBBLES, BITS, HBM], ids=lambda code: NAMES[code])
def test_shuffled_trace_rows(layout):
    """The rows of asp_sa_anneal_shuffled_trace are those of the same call at the device's limit, the
    traced call runs in the untraced call's layout, and a row ends in the oracle's tracked energy."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("mixed")
    _set_limit(c.ham, 0)
    xs0, es0, rows0 = sa.anneal_trace_raw(c.ham, SEED, c.betas, REPS, OFFSET, c.x0, shuffled=True)
    assert _spin_layout(c.ham) in (WORDS, BYTES)
    _set_limit(c.ham, _limits("mixed")[layout])
    try:
        sa.anneal_raw(c.ham, SEED, c.betas, REPS, OFFSET, c.x0, shuffled=True)
        untraced = (_spin_layout(c.ham), _last_m(c.ham))
        xs, es, rows = sa.anneal_trace_raw(c.ham, SEED, c.betas, REPS, OFFSET, c.x0, shuffled=True)
        assert (_spin_layout(c.ham), _last_m(c.ham)) == untraced and untraced[0] == layout
    finally:
        _set_limit(c.ham, 0)
    assert np.array_equal(rows, rows0) and np.array_equal(xs, xs0) and es.tobytes() == es0.tobytes()
    oxs, oes, otracked, _ = _oracle("mixed", True, True)
    assert np.array_equal(rows.min(axis=1), otracked) and np.all(rows[:, 0] == 0)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()


# ---- handles ----------------------------------------------------------------------------------------------------

SEGMENTS = (0, 1, 7, 16, 1, 7)                       # 32 sweeps
SEGMENT_LAYOUTS = (WORDS, HBM, NIBBLES, BITS, HBM, HBM, BYTES)  # the limit before each segment (the third HBM: below)


def _handle_schedule(c):
    from annealing_sign_problem_amd import annealer as sa

    total = sum(SEGMENTS) + 7
    betas = sa.make_schedule(max(c.info.beta0_auto, 1e-3), min(max(c.info.beta1_auto, 1.0), 1e6), total)
    betas[total // 2] = 0.0
    betas[-3:] = 1e12
    return betas


def _run_handle(c, orders, limited):
    """One handle over the whole schedule: segments of 0, 1, 7, 16, 1 and 7 sweeps and a last one of 7, the
    limit changed before each (words, HBM, nibbles, bits, HBM, HBM, bytes) or left at the device's.  The
    state is exported and imported into a fresh handle between the two consecutive HBM segments."""
    from annealing_sign_problem_amd import annealer as sa

    betas = _handle_schedule(c)
    limits = {"shuffled": _limits("mixed"), "colour": _colour_limits_of("mixed")}  # (each order has its own)
    lengths = SEGMENTS + (7,)
    ran = []
    chains = sa.Chains(c.ham, seed=SEED, repetitions=REPS, x0=None, replica_offset=OFFSET)
    try:
        done = 0
        for k, (n, layout) in enumerate(zip(lengths, SEGMENT_LAYOUTS)):
            _set_limit(c.ham, limits[orders[k]][layout] if limited else 0)
            chains.advance(betas[done:done + n], sweep_order=orders[k])
            if n:
                ran.append((orders[k], _spin_layout(c.ham)))
            done += n
            if k == 4:  # in the HBM layout: a checkpoint, and the continuation on another handle
                state = chains.state()
                chains.close()
                chains = sa.Chains(c.ham, seed=SEED, repetitions=REPS, x0=None, replica_offset=OFFSET)
                chains.load_state(state)
        return chains.result(), chains.state(), ran
    finally:
        chains.close()
        _set_limit(c.ham, 0)


@pytest.mark.parametrize("order", ["shuffled", "colour"])
def test_handle_through_every_layout_is_the_closed_call(order):
    """The limit changes under a live handle between segments; the end is the oracle's closed call for the
    whole schedule.  Shuffled: the third and the two HBM segments load a handle's chains as words
    (k_chains_state_in<uint32_t>), resume on them and store them back."""
    c = _case("mixed")
    (xs, es), state, ran = _run_handle(c, [order] * 7, True)
    want = [WORDS, HBM, NIBBLES, BITS, HBM, HBM, BYTES][1:]
    if order == "colour":
        # (the colour order takes nibbles with four chains per workgroup only, and five chains run one per
        # workgroup: from bytes it goes to bits)
        assert [layout for _, layout in ran] == [HBM, BITS, BITS, HBM, HBM, BYTES]
    else:
        assert [layout for _, layout in ran] == want
    oxs, oes, otracked, oaccepted = _oracle("mixed", order == "shuffled", False, _handle_schedule(c))
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    assert np.array_equal(state["tracked_best"], otracked) and np.array_equal(state["accepted"], oaccepted)
    assert int(state["sweeps_done"]) == sum(SEGMENTS) + 7


def test_handle_alternating_orders_through_every_layout():
    """The sweep order alternates between the segments while the limit changes: the handle ends where
    the same segments end at the device's limit (no closed call mixes the orders)."""
    c = _case("mixed")
    orders = ["shuffled", "colour", "shuffled", "colour", "shuffled", "shuffled", "colour"]
    (xs, es), state, ran = _run_handle(c, orders, True)
    assert ran == [("colour", HBM), ("shuffled", NIBBLES), ("colour", BITS), ("shuffled", HBM), ("shuffled", HBM),
                   ("colour", BYTES)]
    (xs0, es0), state0, ran0 = _run_handle(c, orders, False)
    assert all(layout in (WORDS, BYTES) for _, layout in ran0)
    assert np.array_equal(xs, xs0) and es.tobytes() == es0.tobytes()
    _same_state(state, state0)


def test_refused_segment_leaves_the_handle_alone():
    """A limit that not even the HBM layout's tables fit: ASP_ERR_TOO_LARGE before anything is launched —
    the handle is where it was, and goes on to the oracle's closed call once the limit allows a layout."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("leaves")
    limits = _limits("leaves")
    with sa.Chains(c.ham, seed=SEED, repetitions=REPS, x0=c.x0, replica_offset=OFFSET) as chains:
        try:
            _set_limit(c.ham, limits[BITS])
            chains.advance(c.betas[:3], sweep_order="shuffled")
            before = chains.state()
            _set_limit(c.ham, 1)
            with pytest.raises(_lib().AspError) as refused:
                chains.advance(c.betas[3:], sweep_order="shuffled")
            assert refused.value.code == TOO_LARGE
            _same_state(chains.state(), before)
            _set_limit(c.ham, limits[HBM])
            chains.advance(c.betas[3:], sweep_order="shuffled")
            assert _spin_layout(c.ham) == HBM
            (xs, es), state = chains.result(), chains.state()
        finally:
            _set_limit(c.ham, 0)
    oxs, oes, otracked, oaccepted = _oracle("leaves", True, True)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    assert np.array_equal(state["tracked_best"], otracked) and np.array_equal(state["accepted"], oaccepted)


def test_clone_copies_the_limit():
    """asp_sa_plan_clone (Hamiltonian.reweighted) takes the limit with the other launch settings; the two
    plans then keep their own."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("k65")
    ham = c.fresh()
    _set_limit(ham, _limits("k65")[NIBBLES])
    twin = ham.reweighted(ham.exchange.data)
    _set_limit(ham, 0)
    want = _oracle("k65", True, False)
    got = sa.anneal_raw(twin, SEED, c.betas, REPS, OFFSET, None, shuffled=True)
    assert _spin_layout(twin) == NIBBLES
    _same_as_oracle(got, _stats(twin, REPS), want, "clone")
    got = sa.anneal_raw(ham, SEED, c.betas, REPS, OFFSET, None, shuffled=True)
    assert _spin_layout(ham) == WORDS
    _same_as_oracle(got, _stats(ham, REPS), want, "original")


# ---- ladder segments and exchange ---------------------------------------------------------------------------------

N1, N2 = 7, 5


@pytest.mark.parametrize("layout", [NIBBLES, BITS, HBM], ids=lambda code: NAMES[code])
def test_ladder_segment_and_exchange(layout):
    """The ladder law (include/asp.h) in each layout: after a ladder segment chain r is where a one-chain
    handle at the constant beta[r] is (and where the oracle's chain is); an exchange and a second ladder
    segment, traced, then equal the same steps at the device's limit."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("mixed")
    betas = _chain_betas(c.info, REPS)
    x0 = np.stack([np.roll(c.x0, r) for r in range(REPS)])

    def run(limit):
        _set_limit(c.ham, limit)
        try:
            with sa.Chains(c.ham, seed=SEED, repetitions=REPS, x0=x0, replica_offset=OFFSET) as chains:
                trace1 = chains.advance_ladder(betas, N1, sweep_order="shuffled", trace=True)
                ran = _spin_layout(c.ham)
                state1 = chains.state()
                swapped = chains.exchange(betas, 0, 3)
                trace2 = chains.advance_ladder(betas, N2, sweep_order="shuffled", trace=True)
                return ran, trace1, state1, swapped, trace2, chains.state(), chains.result()
        finally:
            _set_limit(c.ham, 0)

    ran, trace1, state1, swapped, trace2, state2, (xs, es) = run(_limits("mixed")[layout])
    assert ran == layout
    for r in range(REPS):
        constant = np.full(N1, betas[r])
        with sa.Chains(c.ham, seed=SEED, repetitions=1, x0=x0[r], replica_offset=OFFSET + r) as alone:
            row = alone.advance(constant, sweep_order="shuffled", trace=True)
            _same_state(state1, alone.state(), rows=slice(r, r + 1))
        assert np.array_equal(trace1[r], row[0])
        _, _, otracked, oaccepted = oracle.sa_anneal_shuffled(c.J, c.h, SEED, constant, 1, OFFSET + r, x0[r],
                                                              c.info.energy_scale_exp)
        assert state1["tracked_best"][r] == otracked[0] and state1["accepted"][r] == oaccepted[0]
    ran0, trace10, state10, swapped0, trace20, state20, (xs0, es0) = run(0)
    assert ran0 in (WORDS, BYTES)
    assert np.array_equal(swapped[0], swapped0[0]) and swapped[1].tobytes() == swapped0[1].tobytes()
    assert swapped[2] == swapped0[2]
    assert np.array_equal(trace2, trace20) and np.array_equal(xs, xs0) and es.tobytes() == es0.tobytes()
    _same_state(state2, state20)


# ---- the batched calls ----------------------------------------------------------------------------------------------

BATCH = (("mixed", HBM), ("leaves", HBM), ("field_only", NIBBLES), ("k65", BITS), ("k64", WORDS), ("k63", NIBBLES))


def _batch_plans():
    plans = []
    for name, layout in BATCH:
        c = _case(name)
        ham = c.fresh()
        _set_limit(ham, _limits(name)[layout])
        plans.append((c, ham, layout))
    return plans


def test_shuffled_batches_over_limited_plans():
    """asp_sa_chains_advance_batch and the shuffled asp_sa_anneal_batch over plans limited to HBM (two of
    them: the word-typed state tables of the shared launches hold two problems), nibbles, bits and words:
    every item is its own single call at the device's limit, and "mixed" the oracle's chains."""
    from annealing_sign_problem_amd import annealer as sa

    plans = _batch_plans()
    T = 16
    schedules = [c.betas[-T:] if c.name == "mixed" else c.betas for c, _, _ in plans]
    singles = [sa.anneal_raw(c.ham, SEED + i, schedules[i], REPS, OFFSET, None, shuffled=True)
               for i, (c, _, _) in enumerate(plans)]
    # the closed batch
    batch = sa.anneal_batch_raw([ham for _, ham, _ in plans], [SEED + i for i in range(len(plans))], schedules,
                                [REPS] * len(plans), [OFFSET] * len(plans), shuffled=True)
    for (c, ham, layout), (bx, be), (sx, se) in zip(plans, batch, singles):
        assert _spin_layout(ham) == layout, (c.name, NAMES[_spin_layout(ham)])
        assert np.array_equal(bx, sx) and be.tobytes() == se.tobytes(), c.name
    # the handles, in two segments (the second one resumes every layout from a handle)
    handles = [sa.Chains(ham, seed=SEED + i, repetitions=REPS, replica_offset=OFFSET)
               for i, (_, ham, _) in enumerate(plans)]
    try:
        sa.advance_chains(handles, [s[:5] for s in schedules], "shuffled")
        for (c, ham, layout) in plans:
            assert _spin_layout(ham) == layout, c.name
        sa.advance_chains(handles, [s[5:] for s in schedules], "shuffled")
        for (c, ham, layout), handle, (sx, se) in zip(plans, handles, singles):
            assert _spin_layout(ham) == layout, c.name
            hx, he = handle.result()
            assert np.array_equal(hx, sx) and he.tobytes() == se.tobytes(), c.name
        state = handles[0].state()
    finally:
        for handle in handles:
            handle.close()
    oxs, oes, otracked, oaccepted = _oracle("mixed", True, False, schedules[0])
    assert np.array_equal(singles[0][0], oxs) and singles[0][1].tobytes() == oes.tobytes()
    assert np.array_equal(state["tracked_best"], otracked) and np.array_equal(state["accepted"], oaccepted)


# ---- the colour order -------------------------------------------------------------------------------------------------

def _colour_limits(ham):
    """The colour order's limits with four chains per workgroup (asp_sa_set_launch): its HBM layout keeps
    nothing but a few counters in LDS and fits any limit, so nothing is refused."""
    _set_launch(ham, 4)
    ordered, middle = _scan(ham, 8, shuffled=False)
    assert _distinct(ordered) == [(WORDS, 4), (BYTES, 4), (NIBBLES, 4), (BITS, 1), (HBM, 1)]
    return middle


_COLOUR_SCANS = {}


def _colour_limits_of(name):
    """The colour order's limits of a case, scanned once on a plan of its own."""
    if name not in _COLOUR_SCANS:
        _COLOUR_SCANS[name] = _colour_limits(_case(name).fresh())
    return _COLOUR_SCANS[name]


def test_colour_order_layouts_through_the_limit():
    """Nibbles at 2131 spins as the closed call; bits and HBM through the limit are the runs forced with
    asp_sa_set_packed; all of them the oracle's chains."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("mixed")
    ham = c.fresh()
    limits = _colour_limits(ham)
    want = _oracle("mixed", False, True)
    for layout in (NIBBLES, BITS, HBM):
        _set_limit(ham, limits[layout])
        got = sa.anneal_raw(ham, SEED, c.betas, REPS, OFFSET, c.x0)
        assert _spin_layout(ham) == layout and _lib().load().asp_sa_last_layout(ham.plan()) == layout
        _same_as_oracle(got, _stats(ham, REPS), want, "colour " + NAMES[layout])
        _set_limit(ham, 0)
        if layout == NIBBLES:
            continue
        _set_packed(ham, 1 if layout == BITS else 2)
        forced = sa.anneal_raw(ham, SEED, c.betas, REPS, OFFSET, c.x0)
        assert _spin_layout(ham) == layout
        forced_stats = _stats(ham, REPS)
        _set_packed(ham, 0)
        assert np.array_equal(got[0], forced[0]) and got[1].tobytes() == forced[1].tobytes()
        _same_as_oracle(forced, forced_stats, want, "colour forced " + NAMES[layout])


def _nibble_plan(c):
    """A plan of its own with four chains per group forced and the limit that runs nibbles: five chains
    from offset 5 are a full group and a ragged one whose first replica is no multiple of four."""
    ham = c.fresh()
    _set_launch(ham, 4)
    _set_limit(ham, _colour_limits_of(c.name)[NIBBLES])
    return ham


@pytest.mark.parametrize("name", ["mixed", "k65"])
def test_colour_handle_segments_in_nibbles(name):
    """The segment kernel in the nibble layout (four chains per group): the case's schedule in segments of
    5, 1, 0 and the rest of its sweeps, untraced; every segment that runs reports nibbles and groups of
    four, and the handle ends where the oracle's closed colour-order call for the whole schedule ends."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case(name)
    ham = _nibble_plan(c)
    lengths = (5, 1, 0, len(c.betas) - 6)
    with sa.Chains(ham, seed=SEED, repetitions=REPS, x0=None, replica_offset=OFFSET) as chains:
        done = 0
        for n in lengths:
            assert chains.advance(c.betas[done:done + n], sweep_order="colour") is None
            if n:
                assert (_spin_layout(ham), _last_m(ham)) == (NIBBLES, 4), (n, NAMES[_spin_layout(ham)])
            done += n
        (xs, es), state = chains.result(), chains.state()
    oxs, oes, otracked, oaccepted = _oracle(name, False, False)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    assert np.array_equal(state["tracked_best"], otracked) and np.array_equal(state["accepted"], oaccepted)
    assert int(state["sweeps_done"]) == len(c.betas)


@pytest.mark.parametrize("name", ["mixed", "k65"])
def test_colour_ladder_segments_in_nibbles(name):
    """The ladder-segment kernel in the nibble layout: after a ladder segment chain r is where a one-chain
    handle at the constant beta[r] and replica offset OFFSET + r is; an exchange and a second ladder segment
    then equal the same steps at the device's limit, where four chains per group run the word layout."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case(name)
    ham = _nibble_plan(c)
    nibble_limit = _colour_limits_of(name)[NIBBLES]
    betas = _chain_betas(c.info, REPS)
    rng = np.random.default_rng(41)
    x0 = np.stack([sa.signs_to_bits(np.where(rng.random(c.K) < 0.5, 1.0, -1.0)) for _ in range(REPS)])

    def run(limit):
        _set_limit(ham, limit)
        with sa.Chains(ham, seed=SEED, repetitions=REPS, x0=x0, replica_offset=OFFSET) as chains:
            assert chains.advance_ladder(betas, N1, sweep_order="colour") is None
            ran = [(_spin_layout(ham), _last_m(ham))]
            state1 = chains.state()
            swapped = chains.exchange(betas, 0, 3)
            chains.advance_ladder(betas, N2, sweep_order="colour")
            ran.append((_spin_layout(ham), _last_m(ham)))
            return ran, state1, swapped, chains.state(), chains.result()

    ran, state1, swapped, state2, (xs, es) = run(nibble_limit)
    assert ran == [(NIBBLES, 4)] * 2, ran
    for r in range(REPS):  # (on the case's own plan: the device's limit, no forced group size)
        with sa.Chains(c.ham, seed=SEED, repetitions=1, x0=x0[r], replica_offset=OFFSET + r) as alone:
            alone.advance(np.full(N1, betas[r]), sweep_order="colour")
            _same_state(state1, alone.state(), rows=slice(r, r + 1))
    ran0, state10, swapped0, state20, (xs0, es0) = run(0)
    assert ran0 == [(WORDS, 4)] * 2, ran0
    _same_state(state1, state10)
    assert np.array_equal(swapped[0], swapped0[0]) and swapped[1].tobytes() == swapped0[1].tobytes()
    assert swapped[2] == swapped0[2]
    assert np.array_equal(xs, xs0) and es.tobytes() == es0.tobytes()
    _same_state(state2, state20)


def test_colour_traced_segment_at_the_nibble_limit_runs_bits():
    """Nibbles are not taken for a traced run: at the limit where an untraced segment runs nibbles with four
    chains per group, the traced segment behind it runs bits with one chain per workgroup, and its rows
    (and the handle) equal the same two segments at the device's limit."""
    from annealing_sign_problem_amd import annealer as sa

    c = _case("mixed")
    ham = _nibble_plan(c)
    nibble_limit = _colour_limits_of("mixed")[NIBBLES]

    def run(limit):
        _set_limit(ham, limit)
        with sa.Chains(ham, seed=SEED, repetitions=REPS, x0=c.x0, replica_offset=OFFSET) as chains:
            chains.advance(c.betas[:1], sweep_order="colour")
            ran = [(_spin_layout(ham), _last_m(ham))]
            rows = chains.advance(c.betas[1:9], sweep_order="colour", trace=True)
            ran.append((_spin_layout(ham), _last_m(ham)))
            return ran, rows, chains.state()

    ran, rows, state = run(nibble_limit)
    assert ran == [(NIBBLES, 4), (BITS, 1)], ran
    ran0, rows0, state0 = run(0)
    assert ran0 == [(WORDS, 4)] * 2, ran0
    assert rows.shape == (REPS, 9) and np.array_equal(rows, rows0)
    _same_state(state, state0)


def test_colour_batch_has_a_nibble_class_at_small_sizes():
    """Plans limited to nibbles go into the shared launches of asp_sa_anneal_batch as its nibble class,
    beside one at the device's limit: every item is its single call, "mixed" the oracle's."""
    from annealing_sign_problem_amd import annealer as sa

    names = ("mixed", "leaves", "k65", "field_only")
    cases = [_case(name) for name in names]
    hams = [c.fresh() for c in cases]
    for c, ham in zip(cases[:3], hams[:3]):
        _set_limit(ham, _colour_limits(ham)[NIBBLES])
        _set_launch(ham, 0)  # (a plan with a forced geometry runs alone)
    singles = [sa.anneal_raw(c.ham, SEED + i, c.betas, REPS, OFFSET, None) for i, c in enumerate(cases)]
    batch = sa.anneal_batch_raw(hams, [SEED + i for i in range(4)], [c.betas for c in cases], [REPS] * 4, [OFFSET] * 4)
    for i, (c, ham, (bx, be), (sx, se)) in enumerate(zip(cases, hams, batch, singles)):
        assert i == 3 or _spin_layout(ham) == NIBBLES, c.name
        assert np.array_equal(bx, sx) and be.tobytes() == se.tobytes(), c.name
    assert _spin_layout(hams[3]) in (WORDS, BYTES)
    oxs, oes, otracked, oaccepted = oracle.sa_anneal(cases[0].J, cases[0].h, SEED, cases[0].betas, REPS, OFFSET, None,
                                                     cases[0].info.energy_scale_exp, num_threads=4)
    tracked, accepted = _stats(hams[0], REPS)
    assert np.array_equal(batch[0][0], oxs) and batch[0][1].tobytes() == oes.tobytes()
    assert np.array_equal(tracked, otracked) and np.array_equal(accepted, oaccepted)


def test_greedy_under_a_bits_limit():
    from annealing_sign_problem_amd import annealer as sa

    c = _case("mixed")
    ham = c.fresh()
    limits = _colour_limits(ham)
    _set_launch(ham, 0)
    x0, e0 = sa.greedy_solve(ham)
    assert _spin_layout(ham) in (WORDS, BYTES)
    _set_limit(ham, limits[BITS])
    x1, e1 = sa.greedy_solve(ham)
    assert _spin_layout(ham) == BITS
    assert np.array_equal(x0, x1) and np.float64(e0).tobytes() == np.float64(e1).tobytes()
    ox, oe = oracle.greedy_solve(c.J, c.h)
    assert np.array_equal(np.asarray(x1).reshape(-1), np.asarray(ox).reshape(-1))
    assert np.float64(e1).tobytes() == np.float64(oe).tobytes()
