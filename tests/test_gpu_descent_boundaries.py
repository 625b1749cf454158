"""The greedy solver's strict descent — flip iff `dE < 0`, until a sweep flips nothing — on every path that
runs it, at `dE == 0` and at chosen sweep counts: asp_sa_greedy (host and device tree; spins as bytes, as bits
and in HBM; field cache on and off; 64 and 1024 threads), the team descent, asp_sa_greedy_batch (shared
launches in any order and composition, per-item caps, items that run alone inside a batch, a batch of one
with its replay), and the Python entry points.

The inputs are tests/descent_cases.py's: dyadic couplings and fields whose every sum is exact in any order,
so a mismatch is a wrong decision, not rounding; tests/test_descent_cases.py shows on the host that they are
what they claim and that they tell `<` from `<=`.  The expected (words, energy, t) of every case comes from
the exact reference there, never from the library; every comparison is exact (the energy with ==), and every
path is asserted to have run through asp_sa_last_layout / _last_spin_layout / _last_launch / _last_stats."""
import ctypes

import numpy as np
import pytest

import descent_cases as dc

pytestmark = pytest.mark.gpu

BYTES, BITS, HBM, TEAM = 0, 1, 3, 4  # asp_sa_last_layout's codes
ALL = dc.names()
CAPPED = dc.names("domino", "stop")  # the cases whose t was chosen: also capped at t - 1, t and t + 1


def _lib():
    from annealing_sign_problem_amd import _lib

    return _lib


def _sa():
    from annealing_sign_problem_amd import annealer

    return annealer


def _plan(c, prepare=None):
    ham = _sa().Hamiltonian(c.J, c.h)
    if prepare is not None:
        prepare(ham)
    return ham


def _greedy(ham, cap=dc.CAP):
    """asp_sa_greedy: (x, e, out_sweeps)."""
    words = (ham.size + 63) // 64
    x = np.zeros(max(words, 1), dtype=np.uint64)
    e = np.zeros(1)
    sweeps = ctypes.c_uint32(0)
    _lib().check(_lib().load().asp_sa_greedy(ham.plan(), ctypes.c_uint32(cap), _lib().ptr(x), _lib().ptr(e),
                                             ctypes.byref(sweeps)))
    return x[:words], float(e[0]), int(sweeps.value)


def _greedy_batch(hams, caps):
    """asp_sa_greedy_batch with a cap per item: [(x, e, t)]."""
    n = len(hams)
    items = (_lib().SaGreedyItem * n)()
    xs = [np.zeros(max((h.size + 63) // 64, 1), dtype=np.uint64) for h in hams]
    es = np.zeros(n)
    sweeps = np.zeros(n, dtype=np.uint32)
    for i, h in enumerate(hams):
        items[i].plan = h.plan()
        items[i].max_sweeps = int(caps[i])
        items[i].flags = 0
        items[i].out_x = xs[i].ctypes.data
        items[i].out_e = es.ctypes.data + 8 * i
        items[i].out_sweeps = sweeps.ctypes.data + 4 * i
    _lib().check(_lib().load().asp_sa_greedy_batch(items, ctypes.c_uint32(n)))
    return [(xs[i][:(hams[i].size + 63) // 64], float(es[i]), int(sweeps[i])) for i in range(n)]


def _chunks(t, cap):
    """What asp_sa_greedy reports when the descent converges at t (include/asp.h): whole chunks of 8."""
    return min(cap, 8 * (-(-(t - 1) // 8) + 1))


def _layouts(ham):
    lib = _lib().load()
    return lib.asp_sa_last_layout(ham.plan()), lib.asp_sa_last_spin_layout(ham.plan())


def _launch(ham):
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib().check(_lib().load().asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return m.value, threads.value, groups.value


def _ran_alone(ham):
    """The plan's last descent went through asp_sa_greedy's device half (it left one chain's statistics), not
    through a shared launch of asp_sa_greedy_batch (which clears them)."""
    return _lib().load().asp_sa_last_stats(ham.plan(), 1, None, None) == 0


def _same(c, got, cap, what):
    """words, energy and (where the path reports it) the exact t against the reference."""
    words, energy, t = c.expected(cap)
    x, e = got[0], got[1]
    if not np.array_equal(x, words):
        a, b = dc.spins_of(x, c.n), dc.spins_of(words, c.n)
        wrong = [i for i in range(c.n) if a[i] != b[i]]
        raise AssertionError("%s, %s, cap %d: %d spins differ from the exact descent, first spin %d (h = %s)" % (
            what, c.name, cap, len(wrong), wrong[0], float(c.h[wrong[0]]).hex()))
    assert e == energy, "%s, %s, cap %d: energy %s, exact %s" % (what, c.name, cap, float(e).hex(), float(energy).hex())
    if len(got) > 2 and got[2] is not None:
        assert got[2] == t, "%s, %s, cap %d: %d sweeps, exact %d" % (what, c.name, cap, got[2], t)


def _caps(c):
    return [dc.CAP] + ([max(c.t - 1, 0), c.t, c.t + 1] if c.name in CAPPED else [])


# ---------------------------------------------------------------------------------------------
# asp_sa_greedy on a fresh plan
# ---------------------------------------------------------------------------------------------

SPIN_LAYOUTS = {"bytes": BYTES, "bits": BITS, "hbm": HBM}


def _prepare_single(tree, layout, cache, threads):
    def prepare(ham):
        lib, check = _lib().load(), _lib().check
        check(lib.asp_sa_set_greedy_tree(ham.plan(), tree))
        check(lib.asp_sa_set_team(ham.plan(), 0))
        if layout == "bits":
            check(lib.asp_sa_set_packed(ham.plan(), 1))
        if layout == "hbm":  # not even a bit per spin fits a limit of one byte: the words stay in HBM
            check(lib.asp_sa_set_lds_limit(ham.plan(), ctypes.c_uint64(1)))
        check(lib.asp_sa_set_field_cache(ham.plan(), cache))
        check(lib.asp_sa_set_launch(ham.plan(), 0, threads))

    return prepare


@pytest.mark.parametrize("threads", [64, 1024])
@pytest.mark.parametrize("cache", [1, 0], ids=["cache", "nocache"])
@pytest.mark.parametrize("layout", sorted(SPIN_LAYOUTS))
@pytest.mark.parametrize("tree", [0, 1, 2], ids=["host_tree", "device_tree", "device_tree_hbm"])
def test_single_call(tree, layout, cache, threads):
    """Every case, the chosen-t ones also capped one below, at and one above t: the reference's words and
    energy, and out_sweeps = min(cap, 8 (ceil((t - 1) / 8) + 1)), the whole chunks performed."""
    for name in ALL:
        c = dc.case(name)
        ham = _plan(c, _prepare_single(tree, layout, cache, threads))
        for cap in _caps(c):
            x, e, sweeps = _greedy(ham, cap)
            _same(c, (x, e), cap, "asp_sa_greedy")
            assert sweeps == _chunks(c.t, cap), (name, cap, sweeps)
            if cap > 0:  # (no sweep, no launch)
                assert _layouts(ham) == (SPIN_LAYOUTS[layout],) * 2, (name, _layouts(ham))
                assert _launch(ham) == (1, threads, 1), (name, _launch(ham))
        ham.release()


def test_twice_on_one_plan():
    """A second descent on the same plan returns the same bytes: nothing is left over from the first (the
    field cache's buffer, the work buffers, the device tree's)."""
    for tree in (0, 1):
        for name in ALL:
            c = dc.case(name)
            ham = _plan(c, lambda ham: _lib().check(_lib().load().asp_sa_set_greedy_tree(ham.plan(), tree)))
            first = _greedy(ham)
            capped = _greedy(ham, max(c.t - 1, 0))
            second = _greedy(ham)
            ham.release()
            _same(c, first[:2], dc.CAP, "first call")
            _same(c, capped[:2], max(c.t - 1, 0), "capped call between")
            assert first[0].tobytes() == second[0].tobytes() and first[1:] == second[1:], name
            assert np.float64(first[1]).tobytes() == np.float64(second[1]).tobytes(), name


# ---------------------------------------------------------------------------------------------
# Team descent
# ---------------------------------------------------------------------------------------------

TEAM_CASES = dc.names("ties", "ties_field", "stop", "domino")


@pytest.mark.parametrize("team", [2, 4, 8])
def test_team_descent(team):
    """k_sa_sweep_team<true> (its own statement of the rule) on every tie, stop and domino case — each has at
    least two colours, which a team needs: the reference's result, byte for byte the result without teams."""
    lib = _lib().load()
    for name in TEAM_CASES:
        c = dc.case(name)
        assert c.colours >= 2
        ham = _plan(c)
        out = {}
        for size in (team, 0):
            _lib().check(lib.asp_sa_set_team(ham.plan(), size))
            for cap in _caps(c):
                out[size, cap] = _greedy(ham, cap)
                if cap > 0:
                    assert _layouts(ham) == ((TEAM, BITS) if size else (BYTES, BYTES)), (name, size, _layouts(ham))
                _same(c, out[size, cap][:2], cap, "team of %d" % size)
                assert out[size, cap][2] == _chunks(c.t, cap), (name, size, cap)
        ham.release()
        for cap in _caps(c):
            assert out[team, cap][0].tobytes() == out[0, cap][0].tobytes() and out[team, cap][1:] == out[0, cap][1:]


# ---------------------------------------------------------------------------------------------
# asp_sa_greedy_batch
# ---------------------------------------------------------------------------------------------

def _batch(names, caps=None, prepare=None):
    """One asp_sa_greedy_batch call on fresh plans: [(x, e, t)] and, per item, whether it ran alone (an item
    capped at 0 sweeps that runs alone launches nothing and leaves no trace: it counts as shared here)."""
    cases = [dc.case(name) for name in names]
    hams = [_plan(c, prepare) for c in cases]
    caps = [dc.CAP] * len(hams) if caps is None else caps
    got = _greedy_batch(hams, caps)
    alone = [_ran_alone(ham) for ham in hams]
    for ham, lonely, cap in zip(hams, alone, caps):
        if not lonely and len(hams) > 1:  # what a shared launch records: one chain in bytes, one workgroup
            assert _layouts(ham) == (BYTES, BYTES) and _launch(ham)[0] == 1 and _launch(ham)[2] == 1
        ham.release()
    return got, alone


def _set(cache, tree):
    def prepare(ham):
        _lib().check(_lib().load().asp_sa_set_field_cache(ham.plan(), cache))
        _lib().check(_lib().load().asp_sa_set_greedy_tree(ham.plan(), tree))

    return prepare


@pytest.mark.parametrize("tree", [0, 1], ids=["host_tree", "device_tree"])
@pytest.mark.parametrize("cache", [1, 0], ids=["cache", "nocache"])
def test_batch_in_any_order_and_composition(cache, tree):
    """All cases in one call, then reversed, then split in two: every item in a shared launch, the exact t per
    item, the same bytes whatever the batch."""
    prepare = _set(cache, tree)
    whole, alone = _batch(ALL, prepare=prepare)
    assert not any(alone)
    for name, got in zip(ALL, whole):
        _same(dc.case(name), got, dc.CAP, "batch")
    backwards = _batch(ALL[::-1], prepare=prepare)[0][::-1]
    half = len(ALL) // 2
    split = _batch(ALL[:half], prepare=prepare)[0] + _batch(ALL[half:], prepare=prepare)[0]
    for name, a, b, s in zip(ALL, whole, backwards, split):
        for other in (b, s):
            assert a[0].tobytes() == other[0].tobytes() and a[1:] == other[1:], name


@pytest.mark.parametrize("cache", [1, 0], ids=["cache", "nocache"])
def test_batch_with_a_cap_per_item(cache):
    """Every case three times in one call, capped at t - 1, t and t + 1 (StopWhenStill against the cap)."""
    names, caps = [], []
    for name in ALL:
        t = dc.case(name).t
        for cap in (t - 1, t, t + 1):
            names.append(name), caps.append(cap)
    got, alone = _batch(names, caps, _set(cache, 0))
    assert not any(alone)
    for name, cap, g in zip(names, caps, got):
        _same(dc.case(name), g, cap, "batch, mixed caps")


def test_batch_of_one_replays_to_the_exact_t():
    """A batch of one takes asp_sa_greedy's chunks of 8 and finds t by replaying the last chunk that flipped
    (csrc/sa_anneal.hip: greedy_relax, t = flipped_at + u + 1): the t of the shared launches, at every cap."""
    for name in ALL:
        c = dc.case(name)
        for cap in _caps(c):
            got, alone = _batch([name], [cap])
            assert alone == [cap > 0]
            _same(c, got[0], cap, "batch of one")


FORCED = {
    "bits": (lambda lib, p: lib.asp_sa_set_packed(p, 1), (BITS, BITS)),
    "hbm": (lambda lib, p: lib.asp_sa_set_lds_limit(p, ctypes.c_uint64(1)), (HBM, HBM)),
    "threads": (lambda lib, p: lib.asp_sa_set_launch(p, 0, 1024), (BYTES, BYTES)),
    "team": (lambda lib, p: lib.asp_sa_set_team(p, 2), (TEAM, BITS)),
}


def test_items_that_run_alone_inside_a_batch():
    """Plans with a forced layout, geometry or team size take the single path inside the call, replay
    included, beside items in the shared launches: the same exact t either way."""
    lib = _lib().load()
    kinds = list(FORCED)
    cases = [dc.case(name) for name in ALL]
    hams, want_alone = [], []
    for i, c in enumerate(cases):
        ham = _plan(c)
        kind = kinds[(i // 2) % len(kinds)] if i % 2 == 0 else None
        if kind is not None:
            _lib().check(FORCED[kind][0](lib, ham.plan()))
        hams.append(ham), want_alone.append(kind)
    got = _greedy_batch(hams, [dc.CAP] * len(hams))
    for c, ham, kind, g in zip(cases, hams, want_alone, got):
        assert _ran_alone(ham) == (kind is not None), c.name
        assert _layouts(ham) == (FORCED[kind][1] if kind else (BYTES, BYTES)), (c.name, kind, _layouts(ham))
        _same(c, g, dc.CAP, "batch, item %s" % (kind or "shared"))
        ham.release()


# ---------------------------------------------------------------------------------------------
# The Python entry points
# ---------------------------------------------------------------------------------------------

PUBLIC = ["ties_63_4", "ties_field_65_6", "ties_257_6", "domino_stop", "domino_t17"]


def test_public_entry_points():
    from annealing_sign_problem_amd import common

    sa = _sa()
    cases = [dc.case(name) for name in PUBLIC]
    for c in cases:
        for tree in (None, "device"):
            ham = _plan(c)
            _same(c, sa.greedy_solve(ham, tree=tree), dc.CAP, "sa.greedy_solve(tree=%r)" % tree)
            ham.release()
    hams = [_plan(c) for c in cases]
    for c, got in zip(cases, sa.greedy_solve_batch(hams, return_sweeps=True)):
        _same(c, got, dc.CAP, "sa.greedy_solve_batch")
    capped = sa.greedy_solve_batch(hams, max_sweeps=9, return_sweeps=True)
    for c, ham, got in zip(cases, hams, capped):
        _same(c, got, 9, "sa.greedy_solve_batch(max_sweeps=9)")
        ham.release()

    def models():
        return [common.IsingModel(np.arange(c.n, dtype=np.uint64) * 3 + 1, None, _plan(c), None) for c in cases]

    batched = common.solve_ising_models(models(), mode="greedy")
    looped = [common.solve_ising_model(m, mode="greedy") for m in models()]
    for c, b, one in zip(cases, batched, looped):
        assert np.array_equal(b, c.expected()[0]) and np.array_equal(one, c.expected()[0]), c.name
