"""The colour sweep's k-loop that ends on the block's last real term (csrc/sa_sweep.hip: block_row_sums,
ColourSweep::start's exact widths in meta[]; csrc/sa_colour_kloop.hpp: accumulate_last) against the CPU
oracle, bit for bit: configurations, energies, tracked energies and accepted counts.

The models are those of tests/kloop_tail_cases.py — every remainder of a block's longest row, one to four
quads, width 1 and 0, dummy lanes, a single longest row; tests/test_kloop_tail_cases.py asserts that —
over a ladder of 22 sweeps from hot to frozen, which ends in the field cache or in tail sweeps.  Every
kernel family that took the new loop runs (closed aligned and generic, tail, batch, segment, ladder
segment; four chains per group in words, bytes and nibbles), and one kernel of every kind that kept the
loop it had but reads the exact width all the same (one, two and eight chains per group, the descent).

Every reference is computed once per module and frozen."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import kloop_tail_cases as cases
import oracle

pytestmark = pytest.mark.gpu

SEED = 977
WORDS, BYTES, NIBBLES = 2, 0, 6  # asp_sa_last_spin_layout's codes
LAYOUTS = {"words": WORDS, "bytes": BYTES, "nibbles": NIBBLES}
FIRST, COUNT = 3, 9            # chains 3 .. 11: a generic launch; chains 4 .. 11 of them an aligned one
MANY = 512                     # chains per problem that give a shared launch groups of four
_MODELS, _ORACLE = {}, {}


def _lib():
    from annealing_sign_problem_amd import _lib as lib_module

    return lib_module


class Model:
    def __init__(self, name):
        from annealing_sign_problem_amd import annealer as sa

        self.name = name
        J, field = cases.CASES[name]()
        self.J, self.field = scipy.sparse.csr_matrix(J), np.ascontiguousarray(field, np.float64)
        ham = sa.Hamiltonian(self.J, self.field)
        self.info = ham.info()
        ham.release()
        self.betas = cases.betas_of(self.info)
        self.betas.setflags(write=False)

    def limit(self, layout):
        """The LDS of the sweep in `layout` (SweepLds in csrc/sa_colour.hpp): as the plan's limit it
        keeps the larger layouts out.  0: the device's own limit (words at these sizes)."""
        nb = self.info.num_blocks
        rest = nb * 8 + 288 + 2 * ((nb + 15) // 16 * 16)
        return {"words": 0, "bytes": nb * 64 + rest, "nibbles": nb * 32 + rest}[layout]

    def plan(self, layout, m=4, threads=0, tail=0):
        from annealing_sign_problem_amd import annealer as sa

        ham = sa.Hamiltonian(self.J, self.field)
        lib = _lib().load()
        if m is not None:
            _lib().check(lib.asp_sa_set_launch(ham.plan(), m, threads))
        _lib().check(lib.asp_sa_set_lds_limit(ham.plan(), ctypes.c_uint64(self.limit(layout))))
        sa.set_tail(ham, tail)
        return ham


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(name)
    return _MODELS[name]


def _oracle(name, count=COUNT, first=FIRST):
    """(xs, es, tracked, accepted) of the model's closed call: computed once, read-only."""
    key = (name, count, first)
    if key not in _ORACLE:
        c = _model(name)
        out = oracle.sa_anneal(c.J, c.field, SEED, c.betas, count, first, None, c.info.energy_scale_exp, num_threads=8)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _ran(ham):
    lib = _lib().load()
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib().check(lib.asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return lib.asp_sa_last_spin_layout(ham.plan()), m.value


def _stats(ham, count):
    tracked, accepted = np.zeros(count, np.int64), np.zeros(count, np.uint64)
    _lib().check(_lib().load().asp_sa_last_stats(ham.plan(), count, _lib().ptr(tracked), _lib().ptr(accepted)))
    return tracked, accepted


def _same(got, want, what, rows=slice(None)):
    names = ("configurations", "energies", "tracked energies", "accepted counts")
    for g, w, name in zip(got, want, names):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w[rows]).tobytes(), \
            "%s: %s differ from the oracle" % (what, name)


def _closed(c, ham, first, count):
    from annealing_sign_problem_amd import annealer as sa

    xs, es = sa.anneal_raw(ham, SEED, c.betas, count, first, None)
    return (xs, es) + _stats(ham, count)


# ---- the closed call: k_sa_sweep<4, ...>, aligned and generic, and k_sa_sweep_tail -------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_closed_call_of_four(name, layout):
    """Four chains per group without tail sweeps (the last sweeps run in the field cache): from replica 3
    (the generic kernel) and from replica 4 (the aligned one), with 1, 4 and 16 wavefronts."""
    c = _model(name)
    want = _oracle(name)
    for threads in (64, 256, 1024):
        ham = c.plan(layout, 4, threads, tail=0)
        got = _closed(c, ham, FIRST, COUNT)
        assert _ran(ham) == (LAYOUTS[layout], 4)
        _same(got, want, "%s %s from replica 3, %d threads" % (name, layout, threads))
        if threads == 256:
            got = _closed(c, ham, FIRST + 1, COUNT - 1)
            assert _ran(ham) == (LAYOUTS[layout], 4)
            _same(got, want, "%s %s from replica 4" % (name, layout), slice(1, None))
        ham.release()


@pytest.mark.parametrize("layout", ["bytes", "words"])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_closed_call_with_tail_sweeps(name, layout):
    """The tail kernels (words and bytes): the automatic threshold enters tail sweeps in the frozen end of
    the ladder, so the hot sweeps are block visits through the new loop and the last ones tail visits."""
    from annealing_sign_problem_amd import annealer as sa

    c = _model(name)
    want = _oracle(name)
    ham = c.plan(layout, 4, 0, tail=-1)
    for first, count, rows in ((FIRST, COUNT, slice(None)), (FIRST + 1, COUNT - 1, slice(1, None))):
        got = _closed(c, ham, first, count)
        assert _ran(ham) == (LAYOUTS[layout], 4)
        sweeps_min, sweeps_max, entries = sa.last_tail(ham)
        # (the first sweeps of the ladder flip about every other spin: block visits whatever the threshold)
        assert entries >= 1 and 0 < sweeps_min <= sweeps_max <= len(c.betas) - 4, (sweeps_min, sweeps_max, entries)
        _same(got, want, "%s %s with tail sweeps from replica %d" % (name, layout, first), rows)
    ham.release()


# ---- the shared launches: k_sa_sweep_batch<4, ...> ---------------------------------------------------------

@pytest.fixture(scope="module")
def many():
    return {name: _oracle(name, MANY, 0) for name in sorted(cases.CASES)}


def test_batched_closed_call(many):
    """The three models in one asp_sa_anneal_batch of 512 chains each: groups of four."""
    from annealing_sign_problem_amd import annealer as sa

    names = sorted(cases.CASES)
    models = [_model(name) for name in names]
    hams = [c.plan("words", None) for c in models]
    batch = sa.anneal_batch_raw(hams, [SEED] * 3, [c.betas for c in models], [MANY] * 3, [0] * 3)
    for name, ham, (xs, es) in zip(names, hams, batch):
        assert _ran(ham)[1] == 4, "the batch did not run groups of four"
        _same((xs, es) + _stats(ham, MANY), many[name], "batched " + name)
        ham.release()


def test_batched_segments(many):
    """asp_sa_chains_advance_batch over the three models, in two segments: the second resumes."""
    from annealing_sign_problem_amd import annealer as sa

    names = sorted(cases.CASES)
    models = [_model(name) for name in names]
    hams = [c.plan("words", None) for c in models]
    handles = [sa.Chains(ham, seed=SEED, repetitions=MANY, x0=None, replica_offset=0) for ham in hams]
    try:
        for part in (slice(0, 9), slice(9, None)):
            sa.advance_chains(handles, [c.betas[part] for c in models], "colour")
            for ham in hams:
                assert _ran(ham)[1] == 4, "the batch did not run groups of four"
        for name, handle in zip(names, handles):
            state = handle.state()
            _same(handle.result() + (state["tracked_best"], state["accepted"]), many[name], "batched segments " + name)
    finally:
        for handle in handles:
            handle.close()
        for ham in hams:
            ham.release()


# ---- a handle's segments: k_sa_sweep_resume<4, ...>, Resume and ResumeLadder --------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_segments_of_four(name, layout):
    from annealing_sign_problem_amd import annealer as sa

    c = _model(name)
    ham = c.plan(layout, 4)
    with sa.Chains(ham, seed=SEED, repetitions=COUNT, x0=None, replica_offset=FIRST) as chains:
        for part in (slice(0, 5), slice(5, 6), slice(6, None)):
            chains.advance(c.betas[part], sweep_order="colour")
            assert _ran(ham) == (LAYOUTS[layout], 4)
        state = chains.state()
        got = chains.result() + (state["tracked_best"], state["accepted"])
    _same(got, _oracle(name), "%s %s in segments" % (name, layout))
    ham.release()


LADDER_SWEEPS = 6


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_ladder_segment_of_four(name, layout):
    """Every chain at a beta of its own, from hot to frozen: chain r is the oracle's one chain at the
    constant beta[r]."""
    from annealing_sign_problem_amd import annealer as sa

    c = _model(name)
    ham = c.plan(layout, 4)
    chain_betas = np.ascontiguousarray(c.betas[[0, 21, 4, 13, 8, 2, 11, 6, 10]])
    with sa.Chains(ham, seed=SEED, repetitions=COUNT, x0=None, replica_offset=FIRST) as chains:
        chains.advance_ladder(chain_betas, LADDER_SWEEPS, sweep_order="colour")
        assert _ran(ham) == (LAYOUTS[layout], 4)
        state = chains.state()
        xs, es = chains.result()
    for r in range(COUNT):
        key = (name, "ladder", r)
        if key not in _ORACLE:
            _ORACLE[key] = oracle.sa_anneal(c.J, c.field, SEED, np.full(LADDER_SWEEPS, chain_betas[r]), 1, FIRST + r,
                                            None, c.info.energy_scale_exp)
        oxs, oes, otracked, oaccepted = _ORACLE[key]
        what = "%s %s ladder chain %d" % (name, layout, r)
        assert np.array_equal(xs[r], oxs[0]) and es[r:r + 1].tobytes() == oes.tobytes(), what
        assert state["tracked_best"][r] == otracked[0] and state["accepted"][r] == oaccepted[0], what
    ham.release()


# ---- the kernels that kept the loop they had, on the exact widths --------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 8])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_other_group_sizes_read_the_exact_width(name, m):
    """One, two and eight chains per group (bytes): every quad in full, (width + 3) / 4 of them; the last
    sweeps run in the field cache, whose marking loop walks the same quads."""
    from annealing_sign_problem_amd import annealer as sa

    c = _model(name)
    ham = c.plan("words", m, 0, tail=0)
    got = _closed(c, ham, FIRST, COUNT)
    assert _ran(ham) == (BYTES, m)
    _same(got, _oracle(name), "%s, %d chains per group" % (name, m))
    if m == 1:
        with sa.Chains(ham, seed=SEED, repetitions=COUNT, x0=None, replica_offset=FIRST) as chains:
            chains.advance(c.betas[:7], sweep_order="colour")
            chains.advance(c.betas[7:], sweep_order="colour")
            state = chains.state()
            _same(chains.result() + (state["tracked_best"], state["accepted"]), _oracle(name), name + " segments of one")
    ham.release()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_descent_reads_the_exact_width(name):
    from annealing_sign_problem_amd import annealer as sa

    c = _model(name)
    ham = c.plan("words", None)
    x, e = sa.greedy_solve(ham)
    ox, oe = oracle.greedy_solve(c.J, c.field)
    assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(ox).reshape(-1))
    assert np.float64(e).tobytes() == np.float64(oe).tobytes()
    ham.release()
