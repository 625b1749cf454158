"""The word layout keeps each chain's best configuration as difference bits of the LDS spin words and
writes it once per launch (csrc/sa_device.hpp, csrc/sa_sweep.hip).  Best configurations,
energies, tracked energies and accepted counts against the CPU oracle bit for bit, four chains per group,
in words, for every kernel family that runs the body in words: the closed call with and without tail
sweeps, aligned and generic, segments of a handle, a ladder segment and a batch.

The cases are those of tests/lazy_best_cases.py; every reference is computed once per module and frozen."""
import numpy as np
import pytest

import lazy_best_cases as lb
import oracle

pytestmark = pytest.mark.gpu

RUN_SEED = 31
WORDS = 2  # asp_sa_last_layout
CHAINS = {"4 chains": (0, 4), "8 chains": (0, 8), "5 chains from replica 3": (3, 5)}
THREADS = (64, 256, 1024)


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class _Model:
    def __init__(self, spins):
        from annealing_sign_problem_amd import annealer as sa

        self.J, self.h = lb.model(spins)
        ham = sa.Hamiltonian(self.J, self.h)
        info = ham.info()
        ham.release()
        self.S, self.auto = info.energy_scale_exp, (info.beta0_auto, info.beta1_auto)
        self.minimum = None

    def x0(self, name):
        if name != "frozen":
            return None
        if self.minimum is None:
            self.minimum = np.ascontiguousarray(oracle.greedy_solve(self.J, self.h)[0], np.uint64)
            self.minimum.setflags(write=False)
        return self.minimum

    def ham(self, threads=0):
        from annealing_sign_problem_amd import _lib
        from annealing_sign_problem_amd import annealer as sa

        ham = sa.Hamiltonian(self.J, self.h)
        _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), 4, threads))
        return ham


_models = {}


def _model(spins):
    if spins not in _models:
        _models[spins] = _Model(spins)
    return _models[spins]


def _stats(ham, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(ham.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _same(got, want, what):
    names = ("configurations", "energies", "tracked energies", "accepted counts")
    for g, w, name in zip(got, want, names):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), \
            "%s: %s differ from the oracle" % (what, name)


# ---------------------------------------------------------------------------------------------
# The closed call
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lb.cases(), ids=lambda c: "%d-%s-%d" % c)
def test_closed_call(case):
    """4 chains (the aligned kernel), 8 chains (two groups) and 5 chains from replica 3 (the generic kernel);
    64, 256 and 1024 threads; tail sweeps on (automatic threshold) and off."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    spins, name, sweeps = case
    model = _model(spins)
    betas = lb.schedule(name, *model.auto, sweeps)
    x0 = model.x0(name)
    lib = _lib.load()
    ham = model.ham()
    for chains, (first, count) in CHAINS.items():
        want = _freeze(oracle.sa_anneal(model.J, model.h, RUN_SEED, betas, count, first, x0, model.S, num_threads=4))
        if name == "frozen":
            assert not want[3].any(), "the frozen case is meant to flip nothing"
        for threads in THREADS:
            _lib.check(lib.asp_sa_set_launch(ham.plan(), 4, threads))
            for tail in (-1, 0):
                sa.set_tail(ham, tail)
                xs, es = sa.anneal_raw(ham, RUN_SEED, betas, count, first, x0)
                assert lib.asp_sa_last_layout(ham.plan()) == WORDS
                _same((xs, es) + _stats(ham, count), want,
                      "%s, %d threads, tail %d" % (chains, threads, tail))
    ham.release()


# ---------------------------------------------------------------------------------------------
# Segments of a handle
# ---------------------------------------------------------------------------------------------

def _improves(trace, before, after):
    """Chains whose tracked energy falls below their lowest of sweeps 0..before somewhere in before+1..after."""
    return trace[:, before + 1:after + 1].min(axis=1) < trace[:, :before + 1].min(axis=1)


@pytest.mark.parametrize("threads", [0, 64])
@pytest.mark.parametrize("spins", [70, 600])
def test_three_segments(spins, threads):
    """Freeze, a hot segment that improves no chain, and a second freeze cut where it has improved only
    some of the chains (both read from the oracle's trace): after every segment the handle's result is the
    oracle's closed call of the sweeps so far."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    model = _model(spins)
    count = 8
    down = sa.make_schedule(*model.auto, 12)
    betas = np.concatenate([down, np.full(3, down[0]), down])
    _, _, trace = oracle.sa_anneal_trace(model.J, model.h, RUN_SEED, betas, count, 0, None, model.S, num_threads=4)
    assert not _improves(trace, 12, 15).any(), "the hot segment is meant to improve no chain"
    cuts = [n for n in range(16, 28) if 0 < _improves(trace, 15, n).sum() < count]
    assert cuts, "no length of the last segment improves only some of the chains"
    ends = [12, 15, cuts[0]]
    print("segments end after sweeps %s; the last improves chains %s" % (ends, np.nonzero(_improves(trace, 15, ends[2]))[0]))
    ham = model.ham(threads)
    chains = sa.Chains(ham, seed=RUN_SEED, repetitions=count)
    done = 0
    for end in ends:
        chains.advance(betas[done:end], sweep_order="colour")
        assert _lib.load().asp_sa_last_layout(ham.plan()) == WORDS
        done = end
        want = oracle.sa_anneal(model.J, model.h, RUN_SEED, betas[:end], count, 0, None, model.S, num_threads=4)
        state = chains.state()
        _same(chains.result() + (state["tracked_best"], state["accepted"]), want, "after sweep %d" % end)
    chains.close()
    ham.release()


def test_ladder_segments():
    """Two ladder segments of 8 chains, one at beta = 0 and seven down the automatic ladder to its coldest:
    chain r is the oracle's closed call at its own constant beta."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    model = _model(600)
    count, sweeps = 8, 6
    chain_betas = np.concatenate([[0.0], sa.make_schedule(*model.auto, count - 1)])
    ham = model.ham()
    chains = sa.Chains(ham, seed=RUN_SEED, repetitions=count)
    for segment in (1, 2):
        chains.advance_ladder(chain_betas, sweeps, sweep_order="colour")
        assert _lib.load().asp_sa_last_layout(ham.plan()) == WORDS
        xs, es = chains.result()
        state = chains.state()
        for r in range(count):
            want = oracle.sa_anneal(model.J, model.h, RUN_SEED, np.full(segment * sweeps, chain_betas[r]), 1, r,
                                    None, model.S)
            _same((xs[r:r + 1], es[r:r + 1], state["tracked_best"][r:r + 1], state["accepted"][r:r + 1]), want,
                  "chain %d after ladder segment %d" % (r, segment))
    chains.close()
    ham.release()


# ---------------------------------------------------------------------------------------------
# A batch
# ---------------------------------------------------------------------------------------------

def test_batch_of_three(monkeypatch):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    monkeypatch.setenv("ASP_BATCH_M", "4")
    models = [_model(k) for k in (70, 600, 3000)]
    hams = [m.ham() for m in models]
    schedules = [lb.schedule(name, *m.auto, 24) for m, name in zip(models, ("reheat", "monotone", "hot"))]
    reps, offsets = [8, 5, 4], [0, 3, 4]
    results = sa.anneal_batch_raw(hams, [RUN_SEED] * 3, schedules, reps, offsets)
    for i, (m, ham, (xs, es)) in enumerate(zip(models, hams, results)):
        assert _lib.load().asp_sa_last_layout(ham.plan()) == WORDS
        want = oracle.sa_anneal(m.J, m.h, RUN_SEED, schedules[i], reps[i], offsets[i], None, m.S, num_threads=4)
        _same((xs, es) + _stats(ham, reps[i]), want, "problem %d of the batch" % i)
        ham.release()
