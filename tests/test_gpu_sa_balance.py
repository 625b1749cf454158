"""The colour sweep hands a colour's blocks to the wavefronts of a workgroup by tickets: the first
W = threads / 64 blocks one per wavefront, every later one to the first wavefront that is free
(DESIGN.md §5.2).  That is scheduling only, so every chain stays what the CPU oracle says.  The tests
run the smallest clusters whose colours put n blocks against W wavefronts in every way the ticket
loop distinguishes — n a multiple of W, a tail round T = n mod W of up to a quarter, up to a half and
more than a half of the wavefronts, fewer blocks than wavefronts, a single wavefront — through every
kernel that shares the sweep body, and compare configurations, energies, tracked energies and
accepted-flip counts exactly.

The block counts are computed from asp_sa_layout_host's `position` output and asserted, so that a
change of the generator or of the plan cannot silently empty a case."""
import ctypes

import numpy as np
import pytest

import oracle

N_MAIN, SEED_MAIN = 3900, 41        # blocks per colour 8 8 9 8 8 8 7 6 2 (asserted below)
REGIMES_BY_THREADS = {              # what the colours of the main cluster give against W = threads / 64
    64: {"W1"},
    128: {"T0", "half"},
    256: {"T0", "quarter", "half", "more", "fewer"},
    512: {"T0", "quarter", "fewer"},
    1024: {"fewer"},
}
REPS, OFFSET, RUN_SEED = 11, 3, 4242  # 11 chains: groups of four leave a padded last group


def _block_counts(J, field):
    """Blocks of every colour, from the host plan."""
    from annealing_sign_problem_amd import _lib

    Jc = J.tocsr()
    n = Jc.shape[0]
    indptr = np.ascontiguousarray(Jc.indptr, np.int64)
    indices = np.ascontiguousarray(Jc.indices, np.int32)
    data = np.ascontiguousarray(Jc.data, np.float64)
    info = _lib.SaInfo()
    colors = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(n, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                              _lib.ptr(np.ascontiguousarray(field, np.float64)),
                                              ctypes.byref(info), _lib.ptr(colors), _lib.ptr(position)))
    return [len(np.unique(position[colors == c] // 64)) for c in range(info.num_colors)]


def _regimes(counts, waves):
    out = set()
    for n in counts:
        if waves == 1:
            out.add("W1")
        elif n < waves:
            out.add("fewer")
        else:
            tail = n % waves
            out.add("T0" if tail == 0 else "quarter" if 4 * tail <= waves
                    else "half" if 2 * tail <= waves else "more")
    return out


def _stats(h, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(h.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _main_cluster():
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(N_MAIN, seed=SEED_MAIN)
    field = np.random.default_rng(SEED_MAIN).normal(size=N_MAIN) * 1e-3
    return J, field


def test_main_cluster_reaches_every_regime():
    """(no GPU) The colours of the main cluster against 1, 2, 4, 8 and 16 wavefronts."""
    J, field = _main_cluster()
    counts = _block_counts(J, field)
    for threads, expected in REGIMES_BY_THREADS.items():
        assert _regimes(counts, threads // 64) == expected, (threads, counts)
    assert set().union(*REGIMES_BY_THREADS.values()) == {"W1", "T0", "quarter", "half", "more", "fewer"}
    assert max(counts) > 2 * 4  # more than two rounds of four wavefronts: tickets beyond the first are drawn


class _Reference:
    """The main cluster, its schedules and the oracle's chains on them: computed once, never changed."""

    def __init__(self):
        from annealing_sign_problem_amd import annealer as sa

        self.J, self.field = _main_cluster()
        ham = sa.Hamiltonian(self.J, self.field)
        info = ham.info()
        self.S = info.energy_scale_exp
        ham.release()
        # hot: about half of the proposals are accepted (asserted where it is used), so many lanes of a
        # block flip in one visit
        self.hot = np.full(16, 600.0)
        # cools into cached and inert mode, reheats and cools again (the parity suite's ladder)
        self.modes = np.concatenate([np.geomspace(1.0, 1e12, 60), np.full(10, 1e12), np.geomspace(1e12, 2e2, 6),
                                     np.geomspace(2e2, 1e12, 40), [1e3, 1e12, 1e12, 1e5, 1e12]])
        self.anneal = sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 24)
        self._runs = {}

    def oracle(self, name):
        if name not in self._runs:
            out = oracle.sa_anneal(self.J, self.field, RUN_SEED, getattr(self, name), REPS, OFFSET, None, self.S,
                                   num_threads=8)
            for a in out:
                a.setflags(write=False)
            self._runs[name] = out
        return self._runs[name]


@pytest.fixture(scope="module")
def ref():
    return _Reference()


def _run_and_compare(ref, schedule, prepare, layout):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(ref.J, ref.field)
    prepare(_lib.load(), ham.plan())
    xs, es = sa.anneal_raw(ham, RUN_SEED, getattr(ref, schedule), REPS, OFFSET, None)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == layout
    tracked, accepted = _stats(ham, REPS)
    ham.release()
    oxs, oes, otracked, oaccepted = ref.oracle(schedule)
    assert np.array_equal(accepted, oaccepted), "accepted-flip counts differ"
    assert np.array_equal(tracked, otracked), "tracked energies differ"
    assert np.array_equal(xs, oxs), "best configurations differ"
    assert es.tobytes() == oes.tobytes(), "energies differ"
    return oaccepted


def _four(wide, threads):
    def prepare(lib, plan):
        from annealing_sign_problem_amd import _lib

        _lib.check(lib.asp_sa_set_wide(plan, 1 if wide else 0))
        _lib.check(lib.asp_sa_set_launch(plan, 4, threads))
    return prepare


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
@pytest.mark.parametrize("threads", sorted(REGIMES_BY_THREADS))
def test_every_tail_regime_hot(ref, threads, wide):
    """Four replicas per workgroup, byte and word layout, 16 hot sweeps: every way a colour's block
    count can stand against the wavefronts, with many lanes of a block flipping in the same visit."""
    accepted = _run_and_compare(ref, "hot", _four(wide, threads), 2 if wide else 0)
    rate = accepted.astype(np.float64) / (16 * N_MAIN)
    assert 0.3 < rate.min() and rate.max() < 0.7, rate


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
@pytest.mark.parametrize("threads", [256, 512])
def test_cache_mode_changes_inside_one_launch(ref, threads, wide):
    """Cooling into cached and inert mode, reheating and cooling again: skipped and cached visits
    draw their tickets like whole ones."""
    accepted = _run_and_compare(ref, "modes", _four(wide, threads), 2 if wide else 0)
    assert accepted.min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("form", ["m1", "m2", "m8", "bits", "global"])
def test_other_group_sizes_and_layouts(ref, form, threads):
    """One, two and eight replicas in bytes, a bit per position in LDS and in HBM."""
    from annealing_sign_problem_amd import _lib

    m = {"m1": 1, "m2": 2, "m8": 8, "bits": 1, "global": 1}[form]
    packed = {"bits": 1, "global": 2}.get(form, 0)

    def prepare(lib, plan):
        _lib.check(lib.asp_sa_set_wide(plan, 0))
        _lib.check(lib.asp_sa_set_packed(plan, packed))
        _lib.check(lib.asp_sa_set_launch(plan, m, threads))

    _run_and_compare(ref, "anneal", prepare, {0: 0, 1: 1, 2: 3}[packed])


@pytest.mark.gpu
def test_nibble_layout():
    """Four bits per position (chosen by the launcher beyond the capacity of bytes): 2344 blocks, eight
    wavefronts."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    n = 150000
    J, h, _ = synthetic.planted_cluster(n, seed=22, mean_degree=6.0)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = sa.make_schedule(info.beta0_auto, info.beta1_auto, 6)
    _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), 4, 512))
    xs, es = sa.anneal_raw(ham, 99, betas, 5, 2)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == 6
    tracked, accepted = _stats(ham, 5)
    ham.release()
    oxs, oes, otracked, oaccepted = oracle.sa_anneal(J, h, 99, betas, 5, 2, None, info.energy_scale_exp,
                                                    num_threads=8)
    assert np.array_equal(accepted, oaccepted) and np.array_equal(tracked, otracked)
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "words"])
def test_resumed_segments(ref, wide):
    """The anneal in three segments of a handle (k_sa_sweep_resume): the oracle's chains."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(ref.J, ref.field)
    _four(wide, 256)(_lib.load(), ham.plan())
    with sa.Chains(ham, seed=RUN_SEED, repetitions=REPS, replica_offset=OFFSET) as chains:
        for part in (ref.anneal[:7], ref.anneal[7:8], ref.anneal[8:]):
            chains.advance(part, sweep_order="colour")
            assert _lib.load().asp_sa_last_layout(ham.plan()) == (2 if wide else 0)
        xs, es = chains.result()
        state = chains.state()
    ham.release()
    oxs, oes, otracked, oaccepted = ref.oracle("anneal")
    assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
    assert np.array_equal(state["tracked_best"], otracked) and np.array_equal(state["accepted"], oaccepted)


@pytest.mark.gpu
@pytest.mark.parametrize("m,wide", [(2, False), (4, False), (4, True)])
def test_ladder_segment(ref, m, wide):
    """Every chain at its own inverse temperature (k_sa_sweep_resume with ResumeLadder): chain r is the oracle's chain on
    the constant schedule beta_r."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    sweeps, reps = 9, 5
    betas = np.array([ref.hot[0], 0.0, 1e9, ref.anneal[12], ref.anneal[-1]])
    ham = sa.Hamiltonian(ref.J, ref.field)
    _lib.check(_lib.load().asp_sa_set_wide(ham.plan(), 1 if wide else 0))
    _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), m, 256))
    with sa.Chains(ham, seed=RUN_SEED, repetitions=reps, replica_offset=OFFSET) as chains:
        chains.advance_ladder(betas, sweeps, sweep_order="colour")
        assert _lib.load().asp_sa_last_layout(ham.plan()) == (2 if wide else 0)
        xs, es = chains.result()
        state = chains.state()
    ham.release()
    for r in range(reps):
        ox, oe, otracked, oaccepted = oracle.sa_anneal(ref.J, ref.field, RUN_SEED, np.full(sweeps, betas[r]), 1,
                                                      OFFSET + r, None, ref.S)
        assert np.array_equal(xs[r], ox[0]) and es[r:r + 1].tobytes() == oe.tobytes(), r
        assert state["tracked_best"][r] == otracked[0] and state["accepted"][r] == oaccepted[0], r


def _three_problems():
    from annealing_sign_problem_amd import synthetic

    out = []
    for k, seed in ((300, 51), (1300, 43), (N_MAIN, SEED_MAIN)):
        J, h, _ = synthetic.planted_cluster(k, seed=seed)
        out.append((J, h))
    return out


@pytest.mark.gpu
def test_batched_anneal_of_three_sizes():
    """anneal_batch of three problems of different size (k_sa_sweep_batch)."""
    from annealing_sign_problem_amd import annealer as sa

    problems = _three_problems()
    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    infos = [ham.info() for ham in hams]
    schedules = [sa.make_schedule(i.beta0_auto, min(i.beta1_auto, 1e6), 18) for i in infos]
    seeds, reps = [61, 62, 63], [5, 9, 7]
    results = sa.anneal_batch_raw(hams, seeds, schedules, reps, [0, 1, 2])
    for k, ((J, h), ham, (xs, es)) in enumerate(zip(problems, hams, results)):
        tracked, accepted = _stats(ham, reps[k])
        oxs, oes, otracked, oaccepted = oracle.sa_anneal(J, h, seeds[k], schedules[k], reps[k], k, None,
                                                        infos[k].energy_scale_exp, num_threads=8)
        assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes(), k
        assert np.array_equal(tracked, otracked) and np.array_equal(accepted, oaccepted), k
    for ham in hams:
        ham.release()


@pytest.mark.gpu
def test_batched_greedy_descent_of_three_sizes():
    """greedy_solve_batch (k_sa_sweep_batch over DescentProblem) against the oracle's greedy solver."""
    from annealing_sign_problem_amd import annealer as sa

    problems = _three_problems()
    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    got = sa.greedy_solve_batch(hams)
    for (J, h), (x, e) in zip(problems, got):
        ox, oe = oracle.greedy_solve(J, h)
        assert np.array_equal(x, ox) and e == oe
    for ham in hams:
        ham.release()
