"""What a colour sweep does outside its visits ("Sweep end"): the exact reduction of the
sweep's energy change and flip counts between registers with the totals in lane 63, skipped by a
wavefront none of whose lanes accepted a flip; the bookkeeping of the sweep's outcome (tracked and best
energy, cache mode, snapshot of the improved replicas) behind it; the skipped visits of cached mode.
None of it may change a chain, so every comparison is exact against the CPU oracle: configurations,
energies, tracked energies, accepted counts and, with a trace, the tracked energy after every sweep.

The cases put single flips at chosen lanes of chosen blocks (the ends of the rows of 16 lanes the
reduction works in, first, last and padded blocks of a colour), make the 64-bit sums carry between
their halves with both signs, put wavefronts without a flip beside wavefronts with flips, switch the
cache mode back and forth, and run every kernel that shares the sweep body.  The spins, block counts
and sizes of the sums the cases rely on are computed from the host plan and the oracle and asserted
without a GPU, so that a change of the generator or of the plan cannot silently empty a case."""
import ctypes

import numpy as np
import pytest

import oracle

N_MAIN, SEED_MAIN = 3900, 41        # blocks per colour 8 8 9 8 8 8 7 6 2, last blocks padded (asserted below)
REPS, OFFSET, RUN_SEED = 11, 3, 4242  # 11 chains from offset 3: unaligned first replica, padded last group of four
LANES = (0, 15, 16, 31, 32, 47, 48, 63)  # first and last lane of every row of 16
FROZEN = np.full(2, 1e15)


def _layout(J, field):
    """(info, colour of every spin, position of every spin) from the host plan."""
    from annealing_sign_problem_amd import _lib

    Jc = J.tocsr()
    n = Jc.shape[0]
    info = _lib.SaInfo()
    colors = np.zeros(n, np.int32)
    position = np.zeros(n, np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(n, _lib.ptr(np.ascontiguousarray(Jc.indptr, np.int64)),
                                              _lib.ptr(np.ascontiguousarray(Jc.indices, np.int32)),
                                              _lib.ptr(np.ascontiguousarray(Jc.data, np.float64)),
                                              _lib.ptr(np.ascontiguousarray(field, np.float64)),
                                              ctypes.byref(info), _lib.ptr(colors), _lib.ptr(position)))
    return info, colors, position


def _stats(h, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(h.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _flipped(x0, spin):
    x = x0.copy()
    x[spin >> 6] ^= np.uint64(1) << np.uint64(spin & 63)
    return x


class _Reference:
    """The main cluster, its plan, its schedules, the single-flip cases and the oracle's chains:
    computed once (on the CPU), never changed."""

    def __init__(self):
        from annealing_sign_problem_amd import annealer as sa
        from annealing_sign_problem_amd import synthetic

        self.J, _, _ = synthetic.planted_cluster(N_MAIN, seed=SEED_MAIN)
        self.field = np.random.default_rng(SEED_MAIN).normal(size=N_MAIN) * 1e-3
        info, self.colors, self.position = _layout(self.J, self.field)
        self.S = info.energy_scale_exp
        self.num_colors = info.num_colors
        self.hot = np.full(16, 600.0)  # about half of the proposals accepted
        # cools into cached and inert mode, reheats and cools again, single hot sweeps between cold ones
        self.modes = np.concatenate([np.geomspace(1.0, 1e12, 60), np.full(10, 1e12), np.geomspace(1e12, 2e2, 6),
                                     np.geomspace(2e2, 1e12, 40), [1e3, 1e12, 1e12, 1e5, 1e12]])
        self.cooling = self.modes[:70]
        self.anneal = sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 24)
        self.x_min, _ = oracle.greedy_solve(self.J, self.field)
        self.x_min.setflags(write=False)
        self._runs = {}
        self._cases = None

    def blocks(self, c):
        """(blocks of colour c in ascending order, spins in each)."""
        return np.unique(self.position[self.colors == c] // 64, return_counts=True)

    def spin_at(self, block, lane):
        hit = np.nonzero(self.position == block * 64 + lane)[0]
        return int(hit[0]) if hit.size else None

    def single(self, spin, reps=4, offset=0):
        """The oracle's two frozen sweeps from the greedy minimum with `spin` flipped back."""
        return oracle.sa_anneal(self.J, self.field, RUN_SEED, FROZEN, reps, offset, _flipped(self.x_min, spin),
                                self.S)

    def cases(self):
        """{(kind, lane): spin}: for every wanted lane of a first block, a last full block and a padded
        last block of a colour, a spin there whose flip back is the only flip of the two sweeps.  That is
        certain in the first colour (the spin is restored before any neighbour is visited); the padded
        blocks of the later colours add the short fills."""
        if self._cases is None:
            found = {}
            for c in range(self.num_colors):
                blocks, fill = self.blocks(c)
                targets = [("first", blocks[0], lane) for lane in LANES]
                last_full = blocks[fill == 64][-1]
                targets += [("last_full", last_full, lane) for lane in LANES]
                if fill[-1] < 64:
                    top = int(fill[-1]) - 1
                    targets += [("padded", blocks[-1], lane) for lane in LANES if lane < top]
                    targets += [("padded_top", blocks[-1], top)]
                for kind, block, lane in targets:
                    key = (kind, lane) if kind != "padded_top" else (kind, c)
                    if key in found:
                        continue
                    spin = self.spin_at(block, lane)
                    if spin is not None and np.all(self.single(spin)[3] == 1):
                        found[key] = spin
            self._cases = found
        return self._cases

    def oracle(self, name, trace=False):
        key = (name, trace)
        if key not in self._runs:
            fn = oracle.sa_anneal_trace if trace else oracle.sa_anneal
            self._runs[key] = _freeze(fn(self.J, self.field, RUN_SEED, getattr(self, name), REPS, OFFSET, None,
                                         self.S, num_threads=8))
        return self._runs[key]


@pytest.fixture(scope="module")
def ref():
    return _Reference()


def test_single_flip_cases_cover_the_lanes_and_blocks(ref):
    """(no GPU) The greedy minimum is frozen at beta = 1e15, and flipping one spin back gives exactly one
    accepted flip for a spin at every wanted lane of a first block and of a last full block, and at the
    lanes a padded last block has, its last filled lane among them."""
    assert np.all(ref.single(0)[3] >= 1)
    frozen = oracle.sa_anneal(ref.J, ref.field, RUN_SEED, FROZEN, 4, 0, ref.x_min, ref.S)
    assert np.all(frozen[3] == 0)
    cases = ref.cases()
    for lane in LANES:
        assert ("first", lane) in cases and ("last_full", lane) in cases, lane
    assert {lane for kind, lane in cases if kind == "padded"} >= {0, 15, 16, 31, 32, 47, 48}
    tops = [c for kind, c in cases if kind == "padded_top"]
    assert len(tops) >= 3, tops
    assert any(ref.blocks(c)[1][-1] < 16 for c in tops), "no padded block shorter than a row of 16 lanes"


def test_hot_sweeps_carry_with_both_signs(ref):
    """(no GPU) The oracle's per-sweep changes of the tracked energy on the hot schedule: both signs, and
    magnitudes beyond 2^32 with both signs, so the 64-bit sums carry between their 32-bit halves."""
    trace = ref.oracle("hot", trace=True)[2]
    delta = np.diff(trace, axis=1)
    assert (delta > 2 ** 32).any() and (delta < -2 ** 32).any()
    accepted = ref.oracle("hot")[3]
    rate = accepted.astype(np.float64) / (16 * N_MAIN)
    assert 0.3 < rate.min() and rate.max() < 0.7, rate


def _prepare(ham, m, threads, wide=0, packed=0, cache=1):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    _lib.check(lib.asp_sa_set_wide(ham.plan(), wide))
    _lib.check(lib.asp_sa_set_packed(ham.plan(), packed))
    _lib.check(lib.asp_sa_set_field_cache(ham.plan(), cache))
    _lib.check(lib.asp_sa_set_launch(ham.plan(), m, threads))


def _compare(got, tracked, accepted, want):
    oxs, oes, otracked, oaccepted = want[0], want[1], want[-2], want[-1]
    assert np.array_equal(accepted, oaccepted), "accepted-flip counts differ"
    assert np.array_equal(tracked, otracked), "tracked energies differ"
    assert np.array_equal(got[0], oxs), "best configurations differ"
    assert got[1].tobytes() == oes.tobytes(), "energies differ"


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 1024])
def test_single_flip_at_every_chosen_lane(ref, threads):
    """Two frozen sweeps from the greedy minimum with one spin flipped back: exactly one accepted flip
    per chain, in one lane of one wavefront, and the oracle's tracked energy."""
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, 4, threads)
    for key, spin in sorted(ref.cases().items()):
        got = sa.anneal_raw(ham, RUN_SEED, FROZEN, 4, 0, _flipped(ref.x_min, spin))
        tracked, accepted = _stats(ham, 4)
        assert np.all(accepted == 1), key
        want = ref.single(spin)
        _compare(got, tracked, accepted, want)
        assert np.all(tracked < 0), key
    ham.release()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 1024])
@pytest.mark.parametrize("reps,offset", [(4, 0), (REPS, OFFSET)], ids=["one_group", "padded_last_group"])
def test_one_flip_in_each_replica_of_a_group(ref, threads, reps, offset):
    """Every chain starts from the minimum with a spin of its own flipped back (per-chain starts of a
    handle): every replica of a group reduces one flip of another lane and block."""
    from annealing_sign_problem_amd import annealer as sa

    spins = [spin for _, spin in sorted(ref.cases().items())]
    spins = [spins[(5 * r + 1) % len(spins)] for r in range(reps)]
    assert len(set(spins[:4])) == 4
    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, 4, threads)
    x0 = np.stack([_flipped(ref.x_min, s) for s in spins])
    with sa.Chains(ham, seed=RUN_SEED, repetitions=reps, x0=x0, replica_offset=offset) as chains:
        trace = chains.advance(FROZEN, sweep_order="colour", trace=True)
        xs, es = chains.result()
        state = chains.state()
    ham.release()
    for r, spin in enumerate(spins):
        ox, oe, otrace, otracked, oaccepted = _single_trace(ref, spin, offset + r)
        assert oaccepted[0] == 1 and state["accepted"][r] == 1, r
        assert np.array_equal(xs[r], ox[0]) and es[r:r + 1].tobytes() == oe.tobytes(), r
        assert state["tracked_best"][r] == otracked[0], r
        assert np.array_equal(trace[r], otrace[0]), r


def _single_trace(ref, spin, replica):
    """(x, e, trace, tracked, accepted) of one oracle chain from the minimum with `spin` flipped back."""
    x0 = _flipped(ref.x_min, spin)
    ox, oe, otrace = oracle.sa_anneal_trace(ref.J, ref.field, RUN_SEED, FROZEN, 1, replica, x0, ref.S)
    _, _, otracked, oaccepted = oracle.sa_anneal(ref.J, ref.field, RUN_SEED, FROZEN, 1, replica, x0, ref.S)
    return ox, oe, otrace, otracked, oaccepted


def _traced_run(ref, schedule, m, threads, wide=0, cache=1):
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, m, threads, wide=wide, cache=cache)
    xs, es, trace = sa.anneal_trace_raw(ham, RUN_SEED, getattr(ref, schedule), REPS, OFFSET, None)
    tracked, accepted = _stats(ham, REPS)
    ham.release()
    oxs, oes, otrace = ref.oracle(schedule, trace=True)
    assert np.array_equal(trace, otrace), "tracked energies after the sweeps differ"
    _compare((xs, es), tracked, accepted, ref.oracle(schedule))
    return accepted


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1], ids=["bytes", "words"])
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_hot_sweeps_carries_and_signs(ref, threads, wide):
    """Sixteen hot sweeps, every sweep's tracked energy compared: sums of both signs beyond 2^32 (asserted
    on the CPU above), many lanes of every wavefront accepting."""
    _traced_run(ref, "hot", 4, threads, wide=wide)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
def test_cooling_leaves_wavefronts_without_flips(ref, threads):
    """The cooling part of the `modes` ladder with a trace: towards its end a sweep's few flips sit in
    one or two of the wavefronts and the others skip their reduction, then nobody flips at all."""
    accepted = _traced_run(ref, "cooling", 4, threads)
    assert accepted.min() > 0
    tail = np.diff(ref.oracle("cooling", trace=True)[2], axis=1)[:, -10:]
    assert np.all(tail == 0), "the ladder's cold end is not frozen"


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [1, 0], ids=["cache_on", "cache_off"])
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_skipped_visits_and_mode_switches(ref, threads, cache):
    """The whole `modes` ladder — freeze, reheat, freeze, single hot sweeps between cold ones — with the
    field cache on and off: both are the oracle's chains, sweep by sweep."""
    _traced_run(ref, "modes", 4, threads, cache=cache)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["m1", "m2", "m4_aligned", "m4_unaligned", "m8", "m4_words", "m4_words_aligned",
                                  "bits", "global"])
def test_every_group_size_and_layout(ref, form):
    """One, two, four and eight replicas in bytes, four in words, a bit per position in LDS and in HBM; four replicas with an aligned first replica (one Philox call per group) and an unaligned one."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    m = {"m1": 1, "m2": 2, "m8": 8, "bits": 1, "global": 1}.get(form, 4)
    wide = 1 if "words" in form else 0
    packed = {"bits": 1, "global": 2}.get(form, 0)
    offset = 4 if "_aligned" in form else OFFSET
    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, m, 256, wide=wide, packed=packed)
    got = sa.anneal_raw(ham, RUN_SEED, ref.modes, REPS, offset, None)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == ({1: 1, 2: 3}[packed] if packed else 2 * wide)
    tracked, accepted = _stats(ham, REPS)
    ham.release()
    if offset == OFFSET:
        want = ref.oracle("modes")
    else:
        want = oracle.sa_anneal(ref.J, ref.field, RUN_SEED, ref.modes, REPS, offset, None, ref.S, num_threads=8)
    _compare(got, tracked, accepted, want)


@pytest.mark.gpu
def test_nibble_layout():
    """Four bits per position: the launcher chooses it beyond the capacity of bytes only, so this one case
    is as large as that takes (2344 blocks, sixteen wavefronts)."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, h, _ = synthetic.planted_cluster(150000, seed=23, mean_degree=6.0)
    ham = sa.Hamiltonian(J, h)
    info = ham.info()
    betas = np.concatenate([sa.make_schedule(info.beta0_auto, info.beta1_auto, 5), [1e15, 1e15]])
    _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), 4, 1024))
    xs, es = sa.anneal_raw(ham, 98, betas, 5, 2)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == 6
    tracked, accepted = _stats(ham, 5)
    ham.release()
    want = oracle.sa_anneal(J, h, 98, betas, 5, 2, None, info.energy_scale_exp, num_threads=8)
    _compare((xs, es), tracked, accepted, want)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1], ids=["bytes", "words"])
def test_resume_in_two_segments(ref, wide):
    """The `modes` ladder in two segments of a handle, cut inside its first frozen stretch (odd and even
    segment lengths): the oracle's chains and, segment by segment, its trace."""
    from annealing_sign_problem_amd import annealer as sa

    cut = 65
    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, 4, 256, wide=wide)
    with sa.Chains(ham, seed=RUN_SEED, repetitions=REPS, replica_offset=OFFSET) as chains:
        first = chains.advance(ref.modes[:cut], sweep_order="colour", trace=True)
        second = chains.advance(ref.modes[cut:], sweep_order="colour", trace=True)
        xs, es = chains.result()
        state = chains.state()
    ham.release()
    otrace = ref.oracle("modes", trace=True)[2]
    assert np.array_equal(first, otrace[:, :cut + 1]) and np.array_equal(second, otrace[:, cut:])
    _compare((xs, es), state["tracked_best"], state["accepted"], ref.oracle("modes"))


@pytest.mark.gpu
@pytest.mark.parametrize("m,wide", [(1, 0), (2, 0), (4, 0), (4, 1), (8, 0)])
def test_ladder_segment(ref, m, wide):
    """Every chain at its own inverse temperature (k_sa_sweep_resume with ResumeLadder), a frozen, a hot and an infinitely hot
    chain side by side in one group: chain r is the oracle's chain on the constant schedule beta_r."""
    from annealing_sign_problem_amd import annealer as sa

    sweeps, reps = 9, 5
    betas = np.array([1e15, ref.hot[0], 0.0, ref.anneal[12], 1e9])
    ham = sa.Hamiltonian(ref.J, ref.field)
    _prepare(ham, m, 1024, wide=wide)
    with sa.Chains(ham, seed=RUN_SEED, repetitions=reps, replica_offset=OFFSET) as chains:
        chains.advance_ladder(betas, sweeps, sweep_order="colour")
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
    for k, seed in ((200, 52), (1100, 44), (N_MAIN, SEED_MAIN)):
        J, h, _ = synthetic.planted_cluster(k, seed=seed)
        out.append((J, h))
    return out


@pytest.mark.gpu
def test_batched_call_of_three_sizes():
    """anneal_batch of three problems of different size (k_sa_sweep_batch), cooled until they freeze."""
    from annealing_sign_problem_amd import annealer as sa

    problems = _three_problems()
    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    infos = [ham.info() for ham in hams]
    schedules = [np.concatenate([sa.make_schedule(i.beta0_auto, i.beta1_auto, 30), np.full(6, 1e15)]) for i in infos]
    seeds, reps = [71, 72, 73], [5, 9, 7]
    results = sa.anneal_batch_raw(hams, seeds, schedules, reps, [0, 1, 2])
    for k, ((J, h), ham, (xs, es)) in enumerate(zip(problems, hams, results)):
        tracked, accepted = _stats(ham, reps[k])
        want = oracle.sa_anneal(J, h, seeds[k], schedules[k], reps[k], k, None, infos[k].energy_scale_exp,
                                num_threads=8)
        _compare((xs, es), tracked, accepted, want)
    for ham in hams:
        ham.release()


@pytest.mark.gpu
def test_descent_stops_when_still():
    """The greedy solver's relaxation (the descent with StopWhenStill, alone and batched): the oracle's
    configuration and energy; the last sweep, the one without a flip, reduces nothing."""
    from annealing_sign_problem_amd import annealer as sa

    problems = _three_problems()
    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    batch = sa.greedy_solve_batch(hams)
    for (J, h), ham, (bx, be) in zip(problems, hams, batch):
        ox, oe = oracle.greedy_solve(J, h)
        x, e = sa.greedy_solve(ham)
        assert np.array_equal(x, ox) and e == oe
        assert np.array_equal(bx, ox) and be == oe
    for ham in hams:
        ham.release()
