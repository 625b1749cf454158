"""GPU: batched isoenergetic cluster moves (asp_sa_chains_cluster_move_batch, annealer.cluster_move_chains /
.parallel_tempering_cluster_batch, common.solve_ising_models(method="tempering-cluster"); DESIGN.md §4.13
"Batched form") against the law as tests/cluster_move_law.py restates it.

Every comparison is exact: all five state arrays of every handle through Chains.state() and the three
outputs, per handle, against cluster_move_law.move.  The states are set with Chains.load_state, so the
differing sets are chosen: one mixed batch holds every shape on which one of the three launch classes
(a wavefront per pair up to 2048 spins; a workgroup per pair with the bit planes in LDS or in HBM) can go
wrong, and the same batch is then composed in other ways.  The expected states are computed once."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import cluster_move_law as law

pytestmark = pytest.mark.gpu

INVALID = -3
STATE = ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")


def _same_state(a, b, what=""):
    for name in STATE:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name])), (what, name)
    assert int(a["sweeps_done"]) == int(b["sweeps_done"]), what


def _random_problem(K, seed, degree=4):
    """Asymmetric J with a diagonal, a field."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, K, size=degree * K)
    cols = rng.integers(0, K, size=degree * K)
    J = scipy.sparse.coo_matrix((rng.normal(size=degree * K), (rows, cols)), shape=(K, K)).tocsr()
    return J, rng.normal(size=K) * 0.3


def _random_x0(K, seed, rows):
    rng = np.random.default_rng(seed)
    return np.stack([law.pack(rng.random(K) < 0.5) for _ in range(rows)])


def _opposite(K, seed):
    up = np.random.default_rng(seed).random(K) < 0.5
    return np.stack([law.pack(up), law.pack(~up)])


def _start(x0, sweeps_done=0):
    """The state of fresh chains at x0, as Chains.state() gives it."""
    R = x0.shape[0]
    return {"x_current": x0.copy(), "x_best": x0.copy(), "tracked_current": np.zeros(R, dtype=np.int64),
            "tracked_best": np.zeros(R, dtype=np.int64), "accepted": np.zeros(R, dtype=np.uint64),
            "sweeps_done": sweeps_done}


class Spec:
    """One handle of the mixed batch: the problem, the chains' seed, the state its chains start from, the
    pairs and the draw of its move, where its planes go (asp_sa_chains_set_cluster_planes)."""

    def __init__(self, name, J, h, seed, start, pairs, draw=0, planes=0):
        self.name, self.J, self.h, self.seed, self.start = name, scipy.sparse.csr_matrix(J), h, seed, start
        self.pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.draw, self.planes = draw, planes
        self.K = self.J.shape[0]
        self.R = start["x_current"].shape[0]
        self.packed = (self.K + 63) // 64 <= 32


def _specs():
    specs = []
    # a path of 300 sites that all differ: 300 search rounds in one wavefront ...
    rng = np.random.default_rng(1)
    J = scipy.sparse.diags(rng.normal(size=299), 1, shape=(300, 300), format="csr")
    specs.append(Spec("path", J, rng.normal(size=300) * 0.2, 3, _start(_opposite(300, 3)), [(0, 1)]))
    # ... while its neighbours in the workgroup finish at once: identical replicas (n = 0)
    J, h = _random_problem(200, 30)
    x0 = _random_x0(200, 31, 2)[[0, 0, 1, 1]]
    specs.append(Spec("identical", J, h, 5, _start(x0), [(1, 0), (2, 3)]))
    # a star whose hub has degree 300: the row the whole wavefront walks; half of the leaves equal
    rng = np.random.default_rng(2)
    J = scipy.sparse.coo_matrix((rng.normal(size=300), (np.full(300, 17), np.delete(np.arange(301), 17))),
                                shape=(301, 301)).tocsr()
    up = rng.random(301) < 0.5
    other = ~up
    other[18:160] = up[18:160]
    x0 = np.stack([law.pack(up), law.pack(other), law.pack(~up), law.pack(up)])
    specs.append(Spec("star", J, rng.normal(size=301) * 0.2, 4, _start(x0), [(1, 0), (3, 2)], draw=2))
    # the tail word and the lanes that own nothing
    for K in (1, 63, 64, 65, 130):
        J, h = _random_problem(K, K)
        specs.append(Spec("K=%d" % K, J, h, 17, _start(_random_x0(K, K + 1, 5), sweeps_done=3), [(3, 0), (1, 4)], draw=7))
    # the last packed size (every lane owns a word) and the first workgroup size
    for K in (2048, 2049):
        J, h = _random_problem(K, K, degree=3)
        specs.append(Spec("K=%d" % K, J, h, 21, _start(_random_x0(K, K + 1, 4)), [(0, 1), (3, 2)], draw=1))
    # two dense blobs joined only through site 40, on which the replicas agree
    rng = np.random.default_rng(5)
    dense = np.zeros((81, 81))
    dense[:40, :40] = np.triu(rng.normal(size=(40, 40)), 1)
    dense[41:, 41:] = np.triu(rng.normal(size=(40, 40)), 1)
    dense[40, 3], dense[40, 60], dense[7, 40] = 0.9, -0.7, 0.4
    up = rng.random(81) < 0.5
    other = ~up
    other[40] = up[40]
    specs.append(Spec("blobs", dense, rng.normal(size=81) * 0.2, 6,
                      _start(np.stack([law.pack(up), law.pack(other)])), [(0, 1)]))
    # 257 chains with 128 pairs
    J, h = _random_problem(70, 12)
    order = np.random.default_rng(13).permutation(257)
    specs.append(Spec("257 chains", J, h, 14, _start(_random_x0(70, 15, 257), sweeps_done=2), order[:256].reshape(128, 2)))
    # no pairs at all
    J, h = _random_problem(90, 40)
    specs.append(Spec("no pairs", J, h, 8, _start(_random_x0(90, 41, 3)), np.zeros((0, 2), dtype=np.int64)))
    # 20 000 spins with the planes in HBM and in LDS
    for planes in (2, 1):
        J, h = _random_problem(20000, 16 + planes, degree=2)
        specs.append(Spec("20000 spins, planes %d" % planes, J, h, 18, _start(_random_x0(20000, 50 + planes, 4)),
                          [(1, 2), (3, 0)], draw=2, planes=planes))
    # a tie with the best energy (slot 2: nothing is replaced) beside strict improvements; see _with_a_tie
    J, h = _random_problem(70, 8)
    specs.append(Spec("tie", J, h, 10, _start(_random_x0(70, 9, 4)), [(0, 1), (2, 3)], draw=3))
    # 5 pairs, the last packed handle: its fifth pair is alone in the last workgroup
    J, h = _random_problem(100, 60)
    specs.append(Spec("5 pairs", J, h, 11, _start(_random_x0(100, 61, 10)), [(0, 9), (1, 8), (2, 7), (3, 6), (5, 4)]))
    return specs


def _with_a_tie(spec, S):
    """Slot 2's best energy becomes what its current energy will be after the move, and its best
    configuration all zeros: step 6 must keep both."""
    _, _, _, deltas = law.move(spec.J, spec.h, S, spec.start, spec.seed, spec.pairs, spec.draw)
    assert deltas[0] != 0 and deltas[1] != 0  # (a condition on the inputs)
    spec.start["tracked_best"][2] = deltas[1]
    spec.start["x_best"][2] = 0


class Batch:
    """The specs with their Hamiltonians (made once: the plans are shared by the runs, one live handle
    at a time) and what the law says comes out of the move."""

    def __init__(self):
        from annealing_sign_problem_amd import annealer as sa

        self.specs = _specs()
        self.hams = [sa.Hamiltonian(s.J, s.h) for s in self.specs]
        self.scales = [ham.info().energy_scale_exp for ham in self.hams]
        for s, S in zip(self.specs, self.scales):
            if s.name == "tie":
                _with_a_tie(s, S)
        self.expected = [law.move(s.J, s.h, S, s.start, s.seed, s.pairs, s.draw)
                         for s, S in zip(self.specs, self.scales)]

    def open(self, which=None):
        """Fresh chains of the specs `which` (indices; default all) at their start states."""
        from annealing_sign_problem_amd import _lib
        from annealing_sign_problem_amd import annealer as sa

        handles = []
        for k in range(len(self.specs)) if which is None else which:
            s = self.specs[k]
            chains = sa.Chains(self.hams[k], seed=s.seed, repetitions=s.R)
            handles.append(chains)
            chains.load_state(s.start)
            _lib.check(_lib.load().asp_sa_chains_set_cluster_planes(chains._live(), ctypes.c_int(s.planes)))
        return handles

    def check(self, which, handles, outputs):
        for k, chains, got in zip(which, handles, outputs):
            s = self.specs[k]
            state, differing, sizes, deltas = self.expected[k]
            assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.int64, s.name
            assert np.array_equal(got[0], differing), s.name
            assert np.array_equal(got[1], sizes), s.name
            assert np.array_equal(got[2], deltas), s.name
            _same_state(chains.state(), state, s.name)


@pytest.fixture(scope="module")
def batch():
    return Batch()


def _close(handles):
    for chains in handles:
        chains.close()


def test_the_inputs_are_what_the_cases_need(batch):
    """Conditions on the inputs, from the law alone."""
    by_name = {s.name: (s, e) for s, e in zip(batch.specs, batch.expected)}
    s, (_, differing, sizes, _) = by_name["path"]
    assert differing[0] == 300 and sizes[0] == 300
    _, (_, differing, sizes, deltas) = by_name["identical"]
    assert not differing.any() and not sizes.any() and not deltas.any()
    _, (_, differing, sizes, _) = by_name["star"]
    assert differing[1] == 301 and sizes[1] == 301 and 1 < differing[0] < 301
    _, (_, differing, sizes, _) = by_name["blobs"]
    assert differing[0] == 80 and sizes[0] == 40
    for name in ("20000 spins, planes 2", "20000 spins, planes 1"):
        assert np.all(by_name[name][1][2] > 1000)  # (large components)
    s, (state, _, _, deltas) = by_name["tie"]
    assert state["tracked_current"][2] == state["tracked_best"][2] == deltas[1] and not state["x_best"][2].any()
    assert state["tracked_best"].min() < 0  # (and a strict improvement)
    assert np.count_nonzero(by_name["257 chains"][1][2]) > 100
    # the path, the identical replicas and the star's first pair share the first workgroup of the packed
    # launch; the packed rows end with one pair in a workgroup of its own
    assert [x.name for x in batch.specs[:3]] == ["path", "identical", "star"]
    assert all(x.packed == (x.K <= 2048) for x in batch.specs)
    packed = sum(len(x.pairs) for x in batch.specs if x.packed)
    last = [x for x in batch.specs if x.packed][-1]
    assert packed % 4 == 1 and last.name == "5 pairs"
    assert {x.name for x in batch.specs if not x.packed} == {"K=2049", "20000 spins, planes 2", "20000 spins, planes 1"}


def _run(batch, which, flags=0):
    from annealing_sign_problem_amd import annealer as sa

    handles = batch.open(which)
    outputs = sa.cluster_move_chains(handles, [batch.specs[k].pairs for k in which],
                                     [batch.specs[k].draw for k in which], flags)
    return handles, outputs


def test_one_call_over_the_mixed_batch_and_the_same_call_again(batch):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    which = list(range(len(batch.specs)))
    handles, outputs = _run(batch, which)
    try:
        assert _lib.load().asp_sa_chains_cluster_move_batch_last_ms() > 0.0
        batch.check(which, handles, outputs)
        # the host mirror follows tracked_current: entry 0 of the next trace
        k = [s.name for s in batch.specs].index("K=65")
        trace = handles[k].advance(np.full(2, 0.4), sweep_order="colour", trace=True)
        assert np.array_equal(trace[:, 0], batch.expected[k][0]["tracked_current"])
    finally:
        _close(handles)
    # involution: the same batched call again, no sweep between, restores x_current and tracked_current
    handles, outputs = _run(batch, which)
    try:
        again = sa.cluster_move_chains(handles, [batch.specs[k].pairs for k in which],
                                       [batch.specs[k].draw for k in which])
        for k, chains, first, second in zip(which, handles, outputs, again):
            s = batch.specs[k]
            state = chains.state()
            assert np.array_equal(state["x_current"], s.start["x_current"]), s.name
            assert np.array_equal(state["tracked_current"], s.start["tracked_current"]), s.name
            assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]), s.name
            assert np.array_equal(first[2], -second[2]), s.name
    finally:
        _close(handles)


def test_composition_reversed_split_unpacked_and_single_calls(batch):
    from annealing_sign_problem_amd import annealer as sa

    count = len(batch.specs)
    # in reversed batch order
    which = list(range(count))[::-1]
    handles, outputs = _run(batch, which)
    try:
        batch.check(which, handles, outputs)
    finally:
        _close(handles)
    # split into two calls (interleaved, so both calls hold all three classes)
    for which in (list(range(0, count, 2)), list(range(1, count, 2))):
        handles, outputs = _run(batch, which)
        try:
            batch.check(which, handles, outputs)
        finally:
            _close(handles)
    # the workgroup form for every item
    which = list(range(count))
    handles, outputs = _run(batch, which, flags=sa.CLUSTER_NO_PACKED)
    try:
        batch.check(which, handles, outputs)
    finally:
        _close(handles)
    # a loop of single calls
    handles = batch.open(which)
    try:
        outputs = [chains.cluster_move(batch.specs[k].pairs, batch.specs[k].draw) for k, chains in zip(which, handles)]
        batch.check(which, handles, outputs)
    finally:
        _close(handles)


def _planted(K, seed):
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(K, seed=seed)
    return J, np.random.default_rng(seed).normal(size=K) * 0.01


@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_the_batched_driver_is_the_list_of_single_drivers_and_the_solver_its_projection(order):
    """Three planted clusters that straddle the packed limit (2048 spins)."""
    from annealing_sign_problem_amd import annealer as sa, common

    problems = [_planted(K, 70 + k) for k, K in enumerate((60, 500, 2100))]
    make = lambda: [sa.Hamiltonian(J, h) for J, h in problems]
    kw = dict(seed=5, number_rounds=6, sweeps_per_round=3, repetitions=8, sweep_order=order)
    for only_best in (False, True):
        got = sa.parallel_tempering_cluster_batch(make(), only_best=only_best, **kw)
        want = [sa.parallel_tempering_cluster(ham, only_best=only_best, **kw) for ham in make()]
        assert len(got) == len(want) == 3
        for (gx, ge), (wx, we) in zip(got, want):
            assert np.array_equal(gx, wx) and np.asarray(ge).tobytes() == np.asarray(we).tobytes()
    some = sa.parallel_tempering_cluster_batch(make(), only_best=False, cluster_rungs=2, **kw)
    for (gx, ge), ham in zip(some, make()):
        wx, we = sa.parallel_tempering_cluster(ham, only_best=False, cluster_rungs=2, **kw)
        assert np.array_equal(gx, wx) and ge.tobytes() == we.tobytes()
    # (the moves did something: without them the chains are others)
    plain = sa.parallel_tempering_cluster_batch(make(), only_best=False, cluster_rungs=0, **kw)
    full = sa.parallel_tempering_cluster_batch(make(), only_best=False, **kw)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(plain, full))

    def models():
        return [common.IsingModel(np.arange(J.shape[0], dtype=np.uint64) * 3 + 1, None, sa.Hamiltonian(J, h), None)
                for J, h in problems]

    rng = np.random.default_rng(5)
    frozen = []
    for J, _ in problems:
        n = J.shape[0]
        frozen.append((np.sort(rng.choice(n, size=n // 3, replace=False)) * 3 + 1).astype(np.uint64))
    frozen[0] = None
    got = common.solve_ising_models(models(), frozen, seed=9, method="tempering-cluster", number_sweeps=60,
                                    repetitions=8, sweep_order=order)
    want = sa.parallel_tempering_cluster_batch([m.ising_hamiltonian for m in models()], seed=9, number_rounds=6,
                                               sweeps_per_round=10, repetitions=8, only_best=True, sweep_order=order)
    assert len(got) == 3
    for model, x, (wx, _), f in zip(models(), got, want, frozen):
        assert np.array_equal(x, common._project_on_frozen(model, wx, f))


def test_an_error_of_one_item_changes_nothing(batch):
    """Validation that needs live handles: every item is checked before any device work and before any
    output is written, and the message names the item."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    names = [s.name for s in batch.specs]
    which = [names.index("K=65"), names.index("K=2049"), names.index("tie")]
    handles = batch.open(which)
    try:
        keep = []

        def items_of(pairs_of, chains_of=None, flags=(0, 0, 0)):
            items = (_lib.SaChainsClusterItem * 3)()
            outputs = []
            for i in range(3):
                pairs = pairs_of[i]
                count = 0 if pairs is None else len(pairs) // 2
                outs = (np.full(2, 77, dtype=np.uint32), np.full(2, 77, dtype=np.uint32), np.full(2, -77, dtype=np.int64))
                keep.append((pairs, outs))
                items[i].chains = (chains_of or handles)[i]._live()
                items[i].pairs = None if pairs is None else pairs.ctypes.data
                items[i].num_pairs = 2 if pairs is None else count
                items[i].draw = 0
                items[i].flags = flags[i]
                items[i].out_differing, items[i].out_size, items[i].out_delta = (o.ctypes.data for o in outs)
                outputs.append(outs)
            return items, outputs

        u32 = lambda *v: np.array(v, dtype=np.uint32)
        good = [u32(3, 0, 1, 4), u32(0, 1, 3, 2), u32(0, 1, 2, 3)]

        def refused(items, outputs, *words):
            assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(3)) == INVALID
            message = _lib.last_error()
            for word in words:
                assert word in message, message
            for outs in outputs:
                assert np.all(outs[0] == 77) and np.all(outs[1] == 77) and np.all(outs[2] == -77)
            for k, chains in zip(which, handles):
                _same_state(chains.state(), batch.specs[k].start, batch.specs[k].name)

        # a slot named twice in item 2 of 3
        refused(*items_of(good[:2] + [u32(0, 1, 2, 0)]), "item 2", "pairs[0]", "pairs[3]")
        # a slot that is not one of the chains; null pairs; unknown flags
        refused(*items_of([good[0], u32(0, 1, 3, 4), good[2]]), "item 1", "pairs[3]")
        refused(*items_of([good[0], None, good[2]]), "item 1", "null pairs")
        refused(*items_of(good, flags=(0, 1, 2)), "item 2", "flags")
        # the same handle twice; two handles of one plan
        refused(*items_of(good, chains_of=[handles[0], handles[1], handles[0]]), "items 0 and 2", "same handle")
        from annealing_sign_problem_amd import annealer as sa

        with sa.Chains(batch.hams[which[1]], seed=1, repetitions=4) as twin:
            refused(*items_of(good, chains_of=[handles[0], handles[1], twin]), "items 1 and 2", "one plan")
        # and the valid batch still runs: what the law says
        items, outputs = items_of([u32(*batch.specs[k].pairs.ravel()) for k in which])
        for i, k in enumerate(which):
            items[i].draw = batch.specs[k].draw
        assert lib.asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(3)) == 0
        batch.check(which, handles, [tuple(o[:len(batch.specs[k].pairs)] for o in outs)
                                     for k, outs in zip(which, outputs)])
    finally:
        _close(handles)
