"""GPU parity of the batched greedy solve (asp_sa_greedy_batch): every problem of a
batch against the CPU oracle's independent restatement AND against asp_sa_greedy on a fresh plan of
the same matrix — the same words, the same double, and sweep counts in the documented relation."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import oracle

pytestmark = pytest.mark.gpu

ASP_ERR_INVALID = -3
# synthetic.planted_cluster(n, seed=s), zero field, converges at t = 3, 5, 11, 27 (found on the CPU
# with oracle.greedy_solve(..., max_sweeps=k) for growing k); the tests assert t > 8 for the last two
PLANTED_T = [(200, 1), (2000, 2), (10000, 3), (30000, 4)]


def _problems():
    """(name, J, h) of the mixed batch: 2 .. 3e4 spins, with and without fields, frustrated and
    not, isolated spins, a single bond, twins, a tree that is a local minimum already."""
    from annealing_sign_problem_amd import synthetic

    rng = np.random.default_rng(2024)
    out = []
    for n, s in PLANTED_T:
        J, h, _ = synthetic.planted_cluster(n, seed=s)
        out.append(("planted_%d_%d" % (n, s), J, h))
    sizes = [3, 17, 64, 65, 130, 333, 500, 777, 1000, 1500, 2200, 3000, 4100, 5000, 6000, 8000]
    for k, n in enumerate(sizes):
        J, h, _ = synthetic.planted_cluster(n, seed=100 + k, mean_degree=min(23.0, max(n / 2, 1.0)))
        out.append(("zero_field_%d" % n, J, h))
        J, h, _ = synthetic.planted_cluster(n, seed=200 + k, mean_degree=min(14.0, max(n / 2, 1.0)),
                                            frustrated_fraction=0.3)
        scale = np.abs(J.data).mean()
        out.append(("field_frustrated_%d" % n, J, rng.normal(size=n) * scale))
    J, h, _ = synthetic.planted_cluster(1200, seed=7, frustrated_fraction=0.0)
    out.append(("unfrustrated", J, h))  # the tree satisfies every bond: t = 1
    Jsk, hsk = synthetic.sk_cluster(500, degree=100, seed=6)
    out.append(("sk", Jsk, hsk))
    J, h, _ = synthetic.planted_cluster(250, seed=9)
    big = scipy.sparse.block_diag([J, scipy.sparse.diags(rng.normal(size=50))], format="csr")
    out.append(("isolated_spins", big, np.concatenate([h, rng.normal(size=50) * 1e-3])))
    out.append(("single_bond", scipy.sparse.csr_matrix(np.array([[0.0, 0.75], [0.75, 0.0]])), np.zeros(2)))
    out.append(("single_bond_in_many", scipy.sparse.csr_matrix(([-0.5, -0.5], ([3, 90], [90, 3])), shape=(100, 100)),
                np.zeros(100)))
    J, h, _ = synthetic.planted_cluster(900, seed=11)
    out.append(("twin_a", J, h))
    out.append(("twin_b", J.copy(), h.copy()))
    assert len(out) >= 40
    return out


def _single(J, h, max_sweeps=10000):
    """asp_sa_greedy on a fresh plan: (x, e, out_sweeps)."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    ham = sa.Hamiltonian(J, h)
    words = (ham.size + 63) // 64
    x = np.zeros(max(words, 1), dtype=np.uint64)
    e = np.zeros(1)
    sweeps = ctypes.c_uint32(0)
    _lib.check(_lib.load().asp_sa_greedy(ham.plan(), ctypes.c_uint32(max_sweeps), _lib.ptr(x), _lib.ptr(e),
                                         ctypes.byref(sweeps)))
    ham.release()
    return x[:words], float(e[0]), int(sweeps.value)


def _batch(problems, max_sweeps=10000, prepare=None):
    """greedy_solve_batch on fresh plans: [(x, e, t)]."""
    from annealing_sign_problem_amd import annealer as sa

    hams = [sa.Hamiltonian(J, h) for _, J, h in problems]
    if prepare is not None:
        prepare(hams)
    got = sa.greedy_solve_batch(hams, max_sweeps=max_sweeps, return_sweeps=True)
    for ham in hams:
        ham.release()
    return got


def _chunks(t, max_sweeps=10000):
    """What asp_sa_greedy reports when t sweeps converged (asp.h)."""
    return min(max_sweeps, 8 * (-(-(t - 1) // 8) + 1))


@pytest.fixture(scope="module")
def solved():
    """The mixed batch solved three ways: oracle, one asp_sa_greedy each, one batch."""
    problems = _problems()
    reference = [oracle.greedy_solve(J, h) for _, J, h in problems]
    single = [_single(J, h) for _, J, h in problems]
    batch = _batch(problems)
    return problems, reference, single, batch


def test_mixed_batch_equals_oracle_and_single_calls(solved):
    from annealing_sign_problem_amd import annealer as sa

    problems, reference, single, batch = solved
    for (name, J, h), (ox, oe), (sx, se, _), (bx, be, _) in zip(problems, reference, single, batch):
        assert np.array_equal(bx, ox) and be == oe, name
        assert np.array_equal(bx, sx) and np.float64(be).tobytes() == np.float64(se).tobytes(), name
        ham = sa.Hamiltonian(J, h)
        assert ham.energy(bx) == be, name
        ham.release()


def test_results_do_not_depend_on_order_or_composition(solved):
    problems, _, _, batch = solved
    backwards = _batch(problems[::-1])[::-1]
    half = len(problems) // 2
    split = _batch(problems[:half]) + _batch(problems[half:])
    for (name, _, _), (bx, be, bt), (rx, re, rt), (px, pe, pt) in zip(problems, batch, backwards, split):
        assert np.array_equal(bx, rx) and be == re and bt == rt, name
        assert np.array_equal(bx, px) and be == pe and bt == pt, name


def test_sweep_counts_are_exact_and_match_the_chunked_single_path(solved):
    problems, _, single, batch = solved
    counts = {name: t for (name, _, _), (_, _, t) in zip(problems, batch)}
    for (name, _, _), (_, _, chunks), (_, _, t) in zip(problems, single, batch):
        print(name, "t =", t, "asp_sa_greedy sweeps =", chunks)
        assert t >= 1 and chunks == _chunks(t), name
    # more than one chunk of the single path is exercised
    assert counts["planted_10000_3"] > 8 and counts["planted_30000_4"] > 8
    assert [counts["planted_%d_%d" % ns] for ns in PLANTED_T] == [3, 5, 11, 27]
    assert counts["unfrustrated"] == 1  # the tree is a local minimum already
    # t is the FIRST sweep that flips nothing: capped one below, the result differs or t is not reached
    for (name, J, h), (bx, _, t) in zip(problems, batch):
        if t >= 2:
            assert not np.array_equal(oracle.greedy_solve(J, h, max_sweeps=t - 2)[0], bx), name


@pytest.mark.parametrize("cap", [0, 1, 4, 9])
def test_capped_descents_equal_the_oracle_with_the_same_cap(solved, cap):
    problems, _, _, batch = solved
    pick = [i for i, (name, _, _) in enumerate(problems)
            if name.startswith("planted_") or name in ("unfrustrated", "sk", "isolated_spins", "single_bond")]
    some = [problems[i] for i in pick]
    capped = _batch(some, max_sweeps=cap)
    below = 0
    for i, (name, J, h), (x, e, t) in zip(pick, some, capped):
        ox, oe = oracle.greedy_solve(J, h, max_sweeps=cap)
        assert np.array_equal(x, ox) and e == oe, name
        full_t = batch[i][2]
        assert t == min(cap, full_t), name
        below += cap < full_t
        if cap == 0:
            tx, te = oracle.greedy_solve(J, h, relax=False)
            assert np.array_equal(x, tx) and e == te, name
    assert below >= 2  # the cap bites for the planted clusters with t = 11 and 27 at least


def test_single_path_items_batch_of_one_empty_batch_and_empty_plan(solved):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    problems, reference, _, batch = solved
    lib = _lib.load()
    names = [name for name, _, _ in problems]
    pick = [names.index(n) for n in ("planted_200_1", "planted_10000_3", "sk", "planted_2000_2", "twin_a")]
    some = [problems[i] for i in pick]

    def force_bits(hams):  # the t = 11 problem runs alone, bit-packed, inside the batch
        _lib.check(lib.asp_sa_set_packed(hams[1].plan(), 1))

    for cap in (10000, 9):
        mixed = _batch(some, max_sweeps=cap, prepare=force_bits)
        for i, (name, J, h), (x, e, t) in zip(pick, some, mixed):
            ox, oe = oracle.greedy_solve(J, h, max_sweeps=cap)
            assert np.array_equal(x, ox) and e == oe, name
            assert t == min(cap, batch[i][2]), name
    # a batch of one takes the single path
    for i in pick[:2]:
        (x, e, t), = _batch([problems[i]])
        assert np.array_equal(x, reference[i][0]) and e == reference[i][1] and t == batch[i][2]
    # nothing to do
    assert sa.greedy_solve_batch([]) == []
    assert lib.asp_sa_greedy_batch(None, ctypes.c_uint32(0)) == 0
    # a plan without spins among others
    empty = ("empty", scipy.sparse.csr_matrix((0, 0)), np.zeros(0))
    got = _batch([problems[pick[0]], empty, problems[pick[3]]])
    assert got[1][0].shape == (0,) and got[1][1] == 0.0 and got[1][2] == 0
    for k, i in ((0, pick[0]), (2, pick[3])):
        assert np.array_equal(got[k][0], reference[i][0]) and got[k][1] == reference[i][1]


def test_refusals_name_the_item_and_write_nothing(solved):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    problems = solved[0][4:8]
    lib = _lib.load()
    hams = [sa.Hamiltonian(J, h) for _, J, h in problems]
    n = len(hams)

    def attempt(edit):
        items = (_lib.SaGreedyItem * n)()
        xs = [np.full((h.size + 63) // 64, 0xABCDABCDABCDABCD, dtype=np.uint64) for h in hams]
        es = np.full(n, -777.25)
        sweeps = np.full(n, 4242, dtype=np.uint32)
        for i, h in enumerate(hams):
            items[i].plan = h.plan()
            items[i].max_sweeps = 100
            items[i].flags = 0
            items[i].out_x = xs[i].ctypes.data
            items[i].out_e = es.ctypes.data + 8 * i
            items[i].out_sweeps = sweeps.ctypes.data + 4 * i
        edit(items)
        rc = lib.asp_sa_greedy_batch(items, ctypes.c_uint32(n))
        message = _lib.last_error()
        assert rc == ASP_ERR_INVALID, (rc, message)
        assert all(np.all(x == np.uint64(0xABCDABCDABCDABCD)) for x in xs)
        assert np.all(es == -777.25) and np.all(sweeps == 4242)
        return message

    def shared_plan(items):
        items[3].plan = items[1].plan

    def null_energy(items):
        items[2].out_e = None

    def null_configuration(items):
        items[3].out_x = None

    def unknown_flag(items):
        items[2].flags = 2

    def null_plan(items):
        items[1].plan = None

    message = attempt(shared_plan)
    assert "1" in message and "3" in message and "share a plan" in message
    assert "item 2" in attempt(null_energy)
    assert "item 3" in attempt(null_configuration)
    message = attempt(unknown_flag)
    assert "item 2" in message and "flags" in message
    assert "item 1" in attempt(null_plan)
    # the same plans are fine afterwards
    got = sa.greedy_solve_batch(hams)
    for (x, e), (_, J, h) in zip(got, problems):
        ox, oe = oracle.greedy_solve(J, h)
        assert np.array_equal(x, ox) and e == oe
    with pytest.raises(ValueError):
        sa.greedy_solve_batch([hams[0], hams[0]])
    for h in hams:
        h.release()


def test_solve_ising_models_greedy_equals_the_loop_with_frozen_spins(solved):
    from annealing_sign_problem_amd import annealer as sa, common

    rng = np.random.default_rng(5)
    problems = solved[0][8:20]

    def models():
        return [common.IsingModel(np.arange(J.shape[0], dtype=np.uint64) * 3 + 1, None, sa.Hamiltonian(J, h), None)
                for _, J, h in problems]

    frozen = []
    for _, J, _ in problems:
        n = J.shape[0]
        keep = np.sort(rng.choice(n, size=max(1, n // 3), replace=False))
        frozen.append((keep * 3 + 1).astype(np.uint64))
    frozen[0] = None
    looped = [common.solve_ising_model(m, mode="greedy", frozen_spins=f) for m, f in zip(models(), frozen)]
    batched = common.solve_ising_models(models(), frozen, mode="greedy")
    assert len(looped) == len(batched)
    for a, b in zip(looped, batched):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    with pytest.raises(ValueError):
        common.solve_ising_models(models()[:1], mode="descent")


def test_driver_output_is_byte_identical_with_greedy_batch(tmp_path):
    from annealing_sign_problem_amd import sampled_components

    common_args = ["--model", "heisenberg_kagome_16", "--order", "2", "--number-samples", "7",
                   "--seed", "99", "--max-cluster-size", "300", "--no-annealing", "--batch", "4"]
    texts = {}
    for name, extra in [("plain1", ["--jobs", "1"]), ("plain4", ["--jobs", "4"]),
                        ("batch1", ["--jobs", "1", "--greedy-batch"]),
                        ("batch4", ["--jobs", "4", "--greedy-batch"])]:
        out = tmp_path / (name + ".csv")
        sampled_components.main(common_args + ["--output", str(out)] + extra)
        texts[name] = out.read_text()
    assert len(texts["plain1"].splitlines()) > 12
    assert texts["plain1"] == texts["plain4"] == texts["batch1"] == texts["batch4"]
