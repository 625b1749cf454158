"""The device tree of the greedy solver (asp_sa_greedy_tree; csrc/greedy_tree.hip) against
the host tree (asp_sa_greedy_tree_host), WORD FOR WORD: every named case of tests/greedy_tree_cases.py in
both forest placements, alone and batched; the greedy solves with the device tree against the host
tree's; the Python keywords and the driver's flag."""
import ctypes

import numpy as np
import pytest

import greedy_tree_cases as cases

pytestmark = pytest.mark.gpu

NAMES = sorted(cases.CASES)


@pytest.fixture(scope="module")
def hamiltonians():
    """One Hamiltonian (and device plan) per named case, shared by the tests of this module."""
    from annealing_sign_problem_amd import annealer as sa

    made = {name: sa.Hamiltonian(*cases.case(name)) for name in NAMES}
    yield made
    for ham in made.values():
        ham.release()


def _device_tree(ham, where):
    """asp_sa_greedy_tree on the plan with asp_sa_set_greedy_tree(where): the words."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    words = (ham.size + 63) // 64
    x = np.full(max(words, 1), 0xABCDABCDABCDABCD, dtype=np.uint64)
    _lib.check(lib.asp_sa_set_greedy_tree(ham.plan(), ctypes.c_int(where)))
    try:
        _lib.check(lib.asp_sa_greedy_tree(ham.plan(), _lib.ptr(x)))
    finally:
        _lib.check(lib.asp_sa_set_greedy_tree(ham.plan(), ctypes.c_int(0)))
    return x[:words]


@pytest.mark.parametrize("where", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_device_tree_equals_host_tree(hamiltonians, name, where):
    got = _device_tree(hamiltonians[name], where)
    want = cases.reference(name)
    assert got.shape == want.shape and np.array_equal(got, want), (name, where, int((got != want).sum()))
    if name in cases.EXPECTED_WORDS:
        assert int(got[0]) == cases.EXPECTED_WORDS[name]


def test_the_setting_is_clamped_and_an_empty_plan_is_left_alone(hamiltonians):
    import scipy.sparse

    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    lib = _lib.load()
    ham = hamiltonians["k130"]
    for where in (-5, 7):  # clamped to 0 and 2: the tree call itself builds the device tree either way
        _lib.check(lib.asp_sa_set_greedy_tree(ham.plan(), ctypes.c_int(where)))
        x = np.zeros(3, dtype=np.uint64)
        _lib.check(lib.asp_sa_greedy_tree(ham.plan(), _lib.ptr(x)))
        assert np.array_equal(x, cases.reference("k130"))
    _lib.check(lib.asp_sa_set_greedy_tree(ham.plan(), ctypes.c_int(0)))
    assert lib.asp_sa_greedy_tree_last_ms() > 0.0
    empty = sa.Hamiltonian(scipy.sparse.csr_matrix((0, 0)), np.zeros(0))
    x = np.full(1, 0xABCDABCDABCDABCD, dtype=np.uint64)
    _lib.check(lib.asp_sa_greedy_tree(empty.plan(), _lib.ptr(x)))
    assert x[0] == np.uint64(0xABCDABCDABCDABCD)  # K = 0: nothing runs, out_x untouched
    # the same plan twice, with real plans
    plans = (ctypes.c_void_p * 2)(ham.plan(), ham.plan())
    a, b = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    outs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
    assert lib.asp_sa_greedy_tree_batch(plans, ctypes.c_uint32(2), outs) == -3
    assert "items 0 and 1" in _lib.last_error() and not a.any() and not b.any()
    empty.release()


@pytest.mark.parametrize("where", ["device", "device-hbm"])
def test_batch_equals_the_single_calls_for_any_order_and_composition(hamiltonians, where):
    from annealing_sign_problem_amd import greedy

    def run(names):
        got = greedy.greedy_tree_batch([hamiltonians[n] for n in names], where=where)
        assert len(got) == len(names)
        for name, x in zip(names, got):
            assert np.array_equal(x, cases.reference(name)), (name, where, len(names))

    run(NAMES)
    run(NAMES[::-1])
    run(NAMES[::2])
    run(NAMES[1::3][::-1])
    run(["sparse_50000", "k1"])  # (forest in HBM and forest in LDS in one call)
    run(["sum_order"])
    rng = np.random.default_rng(3)
    run(list(rng.permutation(NAMES)[:9]))


# ---- the solves ------------------------------------------------------------------------------------------

SOLVE_SIZES = [100, 250, 400, 640, 900, 1200, 1500, 1800, 2100, 2400, 2700, 3000]


@pytest.fixture(scope="module")
def planted():
    """[(J, h)] of a dozen planted clusters of 100 .. 3000 spins, every third with a field."""
    from annealing_sign_problem_amd import synthetic

    rng = np.random.default_rng(17)
    out = []
    for k, n in enumerate(SOLVE_SIZES):
        J, h, _ = synthetic.planted_cluster(n, seed=300 + k, mean_degree=min(23.0, n / 4), frustrated_fraction=0.2)
        if k % 3 == 1:
            h = rng.normal(size=n) * np.abs(J.data).mean()
        out.append((J, h))
    return out


def _solve_batch(problems, trees, launch=None):
    """asp_sa_greedy_batch on fresh plans, plan i with the tree trees[i]: [(x, e, sweeps)]."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    hams = [sa.Hamiltonian(J, h) for J, h in problems]
    for k, ham in enumerate(hams):
        if launch and k in launch:  # a forced geometry: the item runs alone inside the call
            _lib.check(_lib.load().asp_sa_set_launch(ham.plan(), ctypes.c_int(1), ctypes.c_int(256)))
    got = sa.greedy_solve_batch(hams, return_sweeps=True, tree=list(trees))
    for ham in hams:
        ham.release()
    return got


def _same(a, b):
    assert len(a) == len(b)
    for k, ((x, e, t), (y, f, u)) in enumerate(zip(a, b)):
        assert np.array_equal(x, y) and e == f and t == u, k


def test_solves_do_not_depend_on_the_tree(planted):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import greedy

    n = len(planted)
    host = _solve_batch(planted, ["host"] * n)
    _same(_solve_batch(planted, ["device"] * n), host)
    tree_ms, _ = greedy.last_batch_ms()
    assert tree_ms > 0.0 and greedy.last_tree_ms()[0] > 0.0 and tree_ms >= greedy.last_tree_ms()[0]
    _same(_solve_batch(planted, ["device-hbm"] * n), host)
    _same(_solve_batch(planted, ["device" if k % 2 else "host" for k in range(n)]), host)  # a mixed batch
    # items that run alone: a forced geometry among shared items, and a batch of one
    _same(_solve_batch(planted, ["device"] * n, launch={2, 7}), _solve_batch(planted, ["host"] * n, launch={2, 7}))
    _same(_solve_batch(planted, ["device"] * n, launch={2, 7}), host)
    for k in (0, 4, 11):
        _same(_solve_batch(planted[k:k + 1], ["device"]), host[k:k + 1])
    # asp_sa_greedy honours the plan's setting: the same x, energy and (chunked) sweep count
    lib = _lib.load()
    for k in (1, 6):
        J, h = planted[k]
        results = []
        for where in (0, 1, 2):
            ham = sa.Hamiltonian(J, h)
            x = np.zeros((ham.size + 63) // 64, dtype=np.uint64)
            e = np.zeros(1)
            sweeps = ctypes.c_uint32(0)
            _lib.check(lib.asp_sa_set_greedy_tree(ham.plan(), ctypes.c_int(where)))
            _lib.check(lib.asp_sa_greedy(ham.plan(), ctypes.c_uint32(10000), _lib.ptr(x), _lib.ptr(e),
                                         ctypes.byref(sweeps)))
            ham.release()
            results.append((x, float(e[0]), int(sweeps.value)))
        _same(results[1:], [results[0]] * 2)
        assert np.array_equal(results[0][0], host[k][0]) and results[0][1] == host[k][1]
        x, e = sa.greedy_solve(sa.Hamiltonian(J, h), tree="device")
        assert np.array_equal(x, host[k][0]) and e == host[k][1]


def test_solve_ising_models_with_the_device_tree_equals_the_default(planted, monkeypatch):
    from annealing_sign_problem_amd import annealer as sa, common

    monkeypatch.delenv("ASP_GREEDY_TREE", raising=False)
    problems = planted[:6]

    def models():
        return [common.IsingModel(np.arange(J.shape[0], dtype=np.uint64) * 3 + 1, None, sa.Hamiltonian(J, h), None)
                for J, h in problems]

    frozen = [None] + [(np.arange(0, J.shape[0], 3, dtype=np.uint64) * 3 + 1) for J, _ in problems[1:]]
    default = common.solve_ising_models(models(), frozen, mode="greedy")
    device = common.solve_ising_models(models(), frozen, mode="greedy", tree="device")
    for a, b in zip(default, device):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    one = common.solve_ising_model(models()[3], mode="greedy", frozen_spins=frozen[3], tree="device")
    assert np.array_equal(one, default[3])
    monkeypatch.setenv("ASP_GREEDY_TREE", "device")  # what tree=None reads
    for a, b in zip(default, common.solve_ising_models(models(), frozen, mode="greedy")):
        assert np.array_equal(a, b)


def test_driver_output_is_byte_identical_with_the_device_tree(tmp_path, monkeypatch):
    import os

    from annealing_sign_problem_amd import sampled_components

    monkeypatch.delenv("ASP_GREEDY_TREE", raising=False)
    common_args = ["--model", "heisenberg_kagome_16", "--order", "2", "--number-samples", "7", "--seed", "99",
                   "--max-cluster-size", "300", "--no-annealing", "--batch", "4", "--greedy-batch"]
    texts = {}
    for name, extra in [("host", []), ("device", ["--greedy-tree", "device"])]:
        out = tmp_path / (name + ".csv")
        sampled_components.main(common_args + ["--output", str(out)] + extra)
        texts[name] = out.read_bytes()
        assert "ASP_GREEDY_TREE" not in os.environ  # the flag does not outlive the run
    assert len(texts["host"].splitlines()) > 12 and texts["host"] == texts["device"]
