"""The colour sweep's byte layout keeps replica m at bit 2m of a spin byte when a workgroup holds
at most four replicas (the sign of a term is then one shift-or); M = 8 keeps bit m.  The CPU test
checks that sign identity for every replica mask, the GPU tests run the byte layout forced
(no word layout) against the oracle."""
import numpy as np
import pytest

import oracle


def _even_encode(mask):
    return sum(((mask >> m) & 1) << (2 * m) for m in range(4))


def _multiplier(hi):
    return np.array([hi << 32], dtype=np.uint64).view(np.float64)[0]


@pytest.mark.parametrize("M", [1, 2, 4])
def test_even_bit_sign_identity_every_mask(M):
    """(byte << (31 - 2m)) | 0x3FF00000 is the high word of -1.0 when replica m's bit is set and
    of +1.0 otherwise, for every replica mask, exactly (low word 0)."""
    for mask in range(1 << M):
        byte = _even_encode(mask)
        assert byte < 256 and byte & 0xAA == 0
        for m in range(M):
            hi = ((byte << (31 - 2 * m)) & 0xFFFFFFFF) | 0x3FF00000
            expected = -1.0 if (mask >> m) & 1 else 1.0
            assert _multiplier(hi) == expected, (M, mask, m)


def test_dense_bits_need_more_than_one_instruction():
    """Why the encoding changed: with bit m = replica m the same shift-or is wrong for some
    (mask, m) — bit m - 1 lands on bit 30 of the high word."""
    wrong = 0
    for mask in range(16):
        for m in range(4):
            hi = ((mask << (31 - m)) & 0xFFFFFFFF) | 0x3FF00000
            if _multiplier(hi) != (-1.0 if (mask >> m) & 1 else 1.0):
                wrong += 1
    assert wrong > 0


def _stats(h, count):
    from annealing_sign_problem_amd import _lib

    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib.check(_lib.load().asp_sa_last_stats(h.plan(), count, _lib.ptr(tracked), _lib.ptr(accepted)))
    return tracked, accepted


def _byte_layout(ham, m, threads):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    _lib.check(lib.asp_sa_set_wide(ham.plan(), 0))
    _lib.check(lib.asp_sa_set_launch(ham.plan(), m, threads))


def _check(J, field, ham, seed, betas, reps, offset, x0):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    xs, es = sa.anneal_raw(ham, seed, betas, reps, offset, x0)
    assert _lib.load().asp_sa_last_layout(ham.plan()) == 0
    tracked, accepted = _stats(ham, reps)
    oxs, oes, otr, oacc = oracle.sa_anneal(J, field, seed, betas, reps, offset, x0,
                                           ham.info().energy_scale_exp, num_threads=8)
    assert np.array_equal(accepted, oacc), "accepted-flip counts differ"
    assert np.array_equal(tracked, otr), "tracked energies differ"
    assert np.array_equal(xs, oxs), "best configurations differ"
    assert es.tobytes() == oes.tobytes(), "energies differ"
    return oacc


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 4, 8])
@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("degree", [3.0, 9.0])
def test_byte_layout_bit_exact(m, with_x0, degree):
    """Rows of one, two, three ... quads (mean degree 3 and 9 give blocks of both quad-count
    parities), initial configurations from the seed and from x0."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    n = 2500
    J, h, _ = synthetic.planted_cluster(n, seed=int(degree) * 10 + m, mean_degree=degree)
    field = np.random.default_rng(m).normal(size=n) * 1e-3
    ham = sa.Hamiltonian(J, field)
    _byte_layout(ham, m, 256)
    info = ham.info()
    betas = sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 24)
    x0 = None
    if with_x0:
        x0 = sa.signs_to_bits(np.where(np.random.default_rng(3).random(n) < 0.5, -1.0, 1.0))
    _check(J, field, ham, 777 + m, betas, 2 * m + 3, 1, x0)


@pytest.mark.gpu
@pytest.mark.parametrize("m,threads", [(2, 256), (4, 1024)])
def test_byte_layout_field_cache_frozen_tail_and_reheat(m, threads):
    """The field cache (dirty and inert bytes, indexed by replica) through a frozen tail, a
    reheating and a second freeze."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(3000, seed=8)
    field = np.random.default_rng(13).normal(size=3000) * 1e-4
    freeze = np.geomspace(1.0, 1e12, 60)
    betas = np.concatenate([freeze, np.full(10, 1e12), np.geomspace(1e12, 2e2, 6),
                            np.geomspace(2e2, 1e12, 40), [1e3, 1e12, 1e12, 1e5, 1e12]])
    ham = sa.Hamiltonian(J, field)
    _byte_layout(ham, m, threads)
    oacc = _check(J, field, ham, 31, betas, 8, 2, None)
    assert oacc.min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("forced_m", [2, 4])
def test_byte_layout_batch(forced_m, monkeypatch):
    """A batch whose problems run the byte layout at two and four replicas per workgroup."""
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    monkeypatch.setenv("ASP_BATCH_M", str(forced_m))
    lib = _lib.load()
    problems = []
    for i, k in enumerate([90, 700, 2100, 5000, 64, 1300]):
        J, h, _ = synthetic.planted_cluster(k, seed=300 + i, mean_degree=4.0 + 3 * (i % 3))
        ham = sa.Hamiltonian(J, h)
        _lib.check(lib.asp_sa_set_wide(ham.plan(), 0))
        info = ham.info()
        problems.append(dict(J=J, h=h, ham=ham, seed=55 + i, reps=3 + 2 * i, offset=i % 2,
                             betas=sa.make_schedule(info.beta0_auto, min(info.beta1_auto, 1e6), 18),
                             S=info.energy_scale_exp))
    results = sa.anneal_batch_raw([p["ham"] for p in problems], [p["seed"] for p in problems],
                                  [p["betas"] for p in problems], [p["reps"] for p in problems],
                                  [p["offset"] for p in problems])
    for p, (xs, es) in zip(problems, results):
        tracked, accepted = _stats(p["ham"], p["reps"])
        oxs, oes, otr, oacc = oracle.sa_anneal(p["J"], p["h"], p["seed"], p["betas"], p["reps"],
                                               p["offset"], None, p["S"], num_threads=8)
        assert np.array_equal(xs, oxs) and es.tobytes() == oes.tobytes()
        assert np.array_equal(tracked, otr) and np.array_equal(accepted, oacc)
