"""The vote over the configurations RESIDENT in chains handles (asp_sa_chains_vote_batch,
annealer.Chains.consensus / consensus_chains; law ASP-VOTE-1) on planted clusters of 65,
300 and 3000 spins with 2, 64 and 65 chains: equal, bit for bit, to the numpy restatement applied to what
the handle exports, one handle at a time and the three in one call, a handle named twice, the handle
untouched by the call, and the default alignment of a model with a field."""
import ctypes

import numpy as np
import pytest

import vote_cases

pytestmark = pytest.mark.gpu

SHAPES = ((65, 2), (300, 64), (3000, 65))  # (spins, chains)


@pytest.fixture(scope="module")
def problems():
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    out = []
    for k, (spins, chains) in enumerate(SHAPES):
        J, h, planted = synthetic.planted_cluster(spins, seed=40 + k)
        ham = sa.Hamiltonian(J, h)
        info = ham.info()
        out.append({"ham": ham, "spins": spins, "chains": chains, "planted": planted,
                    "betas": sa.make_schedule(info.beta0_auto, info.beta1_auto, 30),
                    "weights": vote_cases.make_weights("lognormal", chains, np.random.default_rng(k))})
    yield out
    for p in out:
        p["ham"].release()


def _annealed(p, seed=11, sweeps=20):
    from annealing_sign_problem_amd import annealer as sa

    chains = sa.Chains(p["ham"], seed=seed, repetitions=p["chains"])
    chains.advance(p["betas"][:sweeps], sweep_order="shuffled")
    return chains


def _exported(chains, which):
    return chains.result()[0] if which == "best" else chains.state()["x_current"]


def _is_law(got, chains, which, weights, anchor, align, rounds, p):
    xs = _exported(chains, which)
    if anchor is None:
        anchor = int(np.argmin(chains.result()[1]))
    law = vote_cases.vote_law(p["spins"], xs, weights, None, anchor, align, rounds)
    assert vote_cases.same(got, law)
    assert np.float64(got.energy).view(np.uint64) == np.float64(p["ham"].energy(law["x"])).view(np.uint64)


@pytest.mark.parametrize("which", ["best", "current"])
def test_consensus_of_resident_chains_is_the_law_on_the_export(problems, which):
    for p in problems:
        with _annealed(p) as chains:
            _is_law(chains.consensus(which=which), chains, which, None, None, True, 1, p)
            _is_law(chains.consensus(p["weights"], which, anchor=p["chains"] - 1, rounds=2), chains, which,
                    p["weights"], p["chains"] - 1, True, 2, p)
            _is_law(chains.consensus(p["weights"], which, anchor=0, align=False), chains, which, p["weights"], 0,
                    False, 1, p)


def test_three_handles_in_one_call_and_a_handle_named_twice(problems):
    from annealing_sign_problem_amd import annealer as sa

    handles = [_annealed(p, seed=5 + k) for k, p in enumerate(problems)]
    try:
        weights = [p["weights"] for p in problems]
        for which in ("best", "current"):
            single = [c.consensus(w, which, anchor=1, rounds=2) for c, w in zip(handles, weights)]
            batch = sa.consensus_chains(handles, weights, which, anchor=1, rounds=2)
            for p, c, one, many in zip(problems, handles, single, batch):
                assert vote_cases.same(many, {name: getattr(one, name) for name in ("distance", "flipped", "ones",
                                                                                     "plus", "minus", "x", "changed")})
                assert many.energy == one.energy
                _is_law(many, c, which, p["weights"], 1, True, 2, p)
        # the same handle twice, with different arguments, between two others
        twice = sa.consensus_chains([handles[1], handles[0], handles[1], handles[2]],
                                    [None, None, weights[1], None], ["best", "best", "current", "current"],
                                    anchor=[None, 0, 3, None], rounds=[1, 1, 3, 1])
        _is_law(twice[0], handles[1], "best", None, None, True, 1, problems[1])
        _is_law(twice[1], handles[0], "best", None, 0, True, 1, problems[0])
        _is_law(twice[2], handles[1], "current", weights[1], 3, True, 3, problems[1])
        _is_law(twice[3], handles[2], "current", None, None, True, 1, problems[2])
    finally:
        for c in handles:
            c.close()


def test_a_vote_between_two_segments_leaves_the_chains_untouched(problems):
    from annealing_sign_problem_amd import annealer as sa

    p = problems[1]

    def run(voting: bool):
        with sa.Chains(p["ham"], seed=8, repetitions=p["chains"]) as chains:
            chains.advance(p["betas"][:15], sweep_order="shuffled")
            if voting:
                chains.consensus(p["weights"], "best", rounds=2)
                chains.consensus(which="current", anchor=5)
                sa.consensus_chains([chains, chains])
            chains.advance(p["betas"][15:], sweep_order="colour")
            state = chains.state()
            xs, es = chains.result()
        return state, xs, es

    plain, voted = run(False), run(True)
    assert set(plain[0]) == set(voted[0])
    for name in plain[0]:
        assert np.array_equal(plain[0][name], voted[0][name]), name
    assert np.array_equal(plain[1], voted[1]) and plain[2].tobytes() == voted[2].tobytes()


def test_a_field_turns_the_alignment_off_by_default(problems):
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import synthetic

    J, _, _ = synthetic.planted_cluster(300, seed=41)
    field = np.zeros(300)
    field[17] = 0.25
    ham = sa.Hamiltonian(J, field)
    p = dict(problems[1], ham=ham)
    try:
        with _annealed(p) as chains:
            # starts that are far apart: with the alignment on, some chains would flip
            got = chains.consensus(which="current", anchor=0)
            assert not got.flipped.any()
            _is_law(got, chains, "current", None, 0, False, 1, p)
            forced = chains.consensus(which="current", anchor=0, align=True)
            _is_law(forced, chains, "current", None, 0, True, 1, p)
    finally:
        ham.release()


def test_refusals_that_need_a_handle(problems):
    from annealing_sign_problem_amd import _lib
    from annealing_sign_problem_amd import annealer as sa

    p = problems[0]
    lib = _lib.load()
    with sa.Chains(p["ham"], seed=1, repetitions=3) as chains:
        before = chains.state()
        distance = np.full(3, 77, dtype=np.uint32)
        consensus = np.full(2, 77, dtype=np.uint64)
        wrong = np.array([1.0, np.nan, 1.0])

        def call(which=0, weights=None, anchor=0, rounds=1):
            items = (_lib.SaChainsVoteItem * 2)()
            for k, item in enumerate(items):
                item.chains, item.rounds = chains._live(), 1
            items[1].which, items[1].anchor, items[1].rounds = which, anchor, rounds
            items[1].weights = None if weights is None else weights.ctypes.data
            items[0].out_distance, items[0].out_consensus = distance.ctypes.data, consensus.ctypes.data
            return lib.asp_sa_chains_vote_batch(items, ctypes.c_uint32(2)), _lib.last_error()

        for arguments in (dict(which=2), dict(weights=wrong), dict(anchor=3), dict(rounds=0), dict(rounds=17)):
            rc, message = call(**arguments)
            assert rc == -3 and "item 1" in message, arguments
        assert np.all(distance == 77) and np.all(consensus == 77)
        with pytest.raises(ValueError):
            chains.consensus(which="first")
        with pytest.raises(ValueError):
            chains.consensus(weights=np.ones(4))
        after = chains.state()
        assert all(np.array_equal(before[name], after[name]) for name in before)
