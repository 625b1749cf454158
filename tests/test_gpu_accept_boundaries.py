"""The acceptance rule at its decision boundaries, at every site it is compiled into (csrc/sa_device.hpp:
metropolis_accept_word — a hardware-exp filter in front of the exact expneg, promised to ALWAYS equal
`u < expneg(x)`): the colour sweep's body in every layout, group size, alignment and in tail sweeps, the
team sweep, the shuffled sweep, the ladder and segment forms of a handle, the batched call, both exchange
kernels, and the resampling weights, where expneg's value itself comes out.

The inputs are tests/accept_cases.py's: chosen (word, x) pairs — adjacent doubles on either side of a
decision, a ladder of distances across both edges of the filter's band, and edge values of x —;
tests/test_accept_cases.py counts them and shows, on the host, that they notice an exp one ulp off and a
band that is too narrow.  Every comparison is exact: configurations, energies, tracked energies and accepted
counts against oracle.sa_anneal / sa_anneal_shuffled, exchange steps against tests/tempering_law.py's steps
2-5 fed with the generator's words (on the host tests/test_accept_cases.py shows that this is
tempering_law.exchange for every step; the scalar Philox of that takes 0.1 s a step),
weights against tests/population_law.py.  On a mismatch the message names the first differing (spin,
chain), the x it presented (hex), its random word and the probe's class.

Every oracle run is made once per module and frozen."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

import accept_cases as ac
import oracle
import population_law
import tempering_law

pytestmark = pytest.mark.gpu

ALWAYS = 2 ** 31 - 1
WORDS, BYTES, BITS, HBM, TEAM, SHUFFLED = 2, 0, 1, 3, 4, 5  # asp_sa_last_layout's codes
_references = {}


def _lib():
    from annealing_sign_problem_amd import _lib

    return _lib


def _sa():
    from annealing_sign_problem_amd import annealer

    return annealer


def _reference(name, random_start=False):
    """{beta: the oracle's (xs, es, tracked, accepted) of all chains of the case at that beta}."""
    key = (name, random_start)
    if key not in _references:
        case = ac.sweep_case(name)
        anneal = oracle.sa_anneal if case.order == "colour" else oracle.sa_anneal_shuffled
        scale = ac.host_scale(case)[0]
        _references[key] = {
            float(beta): ac.freeze(*anneal(case.J, case.field, case.SEED, beta * case.betas, case.R, case.first,
                                           None if random_start else case.x0, scale, num_threads=8))
            for beta in np.unique(case.chain_betas)}
    return _references[key]


def _expected(name, lo=0, count=None, random_start=False):
    """The reference of chains lo .. lo + count of the case, every chain at its own beta."""
    case = ac.sweep_case(name)
    count = case.R - lo if count is None else count
    runs = _reference(name, random_start)
    rows = np.arange(lo, lo + count)
    return [np.stack([runs[float(case.chain_betas[r])][part][r] for r in rows]) for part in range(4)]


def _spins(xs, size):
    return np.unpackbits(np.ascontiguousarray(xs).view(np.uint8), axis=1, bitorder="little")[:, :size]


def _assert_same(case, got, want, what, lo=0):
    got_bits, want_bits = _spins(got[0], case.size), _spins(want[0], case.size)
    if not np.array_equal(got_bits, want_bits):
        spin, chain = (int(v) for v in np.argwhere((got_bits != want_bits).T)[0])
        if spin < case.K:
            x, word, name = case.presented(spin, lo + chain)
            detail = "x = %s, word %d (%s probe; its designated chain is %d), the oracle %s" % (
                x.hex(), word, name, case.designated[spin], "rejects" if want_bits[chain, spin] else "accepts")
        else:
            detail = "the gate" if spin == case.gate else "the gate's helper"
        diff = (got_bits != want_bits)[:, :case.K]
        d = case.designated - lo
        aimed = (d >= 0) & (d < len(diff))
        hit = diff[d[aimed], np.arange(case.K)[aimed]]
        by_class = ", ".join("%d %s" % (int(hit[case.probes.cls[aimed] == c].sum()), ac.CLASS_NAMES[c]) for c in range(3))
        raise AssertionError("%s: %d decisions differ (%s, %d random), first at (spin %d, chain %d): %s" % (
            what, int(diff.sum()), by_class, int(diff.sum() - hit.sum()), spin, lo + chain, detail))
    for g, w, name in zip(got[1:], want[1:], ("energies", "tracked energies", "accepted counts")):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), "%s: %s differ" % (what, name)


def _launch(ham):
    lib = _lib().load()
    m, threads, groups = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib().check(lib.asp_sa_last_launch(ham.plan(), ctypes.byref(m), ctypes.byref(threads), ctypes.byref(groups)))
    return m.value, threads.value, groups.value


def _stats(ham, count):
    tracked = np.zeros(count, np.int64)
    accepted = np.zeros(count, np.uint64)
    _lib().check(_lib().load().asp_sa_last_stats(ham.plan(), count, _lib().ptr(tracked), _lib().ptr(accepted)))
    return tracked, accepted


def _closed(case, ham, lo=0, count=None, shuffled=False):
    count = case.R - lo if count is None else count
    xs, es = _sa().anneal_raw(ham, case.SEED, case.betas, count, case.first + lo, case.x0, shuffled=shuffled)
    return (xs, es) + _stats(ham, count)


def _bytes_limit(blocks):
    """The LDS of the byte layout's sweep (csrc/sa_sweep.hip, sweep_lds_bytes; SweepLds in csrc/sa_colour.hpp): words do not fit it."""
    return blocks * 64 + 34 * 8 + blocks * 8 + 16 + 2 * ((blocks + 15) // 16 * 16)


# ---------------------------------------------------------------------------------------------
# Colour sweep, closed call
# ---------------------------------------------------------------------------------------------

# form: (case, replicas per group, lowered LDS limit, asp_sa_set_packed, asp_sa_set_tail, layout)
COLOUR_FORMS = {
    "m1_bytes": ("isolated", 1, False, 0, 0, BYTES),
    "m2_bytes": ("isolated", 2, False, 0, 0, BYTES),
    "m8_bytes": ("isolated", 8, False, 0, 0, BYTES),
    "m4_words_aligned": ("isolated", 4, False, 0, 0, WORDS),
    "m4_words_generic": ("isolated_from_3", 4, False, 0, 0, WORDS),
    "m4_bytes_aligned": ("isolated", 4, True, 0, 0, BYTES),
    "m4_bytes_generic": ("isolated_from_3", 4, True, 0, 0, BYTES),
    "bits_in_lds": ("isolated", 0, False, 1, 0, BITS),
    "bits_in_hbm": ("isolated", 0, False, 2, 0, HBM),
    "m4_words_tail": ("isolated", 4, False, 0, ALWAYS, WORDS),
    "m4_bytes_tail": ("isolated", 4, True, 0, ALWAYS, BYTES),
    "m4_words_pairs": ("pairs", 4, False, 0, 0, WORDS),
}


@pytest.mark.parametrize("form", sorted(COLOUR_FORMS))
def test_colour_closed_call(form):
    name, m, lowered, packed, tail, layout = COLOUR_FORMS[form]
    lib, case = _lib().load(), ac.sweep_case(name)
    ham = _sa().Hamiltonian(case.J, case.field)
    _lib().check(lib.asp_sa_set_launch(ham.plan(), m, 0))
    _lib().check(lib.asp_sa_set_packed(ham.plan(), packed))
    _lib().check(lib.asp_sa_set_team(ham.plan(), 0))
    if lowered:
        _lib().check(lib.asp_sa_set_lds_limit(ham.plan(), ctypes.c_uint64(_bytes_limit(ham.info().num_blocks))))
    _sa().set_tail(ham, tail)
    got = _closed(case, ham)
    assert lib.asp_sa_last_layout(ham.plan()) == layout
    assert _launch(ham)[0] == (m if m else 1)
    # sweep 1, the probing one, as a tail visit of every row — or no tail sweeps at all
    assert _sa().last_tail(ham) == ((1, 1, 1) if tail else (0, 0, 0))
    ham.release()
    _assert_same(case, got, _expected(name), form)


# ---------------------------------------------------------------------------------------------
# Team sweep
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("team,count", [(2, 64), (8, 16)])
def test_team_sweep(team, count):
    """k_sa_sweep_team on "pairs" (a team needs two colours), `count` chains a launch so that a launch's
    workgroups are resident together; the launches cover all chains of the case."""
    lib, case = _lib().load(), ac.sweep_case("pairs")
    ham = _sa().Hamiltonian(case.J, case.field)
    _lib().check(lib.asp_sa_set_team(ham.plan(), team))
    for lo in range(0, case.R, count):
        got = _closed(case, ham, lo, count)
        assert lib.asp_sa_last_layout(ham.plan()) == TEAM
        _assert_same(case, got, _expected("pairs", lo, count), "team of %d, chains from %d" % (team, lo), lo)
    ham.release()


# ---------------------------------------------------------------------------------------------
# Shuffled sweep
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,waves,teams", [(1, 1, 0), (4, 4, 0), (8, 2, 0), (4, 2, 2)])
@pytest.mark.parametrize("name", ["isolated_shuffled", "pairs_shuffled"])
def test_shuffled_sweep(name, m, waves, teams):
    lib, case = _lib().load(), ac.sweep_case(name)
    ham = _sa().Hamiltonian(case.J, case.field)
    _lib().check(lib.asp_sa_set_shuffled_launch(ham.plan(), m, waves))
    _lib().check(lib.asp_sa_set_shuffled_teams(ham.plan(), teams))
    got = _closed(case, ham, shuffled=True)
    assert lib.asp_sa_last_layout(ham.plan()) == SHUFFLED
    assert _launch(ham)[:2] == (m, 64 * waves * max(teams, 1))
    ham.release()
    _assert_same(case, got, _expected(name), "shuffled sweep (%d, %d), teams %d" % (m, waves, teams))


# ---------------------------------------------------------------------------------------------
# Handles: ladder and segments
# ---------------------------------------------------------------------------------------------

def _handle_outputs(chains):
    xs, es = chains.result()
    state = chains.state()
    assert np.array_equal(state["x_current"], xs), "the state after sweep 1 is not the best one"
    return xs, es, state["tracked_best"], state["accepted"]


@pytest.mark.parametrize("name", ["ladder", "ladder_shuffled"])
def test_ladder_segment(name):
    """Chains.advance_ladder: chain r at beta_r = 2^((r mod 3) - 1) (ladder.of in the sweep's body), the fields
    divided by the designated chain's beta."""
    lib, case = _lib().load(), ac.sweep_case(name)
    ham = _sa().Hamiltonian(case.J, case.field)
    _lib().check(lib.asp_sa_set_launch(ham.plan(), 4, 0))
    with _sa().Chains(ham, seed=case.SEED, repetitions=case.R, x0=case.x0, replica_offset=case.first) as chains:
        chains.advance_ladder(case.chain_betas, 2, sweep_order=case.order)
        assert lib.asp_sa_last_layout(ham.plan()) == (WORDS if case.order == "colour" else SHUFFLED)
        got = _handle_outputs(chains)
    ham.release()
    _assert_same(case, got, _expected(name), name)


@pytest.mark.parametrize("name", ["isolated", "isolated_from_3", "isolated_shuffled"])
def test_two_segments(name):
    """Chains.advance([1.0]) twice: sweep 1 is a segment of its own."""
    lib, case = _lib().load(), ac.sweep_case(name)
    ham = _sa().Hamiltonian(case.J, case.field)
    _lib().check(lib.asp_sa_set_launch(ham.plan(), 4, 0))
    with _sa().Chains(ham, seed=case.SEED, repetitions=case.R, x0=case.x0, replica_offset=case.first) as chains:
        for _ in range(2):
            chains.advance([1.0], sweep_order=case.order)
            assert lib.asp_sa_last_layout(ham.plan()) == (WORDS if case.order == "colour" else SHUFFLED)
        got = _handle_outputs(chains)
    ham.release()
    _assert_same(case, got, _expected(name), name)


# ---------------------------------------------------------------------------------------------
# Batched call
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["colour", "shuffled"])
def test_batched_call(order):
    """anneal_batch_raw of the two models in one call.  The batched call takes no start configuration: the
    chains start at random, a spin that starts up probes in sweep 0 with another word and most spins probe in
    sweep 1 as designed; the outputs are the oracle's all the same."""
    names = ["isolated", "pairs"] if order == "colour" else ["isolated_shuffled", "pairs_shuffled"]
    cases = [ac.sweep_case(name) for name in names]
    hams = [_sa().Hamiltonian(case.J, case.field) for case in cases]
    out = _sa().anneal_batch_raw(hams, [case.SEED for case in cases], [case.betas for case in cases],
                                 [case.R for case in cases], [case.first for case in cases], shuffled=order == "shuffled")
    for name, case, ham, (xs, es) in zip(names, cases, hams, out):
        # (the batch's launcher picks chains per workgroup and layout for the whole batch: bytes or words here)
        layout = _lib().load().asp_sa_last_layout(ham.plan())
        assert layout in ((SHUFFLED,) if order == "shuffled" else (WORDS, BYTES)), layout
        # (a chain whose helper starts up never turns its gate: its best state is an earlier one, and the
        # decisions of sweep 1 show in its accepted count alone)
        _assert_same(case, (xs, es) + _stats(ham, case.R), _expected(name, random_start=True),
                     "batched %s, %s" % (order, name))
        ham.release()


# ---------------------------------------------------------------------------------------------
# Exchange
# ---------------------------------------------------------------------------------------------

def _exchange_plan():
    return _sa().Hamiltonian(scipy.sparse.csr_matrix((1, 1)), np.array([0.5]))


def _explain_exchange(case, parity, draw, got, want):
    pairs, probes, betas = case.steps[parity, draw]
    j = int(np.nonzero(got[pairs] != want[pairs])[0][0])
    return "parity %d, draw %d: %d pairs differ, first pair %d: x = %s, word %d (%s probe), the law %s" % (
        parity, draw, int((got[pairs] != want[pairs]).sum()), pairs[j], float(probes.x[j]).hex(), probes.words[j],
        ac.CLASS_NAMES[probes.cls[j]], "accepts" if probes.accept[j] else "rejects")


def test_exchange_select():
    """k_exchange_select: one handle of 16384 chains, both parities, 24 draws each; every pair of every step is
    an aimed probe.  gather(source) undoes a step."""
    case = ac.exchange_case()
    ham = _exchange_plan()
    with _sa().Chains(ham, seed=case.SEED, repetitions=case.R, x0=case.x0) as chains:
        before = chains.state()
        # the whole law once with its own scalar Philox (for every step: tests/test_accept_cases.py)
        source, accepted = tempering_law.exchange(case.energies, case.steps[1, 3][2], 1, case.SEED, 0, 3)
        assert (source.tolist(), accepted) == (case.expected(1, 3)[0].tolist(), case.expected(1, 3)[1])
        for (parity, draw), (_, _, betas) in sorted(case.steps.items()):
            source, energies, accepted = chains.exchange(betas, parity, draw)
            want_source, want_accepted = case.expected(parity, draw)
            assert energies.tobytes() == case.energies.tobytes()
            assert np.array_equal(source, want_source), _explain_exchange(case, parity, draw, source, want_source)
            assert accepted == want_accepted
            chains.gather(source)
        after = chains.state()
    ham.release()
    for key in before:
        assert np.array_equal(before[key], after[key]), key


def test_exchange_select_batch():
    """k_exchange_select_batch: three handles on three plans (2, 257 and 4096 chains) in one call — the single
    calls, and the law."""
    cases = [ac.exchange_case(chains, (0, 1, 2, 3)) for chains in (2, 257, 4096)]
    hams = [_exchange_plan() for _ in cases]
    handles = [_sa().Chains(ham, seed=case.SEED, repetitions=case.R, x0=case.x0) for ham, case in zip(hams, cases)]
    for parity in (0, 1):
        for draw in (0, 1, 2, 3):
            ladders = [case.steps[parity, draw][2] for case in cases]
            single = []
            for handle, betas in zip(handles, ladders):
                single.append(handle.exchange(betas, parity, draw))
                handle.gather(single[-1][0])
            batch = _sa().exchange_chains(handles, ladders, parity, draw)
            for case, handle, one, (source, energies, accepted) in zip(cases, handles, single, batch):
                want_source, want_accepted = case.expected(parity, draw)
                assert np.array_equal(source, want_source), _explain_exchange(case, parity, draw, source, want_source)
                assert accepted == want_accepted and energies.tobytes() == case.energies.tobytes()
                assert np.array_equal(one[0], source) and one[2] == accepted and one[1].tobytes() == energies.tobytes()
                handle.gather(source)
    for handle, ham in zip(handles, hams):
        handle.close()
        ham.release()


# ---------------------------------------------------------------------------------------------
# Resample weights
# ---------------------------------------------------------------------------------------------

def test_resample_weights():
    """out_q = floor(expneg(gap) 2^31) at dbeta = 1 with gaps on either side of the steps of that floor."""
    field, x0, gaps = ac.weight_case()
    ham = _sa().Hamiltonian(scipy.sparse.csr_matrix((ac.WEIGHT_SPINS, ac.WEIGHT_SPINS)), field)
    R = len(gaps)
    with _sa().Chains(ham, seed=5, repetitions=R, x0=x0) as chains:
        items = (_lib().SaChainsResampleItem * 1)()
        source, energy, q = np.zeros(R, np.uint32), np.zeros(R), np.zeros(R, np.uint64)
        survivors = ctypes.c_uint32(0)
        items[0].chains = chains._live()
        items[0].dbeta, items[0].draw, items[0].flags = 1.0, 0, 0
        items[0].out_source, items[0].out_energy, items[0].out_q = source.ctypes.data, energy.ctypes.data, q.ctypes.data
        items[0].out_survivors = ctypes.addressof(survivors)
        _lib().check(_lib().load().asp_sa_chains_resample_batch(items, ctypes.c_uint32(1)))
    ham.release()
    assert np.array_equal(energy - energy.min(), gaps), "the energies are not the exact dyadics of the model"
    want = population_law.weights(energy, 1.0)
    wrong = np.nonzero(q != np.array(want, np.uint64))[0]
    assert wrong.size == 0, "%d weights differ, first at gap %s: %d, the law %d" % (
        wrong.size, float(gaps[wrong[0]]).hex(), q[wrong[0]], want[wrong[0]])
