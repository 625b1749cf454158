"""The numpy restatement of the consensus vote (tests/vote_cases.py, law ASP-VOTE-1)
against a brute-force scalar loop written from the law's text, the planted cases against their truth, and
the order case against the two orders of summation it is there to tell apart.  No device."""
import numpy as np
import pytest

import vote_cases

SMALL = sorted(name for name, case in vote_cases.cases().items() if case["spins"] * case["xs"].shape[0] <= 20000)


def _scalar_law(case) -> dict:
    """ASP-VOTE-1 site by site and configuration by configuration, on Python integers and floats."""
    spins, xs, count = case["spins"], case["xs"], case["xs"].shape[0]

    def bit(words, i):
        return (int(words[i // 64]) >> (i % 64)) & 1

    weights = [1.0] * count if case["weights"] is None else [float(w) for w in case["weights"]]
    ref = [bit(xs[case["anchor"]] if case["ref"] is None else case["ref"], i) for i in range(spins)]
    for _ in range(case["rounds"]):
        distance = [sum(bit(xs[r], i) != ref[i] for i in range(spins)) for r in range(count)]
        flipped = [bool(case["align"]) and 2 * d > spins for d in distance]
        ones, plus, minus, c = [], [], [], []
        for i in range(spins):
            n, p, m = 0, 0.0, 0.0
            for r in range(count):
                if bit(xs[r], i) ^ int(flipped[r]):
                    n, p = n + 1, p + weights[r]
                else:
                    m = m + weights[r]
            ones.append(n)
            plus.append(p)
            minus.append(m)
            c.append(1 if p > m else 0 if p < m else ref[i])
        changed = sum(a != b for a, b in zip(c, ref))
        ref = c
    return {"distance": np.array(distance, dtype=np.uint32), "flipped": np.array(flipped, dtype=bool),
            "ones": np.array(ones, dtype=np.uint32), "plus": np.array(plus, dtype=np.float64),
            "minus": np.array(minus, dtype=np.float64),
            "x": vote_cases.pack(np.array(c, dtype=np.uint8)), "changed": changed}


def test_the_cases_cover_what_they_should():
    cases = vote_cases.cases()
    assert {c["spins"] for c in cases.values()} >= set(vote_cases.SPINS)
    assert {c["xs"].shape[0] for c in cases.values()} >= set(vote_cases.COUNTS)
    assert all(c["xs"].shape[0] <= 8 for c in cases.values() if c["spins"] > 4096)
    assert {c["rounds"] for c in cases.values()} >= {1, 2, 3}
    assert any(c["xs"].shape[1] > vote_cases.words_of(c["spins"]) for c in cases.values())
    assert len(SMALL) >= 40 and "order" in SMALL and "tie_takes_ref" in SMALL


@pytest.mark.parametrize("name", SMALL)
def test_restatement_is_the_scalar_loop(name):
    assert vote_cases.same(_scalar_law(vote_cases.cases()[name]), vote_cases.laws()[name]), name


def test_planted_truth_is_recovered_up_to_the_flip():
    checked = 0
    for name, case in vote_cases.cases().items():
        if case["truth"] is None:
            continue
        got = vote_cases.unpack(vote_cases.laws()[name]["x"], case["spins"])
        assert np.array_equal(got, case["truth"]) or np.array_equal(got, 1 - case["truth"]), name
        checked += 1
    assert checked >= 8


def test_hand_built_cases_do_what_they_are_built_for():
    laws, cases = vote_cases.laws(), vote_cases.cases()
    for name in laws:
        if name.startswith("flip_even"):  # K/2 stays, K/2 + 1 flips, K/2 - 1 stays
            assert laws[name]["flipped"].tolist() == [False, False, True, False], name
            half = cases[name]["spins"] // 2
            assert laws[name]["distance"].tolist() == [0, half, half + 1, half - 1], name
        if name.startswith("flip_odd"):
            assert laws[name]["flipped"].tolist() == [False, False, True], name
    for name in ("tie_takes_ref", "tie_takes_ref_weighted"):
        ref = vote_cases.unpack(cases[name]["ref"], 70)
        assert np.array_equal(vote_cases.unpack(laws[name]["x"], 70)[:40], ref[:40])
        assert np.array_equal(laws[name]["plus"][:40], laws[name]["minus"][:40])
        assert 0 < ref[:40].sum() < 40
    zero = laws["weights_all_zero"]
    assert zero["changed"] == 0 and not zero["plus"].any() and not zero["minus"].any()
    assert np.array_equal(zero["x"], vote_cases.pack(vote_cases.unpack(cases["weights_all_zero"]["xs"][3], 200)))
    assert not laws["align_off"]["flipped"].any() and laws["ref_is_truth"]["flipped"].any()  # (the same chains)
    # more rounds move on from a random reference and arrive at a fixed point
    assert laws["rounds1_random_ref"]["changed"] > 0 and laws["rounds16"]["changed"] == 0
    assert not np.array_equal(laws["rounds1_random_ref"]["x"], laws["rounds2_random_ref"]["x"])
    # the tail bits of the consensus are zero whatever the inputs carry there
    for name, law in laws.items():
        spins = cases[name]["spins"]
        if spins % 64:
            assert int(law["x"][-1]) >> (spins % 64) == 0, name


def test_order_case_tells_the_orders_apart():
    case = vote_cases.order_case()
    law = vote_cases.laws()["order"]
    assert law["plus"][0] == 2.0 ** 53 and law["minus"][0] == 2.0 ** 53 and int(law["x"][0]) == 0
    up = [w for w, b in zip(case["weights"], case["bits"]) if b]
    tree = (np.float64(up[0]) + np.float64(0.0)) + (np.float64(up[1]) + np.float64(up[2]))  # padded to four
    backwards = (np.float64(up[2]) + np.float64(up[1])) + np.float64(up[0])
    for other in (tree, backwards):
        assert other == 2.0 ** 53 + 2.0 and int(other > law["minus"][0]) == 1 != int(law["x"][0])
