"""(no GPU) The models of tests/kloop_tail_cases.py have the blocks they are built for — read back from
asp_sa_layout_host —, so the GPU tests on them (tests/test_gpu_kloop_tail.py) cannot pass by missing an
end of the colour sweep's k-loop: every remainder of a block's longest row modulo 4, one to four quads,
odd and even, a block of width 1, blocks without couplings, a colour's last block with dummy lanes, and
a block whose longest row belongs to one lane only."""
import numpy as np
import pytest

import kloop_tail_cases as cases


@pytest.fixture(scope="module")
def plans():
    out = {}
    for name, make in cases.CASES.items():
        J, field = make()
        out[name] = (J, field) + cases.blocks(J, field)
    return out


def test_sizes(plans):
    for name, (J, field, longest, holders, live, last, info) in plans.items():
        assert 200 <= J.shape[0] <= 600, name
        assert np.all(field != 0.0), name
        assert int(((longest + 3) // 4 * 4).sum()) * 64 == info.ell_entries, name  # the widths are the plan's


def test_every_class_of_block_end_is_covered(plans):
    seen = set()
    for name, (J, field, longest, holders, live, last, info) in plans.items():
        seen |= cases.classes(longest, holders, live, last)
    assert not cases.REQUIRED - seen, "no block of: %s" % sorted(cases.REQUIRED - seen)


def test_each_model_has_what_it_is_named_for(plans):
    def of(name):
        _, _, longest, holders, live, last, info = plans[name]
        return list(zip(longest.tolist(), holders.tolist(), live.tolist())), info

    rows, info = of("ladder")
    assert info.num_colors == 2
    assert sorted(rows) == sorted([(16, 64, 64), (11, 64, 64), (6, 64, 64), (1, 64, 64)] * 2 + [(0, 64, 64), (0, 2, 2)])
    rows, info = of("short_rows")
    assert info.num_colors == 2
    assert sorted(rows) == sorted([(8, 64, 64), (5, 64, 64), (4, 64, 64), (3, 64, 64)] * 2)
    rows, info = of("single_lane")
    assert info.num_colors == 2
    assert sorted(rows) == sorted([(14, 1, 64), (2, 64, 64), (1, 1, 1)] * 2)


def test_the_ladder_ends_frozen(plans):
    """The schedule every GPU test runs: hot enough at first that most proposals are accepted, and sweeps
    at the end that accept nothing uphill."""
    for name, (J, field, longest, holders, live, last, info) in plans.items():
        betas = cases.betas_of(info)
        assert betas.shape[0] == cases.SWEEPS_HOT + cases.SWEEPS_FROZEN and 16 <= betas.shape[0] <= 24
        assert np.all(np.diff(betas) >= 0) and betas[0] == info.beta0_auto and betas[-1] == 1e12
