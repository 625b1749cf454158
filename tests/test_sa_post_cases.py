"""(no GPU) The clusters of tests/sa_post_cases.py have the structure they are named for — read back
from asp_sa_layout_host —, so the GPU tests on them cannot pass by missing a path; and the CPU oracle's
energy is the plain E = s^T J s + h^T s on every one of them."""
import numpy as np
import pytest

import oracle
import sa_post_cases as cases


@pytest.fixture(scope="module")
def layouts():
    out = {}
    for name, make in cases.CASES.items():
        J, field = make()
        out[name] = (J, field) + cases.layout(J, field)
    return out


def _blocks(position):
    return np.unique(position // 64).shape[0]


def test_widths_account_for_the_whole_ell(layouts):
    """The widths the tests reason with are the plan's: they add up to its ELL size."""
    for name, (J, field, colour, position, width, info) in layouts.items():
        assert width.shape[0] == info.num_blocks == _blocks(position), name
        assert int(width.sum()) * 64 == info.ell_entries, name


def test_small_cases(layouts):
    blocks = {name: layouts[name][5].num_blocks for name in layouts}
    colours = {name: layouts[name][5].num_colors for name in layouts}
    assert blocks["K1"] == 1 and colours["K1"] == 1              # one block, 63 dummy lanes
    assert blocks["K63"] == 2 and colours["K63"] == 2            # dummy lanes in both blocks
    assert blocks["K64"] == 1 and colours["K64"] == 1            # one full block, no dummy lane
    assert blocks["K65"] == 2 and colours["K65"] == 1            # a full block and a single live lane
    assert blocks["K130"] >= 3 and colours["K130"] >= 3
    assert list(layouts["K1"][4]) == [0] and list(layouts["K64"][4]) == [0]
    assert list(layouts["K63"][4]) == [4, 4]
    assert set(layouts["K130"][4]) == {4}


def test_width_ladder_has_every_quad_count(layouts):
    """Blocks of 0, 1, 2, 3, 4 and 5 quads: the empty block, odd and even counts — the k-loop's two-quad
    body runs 0, 1 and 2 times and ends on one quad and on two."""
    J, field, colour, position, width, info = layouts["ladder"]
    assert J.shape[0] == 64 * 2 * len(cases.LADDER_DEGREES) + cases.LADDER_ISOLATED
    assert set(width) == {0, 4, 8, 12, 16, 20}, sorted(width)
    assert info.num_colors == 2
    # every width of the ladder in both colours (the empty block in the first only)
    for c in range(2):
        of_colour = set(width[np.unique(position[colour == c] // 64)])
        assert of_colour >= {4, 8, 12, 16, 20}, (c, sorted(of_colour))


def test_large_case_folds_in_two_levels(layouts):
    J, field, colour, position, width, info = layouts["large"]
    assert info.num_blocks > 64 and info.num_blocks % 64 != 0, info.num_blocks
    assert info.num_blocks <= 64 * 64
    quads = set(width // 4)
    assert {q % 2 for q in quads} == {0, 1}, sorted(quads)  # even and odd quad counts


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_energy_is_the_plain_sum(name):
    """|E_oracle - (s^T J s + h^T s)| <= 1e-12 |s^T J s + h^T s|."""
    from annealing_sign_problem_amd import annealer as sa

    J, field = cases.CASES[name]()
    n = J.shape[0]
    xs = cases.configurations(n, 11)
    got = oracle.sa_energy(J, field, xs)
    for x, e in zip(xs, got):
        s = sa.bits_to_signs(x, n)
        plain = float(s @ (J @ s) + field @ s)
        assert abs(e - plain) <= 1e-12 * max(abs(plain), 1e-300), (name, e, plain)
