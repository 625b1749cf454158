"""The shared cases of asp_sa_plan_create_segments (tests/plan_cases.py) against the host layout, without
a device: plan_front / plan_scales / plan_blocks / plan_fill restate what asp_sa_layout_host computes for
every rebased segment, and every case reaches the edge it is named for."""
import ctypes

import numpy as np
import pytest

import plan_cases as pc

ROUNDS = sorted(pc.rounds())


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def layout_host(seg):
    """(info, colors, positions) of asp_sa_layout_host for one segment."""
    from annealing_sign_problem_amd import _lib

    ip, ix, dv, h = seg
    n = ip.size - 1
    info = _lib.SaInfo()
    colors, positions = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
    _lib.check(_lib.load().asp_sa_layout_host(ctypes.c_uint64(n), _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv), _lib.ptr(h),
                                              ctypes.byref(info), _lib.ptr(colors), _lib.ptr(positions)))
    return info, colors, positions


@pytest.fixture(scope="module")
def restated():
    """name -> per segment (front, scales, blocks, fill, info), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            out = []
            for seg in pc.rounds()[name]:
                info, colors, positions = layout_host(seg)
                front = pc.plan_front(*seg)
                blocks = pc.plan_blocks(front["a_ptr"], colors, positions)
                fill = pc.plan_fill(front, positions, blocks["block_width"], blocks["ell_off"], seg[3])
                out.append((front, pc.plan_scales(front, seg[3]), blocks, fill, info, positions))
            cache[name] = out
        return cache[name]

    return get


@pytest.mark.parametrize("name", ROUNDS)
def test_restatements_equal_the_host_layout(name, restated):
    for seg, (front, scales, blocks, fill, info, positions) in zip(pc.rounds()[name], restated(name)):
        n = seg[0].size - 1
        assert info.num_spins == n
        assert info.nnz_offdiag == front["a_col"].size
        assert info.ell_entries == int(blocks["ell_off"][-1]) * 64
        assert info.num_blocks == blocks["num_blocks"]
        assert info.num_colors == blocks["num_colors"]
        assert info.max_degree == (int(np.diff(front["a_ptr"]).max()) if n else 0)
        assert info.energy_scale_exp == scales["energy_scale_exp"]
        for key in ("diag_sum", "beta0_auto", "beta1_auto"):
            assert _bits(getattr(info, key)) == _bits(scales[key]), key
        # the positions are a permutation into the padded order
        assert np.unique(positions).size == n
        assert np.array_equal(blocks["spin_of_pos"][positions], np.arange(n, dtype=np.uint32))
        assert np.count_nonzero(blocks["spin_of_pos"] != pc.DUMMY) == n
        if n:
            assert fill["ell_col"].size == info.ell_entries + pc.TAIL_SLABS * 64 == fill["ell_val"].size
            assert not fill["ell_col"][info.ell_entries:].any() and not fill["ell_val"][info.ell_entries:].any()
            assert int(fill["ell_col"][:info.ell_entries].max(initial=0)) < blocks["num_blocks"] * 64
            assert np.count_nonzero(fill["ell_val"]) == front["a_col"].size


def test_every_case_reaches_its_edge(restated):
    rounds = pc.rounds()
    sizes = {name: [s[0].size - 1 for s in rounds[name]] for name in rounds}
    assert sizes["empty_first_middle_last"] == [0, 9, 0, 0, 70, 0] and sizes["only_empty"] == [0, 0]
    assert sizes["one_spin"] == [1, 1] and restated("one_spin")[1][0]["has_diagonal"].tolist() == [True]
    assert sizes["isolated"] == [63, 64, 65, 130]
    for (front, _, blocks, _, info, _), blocks_expected in zip(restated("isolated"), (1, 1, 2, 3)):
        assert info.num_colors == 1 and info.num_blocks == blocks_expected and info.ell_entries == 0
        assert not blocks["block_width"].any()
    assert np.count_nonzero(restated("isolated")[0][2]["spin_of_pos"] == pc.DUMMY) == 1   # 63: one padding lane
    assert np.count_nonzero(restated("isolated")[2][2]["spin_of_pos"] == pc.DUMMY) == 63  # 65: 63 of them
    # colour classes of exactly 64 (one full block each) and 65 (a second block with one row)
    _, _, blocks, _, info, _ = restated("class_of_64")[0]
    assert info.num_colors == 2 and blocks["color_block_start"].tolist() == [0, 1, 2]
    assert np.count_nonzero(blocks["spin_of_pos"] == pc.DUMMY) == 0
    _, _, blocks, _, info, _ = restated("class_of_65")[0]
    assert info.num_colors == 2 and blocks["color_block_start"].tolist() == [0, 2, 4]
    assert blocks["block_width"].tolist() == [4, 4, 4, 4]
    # width rounding: degrees 1, 4, 5, 8, 9
    front = restated("widths")[0][0]
    assert sorted(set(np.diff(front["a_ptr"]).tolist())) == [1, 4, 5, 8, 9]
    assert 12 in restated("widths")[0][2]["block_width"].tolist()
    # the hub: one row of 300 entries, a width that is a multiple of 4 and not of 64
    front, _, blocks, _, info, _ = restated("hub_300")[0]
    assert info.max_degree == 300 and 300 in blocks["block_width"].tolist() and 300 % 64 != 0
    # the value edges
    values = dict(zip(pc.VALUE_SEGMENTS, restated("values")))
    assert values["diagonal"][0]["has_diagonal"].tolist() == [True, False, False, True, True]
    assert not values["no_diagonal"][0]["has_diagonal"].any()
    assert values["zeros"][0]["dropped"] == 6 and values["zeros"][0]["a_col"].size == 4
    assert values["zeros"][4].nnz_offdiag == 4
    assert 0.0 < np.abs(values["subnormal"][0]["a_val"]).min() < 2.3e-308
    front = values["value_asymmetric"][0]
    assert front["a_val"].tolist() == [0.1 + 0.2, -3.0 + 0.3, 0.2 + 0.1, 1e16 + 1.0, 0.3 + -3.0, 1.0 + 1e16]
    for name, entry in values.items():
        assert entry[0]["host_front"] == (name in pc.HOST_FRONT), name
    assert values["upper_triangular"][0]["a_col"].size == 8  # A has the entries that J lacks
    assert values["field"][1]["beta1_auto"] == np.log(100.0) / 2e-3
    assert values["value_edge"][0]["dropped"] == 6 and values["value_edge"][0]["has_diagonal"][2]
    # round shapes
    assert len(rounds["round_of_1"]) == 1 and len(rounds["round_of_3"]) == 3 and len(rounds["round_of_128"]) == 128
    assert min(sizes["round_of_128"]) == 1 and max(sizes["round_of_128"]) == 40
    assert restated("planted_20000")[0][4].num_blocks > 256
    info = restated("cubic_45000")[0][4]
    assert info.max_degree == 3 and info.num_spins == 45000
    # (the wide layout keeps 4 bytes per padded position in LDS: 45 000 spins cannot fit 160 KiB)
    assert info.num_blocks * 64 * 4 > 160 * 1024
    for name in rounds:  # everything else takes the device front
        if name != "values":
            assert not any(entry[0]["host_front"] for entry in restated(name)), name


@pytest.mark.parametrize("name", sorted(pc.CONTENT_ERRORS))
def test_content_errors_are_refused_by_the_host_layout(name):
    from annealing_sign_problem_amd import _lib

    good, bad, _ = pc.content_error_round(name)
    layout_host(good)
    with pytest.raises(_lib.AspError):
        layout_host(bad)
