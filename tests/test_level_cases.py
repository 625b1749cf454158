"""The laws of tests/level_cases.py without a device: every law equals oracle.sparsify_component or
operator_cases.extend segment by segment, every WRONG variant is told apart by at least one named case, and the
copies of a matrix scaled by 2^-30, 1 and 2^30 give equal masks (ASP-SPARSIFY-SEG-1's per-segment threshold).
tests/test_gpu_level_batch.py compares the kernels of csrc/level_segments.hip with the same laws on the same cases."""
import numpy as np
import pytest
import scipy.sparse

import level_cases
import operator_cases
import prep_cases


@pytest.mark.parametrize("name", level_cases.SPARSIFY_NAMES)
def test_sparsify_law_is_the_oracle_segment_by_segment(name):
    import oracle

    t = level_cases.sparsify_table(name)
    law = t.law()
    assert law[1][0] == 0 and law[1].shape == (len(t.segments) + 1,) and law[2][0] == 0
    # 4097 segments: every 37th, and the neighbours of the first and the last
    picked = range(len(t.segments)) if len(t.segments) < 100 else sorted(set(range(0, len(t.segments), 37)) | {1, 2, 4095, 4096})
    for g in picked:
        s = t.segments[g]
        keep, ip, col, val = level_cases.rebased(law, t.offsets, g)
        if s.size == 0:
            assert keep.size == 0 and ip.tolist() == [0] and col.size == 0
            continue
        want_keep, block = oracle.sparsify_component(s.matrix, s.frozen, t.reltol, s.anchor)
        block = scipy.sparse.csr_matrix(block)
        block.sort_indices()
        assert np.array_equal(keep, want_keep), (name, g)
        assert np.array_equal(ip, block.indptr) and np.array_equal(col, block.indices), (name, g)
        assert val.tobytes() == block.data.astype(np.float64).tobytes(), (name, g)
        # the restatement with the threshold handed in agrees at reltol * max|data|
        top = float(np.max(np.abs(s.matrix.data))) if s.matrix.data.size else 0.0
        assert np.array_equal(level_cases.keep_with_threshold(s.matrix, s.frozen, t.reltol * top, s.anchor), keep)


def test_the_stray_case_is_refused_with_the_first_segment_and_its_count():
    t = level_cases.sparsify_table(level_cases.STRAY)
    with pytest.raises(level_cases.Stray) as error:
        t.law()
    assert (error.value.segment, error.value.count) == (1, 1)
    with pytest.raises(level_cases.Stray) as error:
        t.law(table_wide_stray=True)
    assert (error.value.segment, error.value.count) == (None, 3)


@pytest.mark.parametrize("name", level_cases.SCALED)
def test_scaled_copies_give_equal_masks_and_a_shared_threshold_does_not(name):
    t = level_cases.sparsify_table("scaled: " + name)
    keep, kept_offsets = t.law()[:2]
    n = t.segments[0].size
    assert np.array_equal(keep[:n], keep[n:2 * n]) and np.array_equal(keep[:n], keep[2 * n:])
    assert np.diff(kept_offsets.astype(np.int64)).tolist() == [int(keep[:n].sum())] * 3 and 1 < keep[:n].sum() < n
    shared = t.law(shared_threshold=True)[0]
    assert np.array_equal(shared[2 * n:], keep[2 * n:])       # the largest copy sets the table's threshold
    assert shared[:n].sum() < keep[:n].sum() and shared[n:2 * n].sum() < keep[:n].sum()
    if name == "directed pairs":
        assert [int(shared[i * n:(i + 1) * n].sum()) for i in range(3)] == [1, 1, 320] and n == 400


SPARSIFY_TELLS = {
    "one threshold for the table": "scaled: directed pairs",
    "the anchor read as a global index": "one matrix, two anchors",
    "columns renumbered over the table": "boundaries in a workgroup",
    "the stray-frozen check made table-wide": level_cases.STRAY,
}


@pytest.mark.parametrize("variant", list(level_cases.SPARSIFY_VARIANTS))
def test_every_wrong_sparsify_variant_is_told_apart(variant):
    assert set(SPARSIFY_TELLS) == set(level_cases.SPARSIFY_VARIANTS)
    t = level_cases.sparsify_table(SPARSIFY_TELLS[variant])
    switches = level_cases.SPARSIFY_VARIANTS[variant]
    if t.name == level_cases.STRAY:
        with pytest.raises(level_cases.Stray) as right:
            t.law()
        with pytest.raises(level_cases.Stray) as wrong:
            t.law(**switches)
        assert (right.value.segment, right.value.count) != (wrong.value.segment, wrong.value.count)
    else:
        try:
            wrong = t.law(**switches)
        except level_cases.Stray:      # (the anchor of segment 1 read in segment 0: its frozen spin is stray)
            return
        assert not level_cases.same_result(wrong, t.law())


def test_the_sparsify_tables_hold_what_their_names_say():
    t = level_cases.sparsify_table("sizes 0 1 2 3 63 64 65 257")
    sizes = np.diff(t.offsets.astype(np.int64)).tolist()
    assert sorted(set(sizes)) == sorted(level_cases.SIZES) and sizes[0] == 0 and sizes[-1] == 0 and [0, 0] == sizes[4:6]
    t = level_cases.sparsify_table("boundaries in a workgroup")
    assert {int(o) % level_cases.ROWS_PER_BLOCK for o in t.offsets[1:-1]} == {0, 1, 2, 3}
    t = level_cases.sparsify_table("boundaries at the scan tile")
    tile = level_cases.SCAN_TILE
    assert t.offsets[1:4].tolist() == [tile - 1, tile, tile + 1]
    t = level_cases.sparsify_table("4097 segments of 1-3 spins")
    assert len(t.segments) == 4097 and set(np.diff(t.offsets.astype(np.int64)).tolist()) == {1, 2, 3}
    t = level_cases.sparsify_table("one matrix, two anchors")
    keep = t.law()[0]
    n = t.segments[0].size
    assert t.segments[0].matrix is t.segments[1].matrix and not np.any(keep[:n] & keep[n:]) and keep[n:].sum() > 1
    t = level_cases.sparsify_table("no non-zeros")
    assert t.segments[1].matrix.nnz == 0 and np.diff(t.law()[1].astype(np.int64)).tolist()[1:3] == [1, 1]
    t = level_cases.sparsify_table("all but the anchor cut")
    assert np.diff(t.law()[1].astype(np.int64)).tolist()[1] == 1 and t.segments[1].size == 70


@pytest.mark.parametrize("name", level_cases.EXTEND_NAMES)
def test_extend_law_is_the_single_law_segment_by_segment(name):
    t = level_cases.extend_table(name)
    states, out_offsets = t.law()
    assert out_offsets[0] == 0 and out_offsets.shape == (t.segments + 1,) and int(out_offsets[-1]) == states.size
    picked = range(t.segments) if t.segments < 100 else sorted(set(range(0, t.segments, 37)) | {1, 2, 4095, 4096})
    for g in picked:
        got = states[int(out_offsets[g]):int(out_offsets[g + 1])]
        assert np.array_equal(got, level_cases.extend_one(t.operator, t.segment(g))), (name, g)
        assert got.size == 0 or np.all(got[1:] > got[:-1])
    if getattr(t.operator.basis, "group", None) is None:
        # (operator_cases.extend itself, on the plain-basis tables)
        g = int(np.argmax(np.diff(t.offsets.astype(np.int64))))
        want = operator_cases.extend(t.operator, t.segment(g), t.operator.basis.number_spins)
        assert np.array_equal(states[int(out_offsets[g]):int(out_offsets[g + 1])], want)


def test_the_symmetric_law_is_the_host_operator():
    """In a sector: np.unique of the host batched_apply's representatives, without the orbits of norm 0 — what
    common.extension_spins does for a foreign operator object."""
    reached = {}
    for name in ("kagome18 inversion -1, four clusters", "ring22 inversion -1, norm-0 targets"):
        t = level_cases.extend_table(name)
        group = t.operator.basis.group
        assert level_cases.drops(t.operator)
        reached[name] = []
        for g in range(t.segments):
            other = np.unique(t.operator.batched_apply(t.segment(g))[0][:, 0])
            want = other[group.state_info(other)[2] > 0]
            assert np.array_equal(level_cases.extend_one(t.operator, t.segment(g)), want)
            reached[name].append(bool(np.any(level_cases.targets(t.operator, t.segment(g)) == level_cases.no_state(t.operator))))
    # norm-0 targets at the end of the sorted targets of three segments, and none in the table's last
    assert reached["ring22 inversion -1, norm-0 targets"] == [True, True, True, False]


EXTEND_TELLS = {
    "the first-flag looks across a boundary": "two segments with the same single key",
    "one sort over the table": "segments of 0 1 2 63 64 65 keys",
    "norm 0 dropped only at the table's end": "ring22 inversion -1, norm-0 targets",
}


@pytest.mark.parametrize("variant", list(level_cases.EXTEND_VARIANTS))
def test_every_wrong_extend_variant_is_told_apart(variant):
    assert set(EXTEND_TELLS) == set(level_cases.EXTEND_VARIANTS)
    t = level_cases.extend_table(EXTEND_TELLS[variant])
    assert not level_cases.same_extension(t.law(**level_cases.EXTEND_VARIANTS[variant]), t.law())


def test_the_extend_tables_hold_what_their_names_say():
    t = level_cases.extend_table("segments of 0 1 2 63 64 65 keys")
    assert [np.unique(t.segment(g)).size for g in range(t.segments)] == [0, 1, 2, 63, 0, 64, 65]
    assert any(np.unique(t.segment(g)).size < t.segment(g).size and np.any(np.diff(t.segment(g).astype(np.int64)) < 0)
               for g in range(t.segments))
    t = level_cases.extend_table("two segments with the same single key")
    assert t.segment(0).tolist() == t.segment(1).tolist() and t.segment(0).size == 1
    t = level_cases.extend_table("ring64 bit 63")
    assert t.operator.basis.number_spins == 64 and np.any(t.keys >> np.uint64(63)) and t.segments > 1
    t = level_cases.extend_table("4097 segments of 1-3 keys")
    assert t.segments == 4097
    t = level_cases.extend_table("single-site flips")
    assert getattr(t.operator.basis, "group", None) is None
