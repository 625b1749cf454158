"""The law of tests/ising_segment_cases.py (ASP-ISING-SEG-1) without a device: for a single segment
it is the stored output of the reference function, bit for bit; concatenation and rebasing are consistent; every
case has something to compute."""
import numpy as np
import pytest

import ising_segment_cases as cases
from conftest import golden


@pytest.mark.parametrize("name", sorted(cases.GOLDEN))
def test_one_segment_is_the_stored_output_of_the_reference_function(name):
    g = golden(name)
    keys, psi = cases.golden_cluster(g)
    op = cases.GOLDEN[name]()
    indptr, col, val = cases.ising_segments_law(op, keys, psi, np.array([0, keys.size]))
    row = np.repeat(np.arange(keys.size, dtype=np.int32), np.diff(indptr))
    assert indptr[0] == 0 and indptr[-1] == g["data"].shape[0]
    assert np.array_equal(row, g["row"]) and np.array_equal(col, g["col"])
    assert cases.same_bits(val, g["data"])
    # the same cluster after an empty segment and twice (only |psi| enters): its rows rebased, its columns local
    offsets = np.array([0, 0, keys.size, 2 * keys.size])
    whole = cases.ising_segments_law(op, np.concatenate([keys, keys]), np.concatenate([psi, -psi]), offsets)
    for g_index in (1, 2):
        assert cases.equal(cases.rebased(*whole, offsets, g_index), (indptr, col, val))
    assert cases.rebased(*whole, offsets, 0)[0].tolist() == [0]


@pytest.mark.parametrize("name", ["three segments", "empty segments", "segments of 2 3 5", "kagome18 inversion -1"])
def test_concatenation_and_rebasing_are_consistent(name):
    c = cases.case(name)
    indptr, col, val = c.law()
    offsets = c.offsets.astype(np.int64)
    assert indptr.shape == (c.keys.size + 1,) and indptr[0] == 0 and np.all(np.diff(indptr) >= 0)
    assert indptr[-1] == col.size == val.size and col.dtype == np.int32 and indptr.dtype == np.int64
    for g in range(c.segments):
        lo, hi = offsets[g], offsets[g + 1]
        part = cases.rebased(indptr, col, val, offsets, g)
        assert cases.equal(part, cases.segment_csr(c.operator, c.keys[lo:hi], c.psi[lo:hi]))
        assert part[1].size == 0 or (part[1].min() >= 0 and part[1].max() < hi - lo)  # segment-local columns
        for r in range(hi - lo):  # canonical: ascending, no duplicates
            assert np.all(np.diff(part[1][part[0][r]:part[0][r + 1]]) > 0)
    # the segments back together
    parts = [cases.rebased(indptr, col, val, offsets, g) for g in range(c.segments)]
    assert cases.equal(cases.concatenate(parts, np.diff(offsets)), (indptr, col, val))


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_has_a_segment_and_a_coupling(name):
    c = cases.case(name)
    offsets = c.offsets.astype(np.int64)
    assert offsets[0] == 0 and offsets[-1] == c.keys.size == c.psi.size and np.any(np.diff(offsets) > 0)
    for g in range(c.segments):
        keys = c.keys[offsets[g]:offsets[g + 1]]
        assert keys.size < 2 or np.all(keys[1:] > keys[:-1])
        if keys.size:
            assert abs(np.linalg.norm(c.psi[offsets[g]:offsets[g + 1]]) - 1.0) < 1e-12
    indptr, col, val = c.law()
    assert val.size >= 1 and np.all(val != 0)


def test_the_cases_cover_what_the_kernels_distinguish():
    sizes = {int(cases.case("kagome16 grown K=%d" % k).keys.size) for k in cases.SIZES}
    assert sizes == {1, 2, 3, 5, 63, 64, 65, 301, 4097}
    assert cases.case("4097 segments of 1-3 keys").segments == 4097
    empty = np.diff(cases.case("empty segments").offsets.astype(np.int64)) == 0
    assert empty[0] and empty[-1] and np.any(empty[1:-1][:-1] & empty[1:-1][1:])
    assert cases.case("one state in 300 segments").segments == 300
    assert np.diff(cases.case("three segments").offsets.astype(np.int64)).tolist() == [5, 70, 130]
    assert np.diff(cases.case("segments of 2 3 5").offsets.astype(np.int64)).tolist() == [2, 3, 5, 2, 3, 5]
    assert int(cases.case("ring64 bit 63").keys.max()) >> 63 == 1
    # one-directional matrix elements: a single key, an empty segment, then the cluster
    for name in ("one-directional, one_way", cases.ONE_WAY_WITH_DUPLICATES):
        assert np.diff(cases.case(name).offsets.astype(np.int64)).tolist() == [1, 0, 120]
    # rows longer than max_connections = 1 + 7 allows: the state 0 is reached from three states per bond
    wide = cases.case("one-directional, wide rows")
    assert int(wide.keys[0]) == 0 and np.diff(wide.law()[0])[0] == 1 + 3 * cases.WIDE_BONDS
    # awkward amplitudes prune and keep entries
    t = cases.case("three segments")
    awkward = cases.awkward_amplitudes(t.keys.size)
    assert t.law(psi=awkward)[2].size < t.law()[2].size
