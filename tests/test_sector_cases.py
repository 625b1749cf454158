"""The table of tests/sector_cases.py still reaches what it claims to reach — asserted from the
host objects alone (no GPU, nothing compiled), so that tests/test_gpu_sector_widths.py cannot lose
its point silently when a case is edited.  The sizing rules of csrc/sector_basis.hip and
csrc/plain_basis.hip are restated in sector_cases as plain arithmetic."""
import numpy as np

import sector_cases as cases


def _permutations(case):
    return cases.host(case).group.permutations.astype(np.int64)


def test_case_names_are_unique_and_every_case_states_its_purpose():
    table = cases.SECTOR_CASES + cases.ENUMERATION_CASES + cases.PLAIN_CASES
    assert len({case.name for case in table}) == len(table)
    assert all(case.reaches for case in table)


def test_sector_cases_reach_all_three_filter_passes(models):
    """asp_sector_enumerate filters with elements [0, 9), [9, 41), [41, P)."""
    sizes = {case.name: _permutations(case).shape[0] for case in cases.SECTOR_CASES}
    assert sizes["ring22 half filling, inversion -1"] == 44 and sizes["ring44 weight 3"] == 88
    assert sizes["kagome_36 weight 4"] == 144 and sizes["pyrochlore weight 4"] == 384
    assert sum(p > 41 for p in sizes.values()) >= 6
    # two passes only: the 12-site rings here, and the rings of tests/test_gpu_sector.py
    assert sizes["ring12 any magnetisation, field on all bonds"] == 24
    import test_gpu_sector

    existing = {name: op.basis.group.num_permutations for name, op in test_gpu_sector._cases(models)
                if op.basis.group is not None}
    assert existing["ring16 even"] == 32 and existing["ring20 no inversion"] == 40
    assert existing["ring12 any magnetisation"] == 24
    assert all(p <= 41 for p in existing.values())   # why this table exists


def test_sector_cases_move_sites_across_the_32_bit_boundary_and_exceed_40_sites():
    """permuted() moves a state as two 32-bit halves; lo_bits is clamped to 20 beyond 40 sites."""
    crossing = []
    for case in cases.SECTOR_CASES:
        p = _permutations(case)[1:]                   # the non-identity elements
        site = np.arange(p.shape[1])[None, :]
        down = bool(np.any((site >= 32) & (p < 32)))  # a site of the high half lands in the low one
        up = bool(np.any((site < 32) & (p >= 32)))
        if down and up:
            crossing.append(case.name)
    assert {"ring44 weight 3", "ring48 weight 3", "kagome_36 weight 4"} <= set(crossing)
    wide = {case.name: cases.sector_word_bits(cases.host(case).operator.basis.number_spins)
            for case in cases.SECTOR_CASES if cases.host(case).operator.basis.number_spins > 40}
    assert wide == {"ring44 weight 3": (20, 24), "ring48 weight 3": (20, 28)}
    assert cases.sector_word_bits(36) == (18, 18) and cases.sector_word_bits(20) == (10, 10)


def test_sector_cases_fill_the_second_mask_word_and_flip_single_sites():
    """k_sector_rows keeps a row's transitions in two 64-bit words; asp_sector_rows takes 128."""
    count = {case.name: cases.transitions(cases.host(case).operator) for case in cases.SECTOR_CASES}
    assert len(count["kagome_36 weight 4"]) == 72 and len(count["pyrochlore weight 4"]) == 96
    assert all(len(t) <= 128 for t in count.values())
    both = count["ring12 any magnetisation, field on all bonds"]
    assert len(both) == 72
    # single-site flips below AND above transition 64
    assert {1, 2} <= set(both[:64]) and {1, 2} <= set(both[64:])
    nearest = count["ring12 any magnetisation, field on nearest bonds"]
    assert len(nearest) == 48 and {1, 2} <= set(nearest)
    # a row does take transitions of the second word: some state flips a bond listed beyond 64
    for name in ("kagome_36 weight 4", "pyrochlore weight 4"):
        reference = cases.host({c.name: c for c in cases.SECTOR_CASES}[name])
        sites = [s for term in reference.operator.terms for s in term.sites][64:]
        states = reference.states
        assert any(np.any(((states >> np.uint64(a)) ^ (states >> np.uint64(b))) & np.uint64(1)) for a, b in sites)


def test_sector_cases_hold_orbits_of_zero_norm_and_unequal_norms():
    by_name = {case.name: case for case in cases.SECTOR_CASES}
    odd = cases.host(by_name["ring22 half filling, inversion -1"])
    even = cases.host(by_name["ring22 half filling, inversion +1"])
    # the orbit minima are the same for both characters; with -1 some of them have norm 0
    assert odd.states.shape[0] == 7800 and even.states.shape[0] > odd.states.shape[0]
    assert np.all(np.isin(odd.states, even.states))
    for reference in (odd, even):
        assert np.all(reference.norms > 0)
        assert np.unique(reference.norms).shape[0] > 1    # stabilisers larger than 1
    # ... and spin inversion away from half filling drops states whose inverted orbit is smaller
    for case in cases.ENUMERATION_CASES:
        reference = cases.host(case)
        basis = reference.operator.basis
        assert basis.hamming_weight * 2 != basis.number_spins and reference.group.spin_inversion != 0
        lattice_only = cases.ring(basis.number_spins, basis.hamming_weight, None).basis
        lattice_only.build()
        assert 0 < reference.states.shape[0] < lattice_only.number_states, case.name


def test_plain_cases_reach_the_wide_words_the_long_classes_and_every_bond_kind():
    from math import comb

    kinds = set()
    populated_beyond_a_workgroup = []
    high_words_beyond_16_bits = []
    narrow = set()
    for case in cases.PLAIN_CASES:
        reference = cases.host(case)
        basis = reference.operator.basis
        n, w = basis.number_spins, basis.hamming_weight
        assert reference.group is None and w is not None
        assert reference.states.shape[0] == comb(n, w), case.name
        lo_bits, hi_bits = cases.plain_word_bits(n)
        kinds |= {cases.plain_bond_kind(a, b, lo_bits) for t in reference.operator.terms for a, b in t.sites}
        # the populated low classes: k = w - popcount(high word) for some high word
        classes = [k for k in range(lo_bits + 1) if 0 <= w - k <= hi_bits]
        if lo_bits == 16 and max(comb(lo_bits, k) for k in classes) > 1024:
            populated_beyond_a_workgroup.append(case.name)
        if hi_bits > 16:
            high_words_beyond_16_bits.append((case.name, hi_bits))
        if lo_bits < 8:
            narrow.add(lo_bits)
        # the two-level rank stays inside its 16 bits
        assert max(comb(lo_bits, k) for k in range(lo_bits + 1)) <= 0xFFFF
    assert kinds == {0, 1, 2, 3}
    assert populated_beyond_a_workgroup == ["sk_32_1 weight 4", "kagome_36 bonds weight 4"]
    assert high_words_beyond_16_bits == [("kagome_36 bonds weight 4", 20), ("chain33 weight 3", 17),
                                         ("chain35 weight 3", 19)]
    assert narrow == {1, 2, 3, 5, 7}
    sizes = {case.name: cases.host(case).states.shape[0] for case in cases.LARGE_PLAIN_CASES}
    assert sizes == {"sk_32_1 weight 4": 35960, "kagome_36 bonds weight 4": 58905}
    # the one-state ends of every small chain
    ends = [case for case in cases.SMALL_PLAIN_CASES if cases.host(case).states.shape[0] == 1]
    assert len(ends) == 2 * 5


def test_sk_32_bonds_are_listed_in_the_order_the_kernel_adds_them(models):
    """(see sector_cases.sk_32_at_weight_4) the same 496 bonds as the model, regrouped."""
    reference = cases.host(cases.LARGE_PLAIN_CASES[0])
    mine = sorted((s, t.matrix.real.tobytes()) for t in reference.operator.terms for s in t.sites)
    model = sorted((tuple(s), np.asarray(t["matrix"], dtype=np.float64).tobytes())
                   for t in models["sk_32_1"]["hamiltonian"]["terms"] for s in t["sites"])
    assert mine == model and len(mine) == 496
    key = {0: 0, 1: 1, 2: 1, 3: 2}
    order = [key[cases.plain_bond_kind(a, b, 16)] for t in reference.operator.terms for a, b in t.sites]
    assert order == sorted(order) and set(order) == {0, 1, 2}


def test_every_host_matrix_is_real_and_symmetric():
    """The sector matrices are compared with the TRANSPOSE of `to_sparse` (an ELL row holds a
    column), so the host matrix's own asymmetry — about 1e-15 of rounding in
    (c * (chi * norm)) / norm — has to stay far below the comparison's 1e-13."""
    for case in cases.SECTOR_CASES + cases.PLAIN_CASES:
        reference = cases.host(case)
        assert reference.imaginary == 0.0, case.name
        h = reference.h
        asymmetry = abs(h - h.T).max() if h.nnz else 0.0
        assert asymmetry <= 1e-12 * reference.largest, (case.name, asymmetry)
        # the slot counts describe the same connections as the matrix
        assert reference.filled.shape == (h.shape[0],) and reference.filled.sum() + h.shape[0] >= h.nnz


def test_the_field_operators_are_hermitian_and_invariant_under_their_group():
    """The 12-site rings in a transverse field, in the full space of 2^12 states: H = H^T, and
    H commutes with every lattice map and with global spin inversion."""
    from annealing_sign_problem_amd import operators

    for case in cases.SECTOR_CASES[-2:]:
        reference = cases.host(case)
        assert reference.operator.basis.hamming_weight is None and reference.group.spin_inversion == 1
        full = operators.Operator(operators.SpinBasis(12), reference.operator.terms)
        full.basis.build()
        h = full.to_sparse()
        assert abs(h.imag).max() == 0
        h = h.real.tocsr()
        scale = abs(h).max()
        assert abs(h - h.T).max() <= 1e-12 * scale, case.name
        states = full.basis.states
        assert np.array_equal(states, np.arange(4096, dtype=np.uint64))
        images = reference.group.images(states).astype(np.int64)
        maps = list(images[1:]) + [(~states & reference.group.mask).astype(np.int64)]
        assert len(maps) == 24
        for image in maps:
            # <g s'| H |g s> = <s'| H |s>
            assert abs(h[image][:, image] - h).max() <= 1e-12 * scale, case.name
        # ... and it does flip single sites: it connects different magnetisations
        weight = np.array([bin(int(s)).count("1") for s in states])
        coo = h.tocoo()
        assert np.any(np.abs(weight[coo.row] - weight[coo.col]) == 1)
