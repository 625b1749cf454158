"""Population annealing on resumable chains (include/asp.h section 4, DESIGN.md §4.11, law ASP-PA-1):
what can be checked without a device — the symbols, the header, the struct mirror, the validation
that runs before any device work, and the properties of the law as tests/population_law.py restates it
(the checker of tests/test_gpu_population.py)."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import population_law as law

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_chains_gather", "asp_sa_chains_resample", "asp_sa_chains_resample_batch",
           "asp_sa_chains_resample_last_ms")


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_four_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"int\s+asp_sa_chains_gather\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*uint32_t\s+const\s*\*\s*source\s*\)\s*;",
                     header)
    assert re.search(r"int\s+asp_sa_chains_resample\s*\(\s*asp_sa_chains\s*\*\s*c\s*,\s*double\s+dbeta\s*,\s*uint32_t\s+draw\s*,"
                     r"\s*uint32_t\s*\*\s*out_source\s*,\s*double\s*\*\s*out_energy\s*,\s*uint64_t\s*\*\s*out_q\s*,"
                     r"\s*uint32_t\s*\*\s*out_survivors\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_chains_resample_batch\s*\(\s*asp_sa_chains_resample_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_chains_resample_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert _lib.SIGNATURES["asp_sa_chains_resample"][1][1] is ctypes.c_double
    assert _lib.SIGNATURES["asp_sa_chains_resample_last_ms"] == (ctypes.c_float, [])


def test_struct_mirror_has_the_headers_field_order_and_size():
    from annealing_sign_problem_amd import _lib

    body = re.search(r"typedef struct asp_sa_chains_resample_item \{(.*?)\} asp_sa_chains_resample_item;", _header(),
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in body.split(";") if part.strip()]
    assert fields == ["chains", "dbeta", "draw", "flags", "out_source", "out_energy", "out_q", "out_survivors"]
    assert [name for name, _ in _lib.SaChainsResampleItem._fields_] == fields
    # LP64: a pointer, a double, two 32-bit words, four pointers
    assert ctypes.sizeof(_lib.SaChainsResampleItem) == 8 + 8 + 2 * 4 + 4 * 8 == 56
    assert _lib.SaChainsResampleItem.draw.offset == 16 and _lib.SaChainsResampleItem.out_source.offset == 24


def test_python_surface():
    import inspect

    from annealing_sign_problem_amd import annealer as sa

    for name in ("resample_chains", "population_anneal", "population_anneal_batch"):
        assert name in sa.__all__ and callable(getattr(sa, name))
    assert callable(sa.Chains.gather) and callable(sa.Chains.resample)
    assert inspect.signature(sa.Chains.resample).parameters["draw"].default == 0
    assert inspect.signature(sa.resample_chains).parameters["draws"].default == 0
    parameters = inspect.signature(sa.population_anneal).parameters
    assert list(parameters) == ["hamiltonian", "seed", "number_steps", "sweeps_per_step", "beta0", "beta1",
                                "repetitions", "only_best", "sweep_order", "resample"]
    defaults = {k: p.default for k, p in parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(seed=None, number_steps=512, sweeps_per_step=10, beta0=None, beta1=None, repetitions=64,
                            only_best=True, sweep_order=None, resample=True)
    batch = inspect.signature(sa.population_anneal_batch).parameters
    assert list(batch)[0] == "hamiltonians" and list(batch)[1:] == list(parameters)[1:]


def test_count_zero_and_null_arguments_need_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    assert lib.asp_sa_chains_resample_batch(None, ctypes.c_uint32(0)) == 0
    items = (_lib.SaChainsResampleItem * 2)()
    assert lib.asp_sa_chains_resample_batch(items, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_resample_last_ms() == 0.0
    assert lib.asp_sa_chains_resample_batch(None, ctypes.c_uint32(1)) == INVALID
    assert "null items" in _lib.last_error()
    # a null handle: the item's index is in the message, and no output is touched
    source = np.full(4, 77, dtype=np.uint32)
    energy = np.full(4, -77.0)
    q = np.full(4, 77, dtype=np.uint64)
    survivors = ctypes.c_uint32(12345)
    for k in range(2):
        items[k].out_source = source.ctypes.data
        items[k].out_energy = energy.ctypes.data
        items[k].out_q = q.ctypes.data
        items[k].out_survivors = ctypes.addressof(survivors)
    assert lib.asp_sa_chains_resample_batch(items, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null" in _lib.last_error()
    assert lib.asp_sa_chains_resample(None, ctypes.c_double(0.0), ctypes.c_uint32(0), None, None, None, None) == INVALID
    assert "null" in _lib.last_error()
    assert lib.asp_sa_chains_gather(None, _lib.ptr(source)) == INVALID
    assert "null" in _lib.last_error()
    assert np.all(source == 77) and np.all(energy == -77.0) and np.all(q == 77) and survivors.value == 12345


def test_non_zero_flags_are_rejected_with_the_items_index():
    """An item's flags are looked at before its handle, so the check needs none (with a real handle:
    tests/test_gpu_population.py)."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    items = (_lib.SaChainsResampleItem * 2)()
    items[1].flags = 4
    assert lib.asp_sa_chains_resample_batch(items, ctypes.c_uint32(2)) == INVALID
    assert "item 0" in _lib.last_error() and "null chains handle" in _lib.last_error()
    items[0].flags = 1
    assert lib.asp_sa_chains_resample_batch(items, ctypes.c_uint32(2)) == INVALID
    assert "item 0" in _lib.last_error() and "flags" in _lib.last_error()


# ---- the restated law ------------------------------------------------------------------------------

SIZES = (1, 2, 3, 64, 257, 65536)


def _weights(R, kind, rng):
    if kind == "equal":
        return [2 ** 31] * R
    if kind == "one":  # one chain at the minimum, the others dead
        q = [0] * R
        q[int(rng.integers(R))] = 2 ** 31
        return q
    q = [int(x) for x in rng.integers(0, 2 ** 31, size=R, endpoint=True)]
    if kind == "sparse":
        q = [x if rng.random() < 0.1 else 0 for x in q]
    q[int(rng.integers(R))] = 2 ** 31  # (the best chain has w = 1)
    return q


@pytest.mark.parametrize("R", SIZES)
def test_law_properties(R):
    rng = np.random.default_rng(R)
    for kind in ("equal", "one", "random", "sparse"):
        q = _weights(R, kind, rng)
        T = sum(q)
        assert 2 ** 31 <= T and R * T <= 2 ** 63  # every product of the law fits 64 bits
        for v in (0, 2 ** 32 - 1, int(rng.integers(2 ** 32))):
            source, survivors = law.select(q, v)
            assert len(source) == R and all(0 <= s < R for s in source)
            assert all(a <= b for a, b in zip(source, source[1:]))  # sorted
            children = np.bincount(np.array(source), minlength=R)
            assert survivors == int(np.count_nonzero(children))
            for s in (range(R) if R <= 257 else rng.integers(R, size=200)):
                share = Fraction(R * q[s], T)
                assert math.floor(share) <= int(children[s]) <= math.ceil(share), (kind, v, s)
            assert all(children[s] == 0 for s in range(min(R, 300)) if q[s] == 0)
            if kind == "equal":
                assert source == list(range(R))  # equal weights: the identity
            if kind == "one":
                assert survivors == 1 and source == [q.index(2 ** 31)] * R


def test_law_weights_and_draw():
    import oracle

    # dbeta = 0: every weight is 1; a gap with dbeta * gap >= 23 is dead; the best chain is 2^31
    assert law.weights([3.0, -1.5, 7.25], 0.0) == [2 ** 31] * 3
    q = law.weights([0.0, 1.0, 20.0, 23.0, 1e9], 1.0)
    assert q[0] == 2 ** 31 and q[3] == 0 and q[4] == 0 and 0 < q[2] < q[1] < 2 ** 31
    assert q[1] == int(oracle.expneg(1.0) * 2.0 ** 31)
    # the draw: its own counter word, and every argument matters
    words = {law.draw_word(5, 0, 0), law.draw_word(5, 16, 0), law.draw_word(5, 0, 7), law.draw_word(6, 0, 0),
             law.draw_word(5 + 2 ** 32, 0, 0)}
    assert len(words) == 5
    assert law.DRAW_WORD >= 2 ** 30 and law.DRAW_WORD not in (0xFFFFFFFE, 0xFFFFFFFF)
    q, source, survivors = law.resample([1.0, 1.0, 1.0, 1.0], 3.0, 1, 0, 0)
    assert q.dtype == np.uint64 and source.dtype == np.uint32 and list(source) == [0, 1, 2, 3] and survivors == 4
