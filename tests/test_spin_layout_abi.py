"""The per-plan limit for the spin layout and the report of the layout that ran (include/asp.h:
asp_sa_set_lds_limit, asp_sa_last_spin_layout): what can be checked without a
device — the symbols, the header against the bindings and the null-plan refusals that run before any
device work."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_sa_set_lds_limit", "asp_sa_last_spin_layout")


def test_library_exports_and_header_declares_the_two_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int\s+asp_sa_set_lds_limit\s*\(\s*asp_sa_plan\s*\*\s*p\s*,\s*uint64_t\s+bytes\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sa_last_spin_layout\s*\(\s*asp_sa_plan\s+const\s*\*\s*p\s*\)\s*;", header)
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_sa_set_lds_limit"] == (ctypes.c_int, [p, u64])
    assert _lib.SIGNATURES["asp_sa_last_spin_layout"] == (ctypes.c_int, [p])
    # the layout report the new one sits beside keeps its declaration
    assert re.search(r"int\s+asp_sa_last_layout\s*\(\s*asp_sa_plan\s+const\s*\*\s*p\s*\)\s*;", header)
    assert _lib.SIGNATURES["asp_sa_last_layout"] == (ctypes.c_int, [p])


def test_header_names_every_layout_code_and_the_clone():
    """The codes of asp_sa_last_spin_layout are asp_sa_last_layout's, and the clone's comment lists the
    setting among those it copies."""
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        header = f.read()
    comment = header[:header.index("int asp_sa_last_spin_layout")].rsplit("/*", 1)[1]
    for code in ("0 bytes", "1 bits in LDS", "2 words", "3 words in HBM", "6 nibbles", "lane packing reports 2"):
        assert code in comment, code
    clone = header[:header.index("int asp_sa_plan_clone")].rsplit("/*", 1)[1]
    assert "_set_lds_limit" in clone


def test_null_plan_is_refused_without_a_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = lib.asp_device_touched()
    for limit in (0, 1, 4096, 2**64 - 1):
        assert lib.asp_sa_set_lds_limit(None, ctypes.c_uint64(limit)) == INVALID
        assert b"null plan" in lib.asp_last_error()
    assert lib.asp_sa_last_spin_layout(None) == -1
    assert lib.asp_sa_last_layout(None) == -1
    assert lib.asp_device_touched() == touched  # refused before any device work
