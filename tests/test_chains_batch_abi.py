"""asp_sa_chains_advance_batch (include/asp.h section 4): what can be checked
without a device — the symbols, the header, the struct mirror and the validation that runs before
any device work."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_batched_advance():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in ("asp_sa_chains_advance_batch", "asp_sa_chains_batch_last_ms"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header)
    assert re.search(r"int\s+asp_sa_chains_advance_batch\s*\(\s*asp_sa_chains_item\s+const\s*\*\s*items\s*,"
                     r"\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"float\s+asp_sa_chains_batch_last_ms\s*\(\s*void\s*\)\s*;", header)


def test_struct_mirror_has_the_headers_field_order_and_size():
    from annealing_sign_problem_amd import _lib

    body = re.search(r"typedef struct asp_sa_chains_item \{(.*?)\} asp_sa_chains_item;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in body.split(";") if part.strip()]
    assert fields == ["chains", "betas", "num_sweeps", "order", "flags", "out_trace", "out_tracked_best",
                      "out_improved"]
    assert [name for name, _ in _lib.SaChainsItem._fields_] == fields
    # LP64: two pointers, three 32-bit words padded to the next pointer, three pointers
    assert ctypes.sizeof(_lib.SaChainsItem) == 8 + 8 + 3 * 4 + 4 + 3 * 8 == 56
    assert _lib.SaChainsItem.num_sweeps.offset == 16 and _lib.SaChainsItem.out_trace.offset == 32


def test_count_zero_and_null_arguments_need_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    assert lib.asp_sa_chains_advance_batch(None, ctypes.c_uint32(0)) == 0
    items = (_lib.SaChainsItem * 2)()
    assert lib.asp_sa_chains_advance_batch(items, ctypes.c_uint32(0)) == 0
    assert lib.asp_sa_chains_batch_last_ms() == 0.0
    assert lib.asp_sa_chains_advance_batch(None, ctypes.c_uint32(1)) == INVALID
    assert "null items" in _lib.last_error()
    # a null handle: the item's index is in the message, and no output is touched
    best = np.full(4, -77, dtype=np.int64)
    improved = ctypes.c_uint32(12345)
    for k in range(2):
        items[k].out_tracked_best = best.ctypes.data
        items[k].out_improved = ctypes.addressof(improved)
    assert lib.asp_sa_chains_advance_batch(items, ctypes.c_uint32(1)) == INVALID
    assert "item 0" in _lib.last_error() and "null" in _lib.last_error()
    assert np.all(best == -77) and improved.value == 12345
