"""The C ABI of the batched greedy solve without a device: the header declares the struct and the
symbols, the library exports them, the ctypes mirror has the header's field order and size, and an
empty batch is fine."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {
    "asp_sa_plan *": (ctypes.c_void_p, 8),
    "uint32_t": (ctypes.c_uint32, 4),
    "uint64_t *": (ctypes.c_void_p, 8),
    "double *": (ctypes.c_void_p, 8),
    "uint32_t *": (ctypes.c_void_p, 8),
}


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def _struct_fields(header):
    """[(C type, name)] of asp_sa_greedy_item as the header declares it."""
    body = re.search(r"typedef struct asp_sa_greedy_item \{(.*?)\} asp_sa_greedy_item;", header, flags=re.S)
    assert body, "include/asp.h does not declare asp_sa_greedy_item"
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for declaration in text.split(";"):
        declaration = " ".join(declaration.split())
        if not declaration:
            continue
        m = re.fullmatch(r"(.*?)(\w+)", declaration)
        fields.append((m.group(1).strip().replace(" *", " *"), m.group(2)))
    return fields


def test_header_declares_the_struct_and_the_entry_points():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert [name for _, name in _struct_fields(_header())] == [
        "plan", "max_sweeps", "flags", "out_x", "out_e", "out_sweeps"]
    assert re.search(r"\bint\s+asp_sa_greedy_batch\s*\(\s*asp_sa_greedy_item const \*items,\s*uint32_t count\s*\)\s*;",
                     header)
    assert re.search(r"\bint\s+asp_sa_greedy_batch_last_ms\s*\(", header)
    # asp_sa_batch_item keeps its layout: existing callers build it through ctypes
    body = re.search(r"typedef struct asp_sa_batch_item \{(.*?)\} asp_sa_batch_item;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == ["plan", "seed", "betas", "num_sweeps", "repetitions",
                                               "replica_offset", "flags", "out_x", "out_e"]


def test_library_exports_the_symbols():
    from annealing_sign_problem_amd import _lib

    for name in ("asp_sa_greedy_batch", "asp_sa_greedy_batch_last_ms"):
        assert name in _lib.SIGNATURES
    _lib.load()  # resolves every symbol of SIGNATURES or raises
    raw = ctypes.CDLL(_lib.library_path())
    assert raw.asp_sa_greedy_batch is not None and raw.asp_sa_greedy_batch_last_ms is not None


def test_ctypes_struct_mirrors_the_header():
    from annealing_sign_problem_amd import _lib

    declared = _struct_fields(_header())
    mirror = _lib.SaGreedyItem._fields_
    assert [name for name, _ in mirror] == [name for _, name in declared]
    offset = 0
    for (c_type, name), (_, py_type) in zip(declared, mirror):
        expected, size = C_TYPES[c_type]
        assert py_type is expected, (name, c_type, py_type)
        offset = (offset + size - 1) // size * size  # natural alignment
        assert getattr(_lib.SaGreedyItem, name).offset == offset, name
        offset += size
    assert ctypes.sizeof(_lib.SaGreedyItem) == (offset + 7) // 8 * 8 == 40
    signature = _lib.SIGNATURES["asp_sa_greedy_batch"]
    assert signature[0] is ctypes.c_int
    assert signature[1] == [ctypes.POINTER(_lib.SaGreedyItem), ctypes.c_uint32]


def test_empty_batch_is_ok_without_a_device():
    from annealing_sign_problem_amd import _lib, greedy

    lib = _lib.load()
    touched = _lib.gpu_touched()
    assert lib.asp_sa_greedy_batch(None, ctypes.c_uint32(0)) == 0
    items = (_lib.SaGreedyItem * 1)()
    assert lib.asp_sa_greedy_batch(items, ctypes.c_uint32(0)) == 0
    assert lib.asp_last_error_code() == 0
    assert greedy.greedy_solve_batch([]) == []
    assert greedy.greedy_solve_batch([], return_sweeps=True) == []
    assert _lib.gpu_touched() == touched  # the empty batch did not ask for the GPU
    # a non-empty batch is validated before the device is asked for: a null plan is named
    assert lib.asp_sa_greedy_batch(items, ctypes.c_uint32(1)) == -3
    assert "item 0" in _lib.last_error()
    assert _lib.gpu_touched() == touched
