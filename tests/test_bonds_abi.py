"""Bond statistics (include/asp.h: asp_bonds_*, asp_sector_bonds_create): what can be
checked without a device — the symbols, the header against the bindings, the layout of the summary, the
refusals that run before any device work, and that nothing falls back to the host."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -3
SYMBOLS = ("asp_bonds_create", "asp_bonds_set_signs", "asp_bonds_get_summary", "asp_bonds_rows",
           "asp_bonds_histogram", "asp_bonds_magnitudes", "asp_bonds_destroy", "asp_bonds_last_ms",
           "asp_sector_bonds_create")


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_symbols():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    header = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    p, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    assert re.search(r"int\s+asp_bonds_create\s*\(\s*uint64_t\s+num_spins\s*,\s*int64_t\s+const\s*\*\s*indptr\s*,"
                     r"\s*int32_t\s+const\s*\*\s*indices\s*,\s*double\s+const\s*\*\s*data\s*,"
                     r"\s*uint64_t\s+const\s*\*\s*sign_words\s*,\s*asp_bonds\s*\*\*\s*out\s*\)\s*;", header)
    assert re.search(r"int\s+asp_sector_bonds_create\s*\(\s*uint64_t\s+n\s*,\s*uint32_t\s+width\s*,"
                     r"\s*uint32_t\s+const\s*\*\s*idx_dev\s*,\s*double\s+const\s*\*\s*val_dev\s*,"
                     r"\s*double\s+const\s*\*\s*psi_dev\s*,\s*asp_bonds\s*\*\*\s*out\s*\)\s*;", header)
    assert re.search(r"float\s+asp_bonds_last_ms\s*\(\s*void\s*\)\s*;", header)
    assert _lib.SIGNATURES["asp_bonds_create"] == (ctypes.c_int, [u64, p, p, p, p, ctypes.POINTER(p)])
    assert _lib.SIGNATURES["asp_bonds_set_signs"] == (ctypes.c_int, [p, p])
    assert _lib.SIGNATURES["asp_bonds_rows"] == (ctypes.c_int, [p, p, p, p])
    assert _lib.SIGNATURES["asp_bonds_histogram"][1][:5] == [p, u32, p, p, p]
    assert _lib.SIGNATURES["asp_bonds_magnitudes"] == (ctypes.c_int, [p, u64, p])
    assert _lib.SIGNATURES["asp_bonds_destroy"] == (None, [p])
    assert _lib.SIGNATURES["asp_bonds_last_ms"] == (ctypes.c_float, [])
    assert _lib.SIGNATURES["asp_sector_bonds_create"] == (ctypes.c_int, [u64, u32, p, p, p, ctypes.POINTER(p)])


def test_summary_mirror_has_the_headers_order_and_size():
    from annealing_sign_problem_amd import _lib

    body = re.search(r"typedef\s+struct\s+asp_bonds_summary\s*\{(.*?)\}\s*asp_bonds_summary\s*;", _header(), flags=re.S)
    assert body
    declared = []
    for ctype, names in re.findall(r"(uint64_t|double)\s+([^;]+);", body.group(1)):
        declared += [(name.strip(), ctype) for name in names.split(",")]
    mirror = [(name, {ctypes.c_uint64: "uint64_t", ctypes.c_double: "double"}[kind])
              for name, kind in _lib.BondsSummary._fields_]
    assert declared == mirror and len(declared) == 8
    assert ctypes.sizeof(_lib.BondsSummary) == 64
    assert [getattr(_lib.BondsSummary, name).offset for name, _ in mirror] == list(range(0, 64, 8))


def test_null_arguments_are_invalid_without_a_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = lib.asp_device_touched()
    edges = np.array([1.0, 2.0])
    counts = np.zeros(1, dtype=np.uint64)
    assert lib.asp_bonds_set_signs(None, None) == INVALID
    assert b"null bonds handle" in lib.asp_last_error()
    assert lib.asp_bonds_get_summary(None, ctypes.byref(_lib.BondsSummary())) == INVALID
    assert lib.asp_bonds_rows(None, None, None, None) == INVALID
    assert lib.asp_bonds_histogram(None, 1, _lib.ptr(edges), _lib.ptr(counts), _lib.ptr(counts), None, None) == INVALID
    assert lib.asp_bonds_magnitudes(None, ctypes.c_uint64(0), None) == INVALID
    assert lib.asp_bonds_create(ctypes.c_uint64(0), None, None, None, None, None) == INVALID
    assert lib.asp_sector_bonds_create(ctypes.c_uint64(0), 0, None, None, None, None) == INVALID
    lib.asp_bonds_destroy(None)
    assert lib.asp_device_touched() == touched  # refused before any device work


def test_python_surface():
    from annealing_sign_problem_amd import bonds, common, coupling_analysis

    assert list(inspect.signature(bonds.BondStatistics.__init__).parameters) == ["self", "exchange", "sign_bits"]
    assert list(inspect.signature(bonds.BondStatistics.from_sector).parameters) == ["matrix", "psi"]
    for member in ("summary", "rows", "histogram", "magnitudes", "set_signs", "release", "__enter__", "__exit__"):
        assert hasattr(bonds.BondStatistics, member), member
    assert list(inspect.signature(bonds.log_edges).parameters) == ["lo", "hi", "count"]
    parameters = inspect.signature(common.probability_of_frustration).parameters
    assert list(parameters) == ["model", "signs", "bins", "span", "min_count"]
    assert (parameters["signs"].default, parameters["bins"].default, parameters["span"].default,
            parameters["min_count"].default) == (None, 50, 20.0, 100)
    assert list(inspect.signature(common.coupling_distribution).parameters) == ["model"]
    assert list(inspect.signature(common.cluster_statistics).parameters) == ["spins", "quantum_hamiltonian", "ground_state"]
    for name in ("cluster_statistics", "coupling_distribution", "probability_of_frustration"):
        assert name in common.__all__
    assert callable(coupling_analysis.main)
    # host-side validation runs before the device is asked for
    with pytest.raises(ValueError):
        bonds.BondStatistics(scipy.sparse.csr_matrix(np.ones((2, 3))), np.zeros(1, dtype=np.uint64))
    with pytest.raises(ValueError):
        bonds.BondStatistics(scipy.sparse.identity(65, format="csr"), np.zeros(1, dtype=np.uint64))


def test_no_host_fallback():
    """Without a GPU the constructor fails with AspError (no device); with one it computes."""
    # in a child: asking for the device marks a process for good (asp_device_touched), and later tests
    # of this session fork workers only from a process that never did
    script = (
        "import numpy as np, scipy.sparse\n"
        "from annealing_sign_problem_amd import _lib, bonds\n"
        "matrix = scipy.sparse.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))\n"
        "bits = np.array([3], dtype=np.uint64)\n"
        "if _lib.device_count() > 0:\n"
        "    with bonds.BondStatistics(matrix, bits) as stats:\n"
        "        assert stats.summary['bonds'] == 2 and stats.summary['frustrated'] == 2\n"
        "    print('computed')\n"
        "else:\n"
        "    try:\n"
        "        bonds.BondStatistics(matrix, bits)\n"
        "    except _lib.AspError as error:\n"
        "        assert error.code == -1\n"
        "        print('refused')\n"
    )
    done = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split()[-1:] in (["computed"], ["refused"])
