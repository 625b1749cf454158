"""Bond statistics of an Ising model on the GPU (csrc/bond_stats.hip, specification ASP-BONDS-1 in
DESIGN.md §3.6): how many couplings are frustrated, how strong they are, and how the couplings are
distributed — what the reference's ``cluster_statistics``, ``analyze_probability_of_frustration`` and
``analyze_coupling_distribution`` (common.py:439-478, 963-1002, 940-960) compute with scipy on the host.

A *bond* is a stored entry ``J_ij`` with ``j != i`` and ``J_ij != 0`` (``(i, j)`` and ``(j, i)`` are two
bonds, as in the reference's ``tocoo()``); it is *frustrated* iff ``J_ij s_i s_j > 0``.  The matrix stays
on the device in a :class:`BondStatistics`; every result is exact.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np
import scipy.sparse

from . import _lib

__all__ = ["BondStatistics", "log_edges", "MAX_BINS"]

MAX_BINS = 4096


def log_edges(lo: float, hi: float, count: int) -> np.ndarray:
    """Value-space edges of the reference's log-space bins ``b = np.linspace(lo, hi, count)``
    (common.py:992): for every ``b`` the smallest double ``x`` with ``np.log(x) >= b``.  ``np.log`` is
    monotone, so ``edges[k] <= x`` is ``b[k] <= np.log(x)`` for every double x, and a histogram of
    ``|J|`` over these edges is ``np.histogram(np.log(|J|), b)``.  The LAST edge closes its bin from the
    right, where that rule is ``np.log(x) <= b``: several doubles share one logarithm, so the last edge
    is moved up to the largest of them (``np.log(max|J|)`` is the reference's last edge, and ``max|J|``
    need not be the smallest double with that logarithm)."""
    targets = np.linspace(lo, hi, count)
    edges = np.exp(targets)
    for k, b in enumerate(targets):
        x = edges[k]
        while np.log(x) < b:
            x = np.nextafter(x, np.inf)
        while True:
            below = np.nextafter(x, 0.0)
            if not (below > 0.0 and np.log(below) >= b):
                break
            x = below
        edges[k] = x
    if count > 0:
        x, b = edges[-1], targets[-1]
        while True:
            above = np.nextafter(x, np.inf)
            if not (np.isfinite(above) and np.log(above) <= b):
                break
            x = above
        edges[-1] = x
    return edges


class BondStatistics:
    """``exchange``: a square scipy sparse matrix (any format; duplicates are summed), an
    ``annealer.Hamiltonian``, or a tuple ``(indptr, indices, data)`` of CSR arrays that is handed over as
    it is (columns of a row unique, in any order; zeros and the diagonal may be stored); ``sign_bits``:
    the packed signs (``annealer.signs_to_bits``: bit set, ``s_i = +1``).  A context manager;
    :meth:`release` frees the device copy.

    ``summary`` is a dict of ``num_spins``, ``stored``, ``bonds``, ``frustrated``, ``rows_with_bonds``,
    ``strongest_frustrated`` (rows whose strongest bond is frustrated), ``max_abs`` and ``min_abs``."""

    def __init__(self, exchange, sign_bits):
        matrix = getattr(exchange, "exchange", exchange)
        if isinstance(matrix, tuple):  # raw CSR arrays, handed over as they are
            indptr, indices, data = matrix
            n = len(indptr) - 1
            if n < 0:
                raise ValueError("'indptr' is empty")
        else:
            if not (scipy.sparse.isspmatrix_csr(matrix) and matrix.has_canonical_format):
                matrix = scipy.sparse.csr_matrix(matrix, dtype=np.float64, copy=True)
                matrix.sum_duplicates()
            if matrix.shape[0] != matrix.shape[1]:
                raise ValueError("'exchange' must be square, got {}".format(matrix.shape))
            n = matrix.shape[0]
            indptr, indices, data = matrix.indptr, matrix.indices, matrix.data
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if indices.shape != data.shape or (n and indices.shape[0] < indptr[-1]):
            raise ValueError("'indices' and 'data' do not hold indptr[-1] entries")
        bits = self._words(sign_bits, n)
        lib = _lib.load()
        _lib.require_gpu()
        handle = ctypes.c_void_p()
        _lib.check(lib.asp_bonds_create(ctypes.c_uint64(n), _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                        _lib.ptr(bits), ctypes.byref(handle)))
        self._adopt(handle, n)

    @classmethod
    def from_sector(cls, matrix, psi) -> "BondStatistics":
        """The Ising model of a whole symmetry sector, built on the device from a
        ``sector_ed.SectorMatrix`` and its ground state (a device f64 tensor, as
        ``sector_ed.lanczos_ground_state`` returns it): nothing of it goes through the host."""
        import torch

        if psi.dtype != torch.float64 or not psi.is_cuda or not psi.is_contiguous() or psi.shape != (matrix.n,):
            raise ValueError("psi must be a contiguous f64 device vector of the sector's dimension")
        lib = _lib.load()
        _lib.require_gpu()
        torch.cuda.synchronize()  # the library runs on a stream of its own
        handle = ctypes.c_void_p()
        _lib.check(lib.asp_sector_bonds_create(ctypes.c_uint64(matrix.n), ctypes.c_uint32(matrix.width),
                                               ctypes.c_void_p(matrix.idx.data_ptr()),
                                               ctypes.c_void_p(matrix.val.data_ptr()),
                                               ctypes.c_void_p(psi.data_ptr()), ctypes.byref(handle)))
        self = cls.__new__(cls)
        self._adopt(handle, matrix.n)
        return self

    def _adopt(self, handle, n: int) -> None:
        self._lib_module = _lib
        self._handle = handle
        self.size = int(n)
        self.create_ms = float(_lib.load().asp_bonds_last_ms())
        _lib.track(self)

    @staticmethod
    def _words(sign_bits, n: int) -> np.ndarray:
        bits = np.ascontiguousarray(sign_bits, dtype=np.uint64).reshape(-1)
        words = (n + 63) // 64
        if bits.shape[0] < words:
            raise ValueError("'sign_bits' holds fewer than {} spins".format(n))
        return bits[:words] if words else np.zeros(1, dtype=np.uint64)

    def _live(self):
        if not getattr(self, "_handle", None):
            raise ValueError("this BondStatistics was released")
        return self._handle

    @property
    def summary(self) -> dict:
        out = _lib.BondsSummary()
        _lib.check(_lib.load().asp_bonds_get_summary(self._live(), ctypes.byref(out)))
        return {name: getattr(out, name) for name, _ in _lib.BondsSummary._fields_}

    def set_signs(self, sign_bits) -> "BondStatistics":
        """Other signs on the resident matrix (the row pass runs again)."""
        bits = self._words(sign_bits, self.size)
        _lib.check(_lib.load().asp_bonds_set_signs(self._live(), _lib.ptr(bits)))
        return self

    def rows(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(strongest f64[K], strongest_col i32[K], strongest_frustrated bool[K])``: per row the
        largest ``|J_ij|``, ``j != i`` (0 without a bond; ``common.get_strongest_off_diag``), the smallest
        column that attains it (-1 without) and whether that bond is frustrated."""
        n = self.size
        strongest = np.zeros(n, dtype=np.float64)
        col = np.zeros(n, dtype=np.int32)
        frustrated = np.zeros(n, dtype=np.uint8)
        _lib.check(_lib.load().asp_bonds_rows(self._live(), _lib.ptr(strongest), _lib.ptr(col), _lib.ptr(frustrated)))
        return strongest, col, frustrated.astype(bool)

    def histogram(self, edges):
        """``(normal u64[nb], frustrated u64[nb], below, above)`` over ``edges[nb + 1]`` (strictly
        ascending, ``1 <= nb <= 4096``) with ``np.histogram``'s bins of ``|J|``: half-open, the last one
        closed; ``below`` and ``above`` count the bonds outside the edges."""
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        nb = max(edges.shape[0] - 1, 0)
        normal = np.zeros(max(nb, 1), dtype=np.uint64)
        frustrated = np.zeros(max(nb, 1), dtype=np.uint64)
        below, above = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(_lib.load().asp_bonds_histogram(self._live(), ctypes.c_uint32(min(nb, 0xFFFFFFFF)), _lib.ptr(edges),
                                                   _lib.ptr(normal), _lib.ptr(frustrated), ctypes.byref(below),
                                                   ctypes.byref(above)))
        return normal[:nb], frustrated[:nb], int(below.value), int(above.value)

    def magnitudes(self) -> np.ndarray:
        """``|J|`` of all bonds, descending: ``np.sort(np.abs(bonds))[::-1]`` bit for bit."""
        bonds = self.summary["bonds"]
        out = np.zeros(max(bonds, 1), dtype=np.float64)
        _lib.check(_lib.load().asp_bonds_magnitudes(self._live(), ctypes.c_uint64(bonds), _lib.ptr(out)))
        return out[:bonds]

    @staticmethod
    def last_ms() -> float:
        """Device time (ms) of this thread's last create, set_signs, histogram or magnitudes."""
        return float(_lib.load().asp_bonds_last_ms())

    def release(self) -> None:
        handle, self._handle = getattr(self, "_handle", None), None
        if handle:
            self._lib_module.load().asp_bonds_destroy(handle)

    def __enter__(self) -> "BondStatistics":
        return self

    def __exit__(self, *exc) -> None:
        self.release()

    def __del__(self):
        module = getattr(self, "_lib_module", None)
        if module is not None and getattr(self, "_handle", None) and not module.closed():
            try:
                self.release()
            except Exception:
                pass
